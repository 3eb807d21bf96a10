"""GPU: every tree shape of tests/crs_sweep.py through the .crs packer (k_emit / k_emit_long under GHF_EMIT_LONG_CODES), the
tree's decode tables (k_crs_decode_tables, dec_long, dec_long64 inside K7's hot variants and its one-symbol-at-a-time path)
and K6 on a .crs (whole bodies and bodies in pieces).

Nothing expected comes from the library: trees, codes, bodies, files, side-cars and every piece's (landing, n_symbols) are
the model's (tests/test_crs_sweep_cpu.py holds them to the oracle and to the compiled reference's own decoder).  A tree
reaches the device as ghf.crs_parse_header(model header) -> tree_to_device, so the host parser is swept too.  Every output
sits between guard bytes that are checked afterwards.

The ids are per depth, `len<max>-pack` and `len<max>-pieces` (`-a`, `-b`, .. where a depth's pieces are split; depths and
parts are pinned in tests/golden/golden_crs_sweep.json); a
failure names tree and item, e.g. `chain/fib/k40/first~mirror :: block/4097`: crs_sweep.pool() and crs_sweep.items() give
that case alone.  The run0 / run1 items of the combs of depth 16, 32 and 64 are the ones that K6 cannot settle by passes
alone (profiles/crs_sweep/README.md has the pass counts)."""
import json
import os

import numpy as np
import pytest

import crs_sweep as zs
import hist_families as hf
import pkgload
from guarded import GUARD, Arena, first_diff
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

E_FORMAT, E_CORRUPT = 6, 7
MAX_SYMBOLS = 6 * 4096  # a side-car slice for the longest item
CARS = 20               # slices: one per item of a tree
assert MAX_SYMBOLS >= zs.DRAWN_MAX
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_crs_sweep.json")) as _f:
    _pins = json.load(_f)
GROUPS = _pins["groups"]
# the pieces cost a host round trip each: a depth's (tree, item) pairs go into as many ids as test_crs_sweep_cpu pins
PIECE_IDS = [(d, k) for d, parts in zip(GROUPS, _pins["piece_parts"]) for k in range(parts)]


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


@pytest.fixture(scope="module")
def cars(env):
    ghf, ctx, torch = env
    bidx = ctx.batch_index_alloc(CARS, MAX_SYMBOLS)
    yield bidx
    ctx.batch_index_free(bidx)


@pytest.fixture(scope="module", autouse=True)
def sweep():
    """the pool and its items, made once before the first id runs"""
    pool = zs.pool()
    assert zs.groups() == GROUPS
    for t in pool:
        assert len(zs.items(t)) <= CARS
    return pool


@pytest.fixture(scope="module", autouse=True)
def warm(env, cars, sweep):
    """the first launch of a kernel loads its code object: one shallow and one deep tree run here, so that no id's time
    depends on the order in which the ids run"""
    for depth in (9, 33):
        t = zs.trees_of(depth)[0]
        pack_and_decode(env, cars, t, zs.items(t)[:2])
        pieces(env, t, zs.items(t)[:1])


@pytest.fixture(autouse=True)
def clean_status(env):
    """a failed id leaves no latched status behind for the next one"""
    yield
    ghf, ctx, torch = env
    torch.cuda.synchronize()
    ctx.L.ghf_clear_status(ctx.h)


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def sync_status(ghf, ctx):
    """the status the queued work latched (0: none); the context is usable again afterwards"""
    try:
        ctx.sync()
    except ghf.GhfError as e:
        return e.status
    return 0


def call_status(ghf, ctx, f):
    """the status a call returns or latches; cleared afterwards"""
    try:
        f()
    except ghf.GhfError as e:
        ctx.L.ghf_clear_status(ctx.h)
        return e.status
    return sync_status(ghf, ctx)


def model_code(ghf, t):
    """the ghf_code of the tree's codes as ghf_crs_build_code documents it: codeword[] = bits 0..31, symbol[] = bits 32..63
    only when the tree is deeper than 32, otherwise 0xFFFFFFFF"""
    code = ghf.Code()
    deep = t.max_len > 32
    for s in range(ghf.NSYM):
        code.length[s], code.codeword[s], code.symbol[s] = 0, 0, 0 if deep else 0xFFFFFFFF
    for k in t.live.tolist():
        v = t.value[k]
        code.length[k], code.codeword[k] = int(t.length[k]), v & 0xFFFFFFFF
        if deep:
            code.symbol[k] = v >> 32
    code.min_len, code.max_len = t.min_len, t.max_len
    return code


def parsed_tree(ghf, t):
    """the host parser's tree of the model's header, every field held to the model"""
    tree, tb = ghf.crs_parse_header(t.header)
    n_par = t.n_leaves - 1
    assert (tb, tree.tree_bytes, tree.max_len, tree.n_leaves, tree.root) == (t.tree_bytes, t.tree_bytes, t.max_len, t.n_leaves, t.root), t
    assert list(tree.left[:n_par]) == t.left[:n_par] and list(tree.right[:n_par]) == t.right[:n_par], t
    assert not any(tree.left[n_par:]) and not any(tree.right[n_par:]), t
    assert bytes(tree.header[:tb]) == t.header.tobytes() and not any(tree.header[tb:]), t
    # a header with bytes behind it (the file) parses to the same tree
    tree2, tb2 = ghf.crs_parse_header(np.concatenate((t.header, np.array([3, 0x80, 0xFF], dtype=np.uint8))))
    assert tb2 == tb and bytes(tree2) == bytes(tree), t
    return tree


def emit_cap(end_bit):
    """the smallest capacity ghf_encode_emit takes: through the 16-byte unit that holds the end bit (which is in no unit when
    the stream ends on one's edge)"""
    return end_bit >> 3 if end_bit % 128 == 0 else ((end_bit >> 7) + 1) << 4


class Streams:
    """the decoders' inputs of a case in one device buffer: every stream 16-byte aligned, GUARD bytes behind it (the library
    reads no bit behind stream_bytes: whatever stands there must not matter)"""

    def __init__(self, torch, arrays):
        self.offs, at = [], 0
        for a in arrays:
            self.offs.append(at)
            at += (a.size + 15 & ~15) + 32
        h = np.full(max(at, 16), GUARD, dtype=np.uint8)
        for o, a in zip(self.offs, arrays):
            h[o : o + a.size] = a
        self.sizes = [int(a.size) for a in arrays]
        self.d = torch.from_numpy(h).cuda()
        assert self.d.data_ptr() % 16 == 0

    def view(self, k):
        return self.d[self.offs[k] : self.offs[k] + (self.sizes[k] + 15 & ~15) + 32]


# ------------------------------------------------------------------------------ pack, decode with the side-car, K6 + decode
def pack_and_decode(env, cars, t, its):
    ghf, ctx, torch = env
    tree = parsed_tree(ghf, t)
    d_tree = ctx.tree_to_device(tree)
    d_code = ctx.code_to_device(model_code(ghf, t))
    head = t.tree_bytes + 2
    start = torch.tensor([8 * head], dtype=torch.int64, device="cuda")
    inputs = Streams(torch, [it.data for it in its])        # (the packer's inputs: same packing)
    files = Streams(torch, [it.decoder_input for it in its])
    a, plan = Arena(), []
    for it in its:
        r = {"cap": emit_cap(8 * head + it.total_bits)}
        r["stream"] = a.add(r["cap"])
        r["car"], r["cold"], r["k6"] = a.add(it.n), a.add(it.n, skew=1), a.add(it.n, skew=7)
        plan.append(r)
    a.alloc(torch)
    meta = torch.full((len(its), 8), -1, dtype=torch.int64, device="cuda")
    sizes = []
    for i, (it, r) in enumerate(zip(its, plan)):
        d_in = inputs.view(i)[: it.n]
        ix = ghf.batch_index_item(cars, i, it.n)
        d_stream = a.view(r["stream"])
        sbytes = head + int(it.body.size)
        d_stream[:head] = files.view(i)[:head]  # tree and prefix bytes: the packer leaves what stands in front of its start bit
        ctx.encode_plan(d_in, d_code, total=meta[i, 0:1])
        ctx.encode_emit(d_in, d_code, d_stream, start_bit=start, flags=ghf.EMIT_LONG_CODES, index=ix, end=meta[i, 1:3])
        # K7 with the packer's side-car: 16-byte stores, and one byte off alignment (one symbol at a time, at every depth)
        ctx.crs_decode(d_stream, sbytes, it.left_bits, d_tree, ix, d_out=a.view(r["car"]), nbytes=meta[i, 3:4])
        ctx.crs_decode(d_stream, sbytes, it.left_bits, d_tree, ix, d_out=a.view(r["cold"]), nbytes=meta[i, 4:5])
        # from the model's file alone: K6 rebuilds the side-car (synchronises), no symbol may come out of the padding
        d_file = files.view(i)
        assert files.sizes[i] == sbytes
        try:
            sizes.append(ctx.crs_decoded_size(d_file, sbytes, it.left_bits, d_tree))
            ctx.crs_decode(d_file, sbytes, it.left_bits, d_tree, None, d_out=a.view(r["k6"]), nbytes=meta[i, 5:6])
        except ghf.GhfError as e:  # (K6 reports to the host at once)
            raise AssertionError((it, "K6 on the file", str(e)))
    status = sync_status(ghf, ctx)  # (held at the end: the comparisons below name the item)
    clean = a.fetch()
    chunk = np.zeros((CARS, cars.blocks_per_item), dtype=np.uint64)
    seg = np.zeros((CARS, cars.segs_per_item), dtype=np.uint32)
    assert ctx.L.ghf_copy_d2h(ctx.h, chunk.ctypes.data, cars.d_chunk_bit, chunk.nbytes) == 0
    assert ctx.L.ghf_copy_d2h(ctx.h, seg.ctypes.data, cars.d_seg_bit, seg.nbytes) == 0
    assert sync_status(ghf, ctx) == 0
    h_meta = meta.cpu().tolist()
    for i, (it, r) in enumerate(zip(its, plan)):
        m, sbytes = h_meta[i], head + int(it.body.size)
        end_bit = 8 * head + it.total_bits
        assert m[0] == it.total_bits and m[1:3] == [end_bit, (end_bit + 7) // 8], (it, "encode_plan / encode_emit", m)
        got, want = a.got(r["stream"]), it.decoder_input  # = tree || prefix || the body with its zero-filled last byte
        assert np.array_equal(got[:sbytes], want), (it, "encode_emit", first_diff(got[:sbytes], want))
        assert not got[sbytes:].any(), (it, "encode_emit: the rest of the last unit is zero")
        want_chunk, want_seg = it.index()
        assert np.array_equal(chunk[i, : want_chunk.size], want_chunk) and np.array_equal(seg[i, : want_seg.size], want_seg), (it, "side-car")
        assert m[3:6] == [it.n] * 3 and sizes[i] == it.n, (it, "decoded sizes", m, sizes[i])
        for what, k in (("decode with the side-car", "car"), ("decode into an unaligned output", "cold"), ("K6 + decode from the file", "k6")):
            assert np.array_equal(a.got(r[k]), it.data), (it, what, first_diff(a.got(r[k]), it.data))
    assert clean, (t.label, "guard bytes")
    assert status == 0, (t.label, "latched status", status)


@pytest.mark.parametrize("depth", GROUPS, ids=lambda d: "len%d-pack" % d)
def test_pack_and_decode(env, cars, depth):
    for t in zs.trees_of(depth):
        pack_and_decode(env, cars, t, zs.items(t))


# ------------------------------------------------------------------------------ a body in pieces
def pieces(env, t, its):
    """ghf_crs_sync_piece + ghf_crs_decode(index = NULL) piece by piece, as tests/test_gpu_crs.py::test_crs_body_in_pieces: own
    bytes + 16 bytes of look-ahead (the stored last byte, then zeros, behind the last piece), every (landing, n_symbols) the
    model's, the outputs back to back in one guarded region"""
    ghf, ctx, torch = env
    d_tree = ctx.tree_to_device(parsed_tree(ghf, t))
    a, plan = Arena(), []
    for it in its:
        plan.append([(own, it.pieces(own), a.add(it.n, skew=(own + it.n) % 16)) for own in it.cuts()])
    a.alloc(torch)
    for it, cuts in zip(its, plan):
        if not cuts:
            continue
        d_body = to_dev(torch, np.concatenate((it.body, np.zeros(4096 + 64, dtype=np.uint8))))
        for own, want, region in cuts:
            d_out, at = a.view(region), 0
            psize = (own + 16 + 15 & ~15) + 16
            nbs = torch.full((len(want),), -1, dtype=torch.int64, device="cuda")
            for k, (lo, hi, first, end_bit, landing, nsym) in enumerate(want):
                d_piece = torch.zeros(psize, dtype=torch.uint8, device="cuda")
                d_piece[: hi - lo + 16] = d_body[lo : hi + 16]
                try:
                    got = ctx.crs_sync_piece(d_piece, psize, first, end_bit, d_tree)
                except ghf.GhfError as e:
                    raise AssertionError((it, "piece of %d at byte %d" % (own, lo), str(e)))
                assert got == (landing, nsym), (it, "piece of %d at byte %d" % (own, lo), got, (landing, nsym))
                if nsym:
                    ctx.crs_decode(d_piece, psize, 0, d_tree, None, d_out=d_out[at : at + nsym], nbytes=nbs[k : k + 1])
                    at += nsym
            assert at == it.n, (it, own)
            status = sync_status(ghf, ctx)
            assert status == 0, (it, "pieces of %d" % own, "latched status", status)
            assert nbs.cpu().tolist() == [p[5] if p[5] else -1 for p in want], (it, own)
    clean = a.fetch()
    for it, cuts in zip(its, plan):
        for own, want, region in cuts:
            assert np.array_equal(a.got(region), it.data), (it, "pieces of %d" % own, first_diff(a.got(region), it.data))
    assert clean, (t.label, "guard bytes")


@pytest.mark.parametrize("depth,part", PIECE_IDS, ids=["len%d-pieces%s" % (d, "-" + "abcd"[k] if (d, 1) in PIECE_IDS else "") for d, k in PIECE_IDS])
def test_pieces(env, depth, part):
    assert zs.piece_parts(depth) == sum(1 for d, _ in PIECE_IDS if d == depth)
    for t, its in zs.piece_part(depth, part):
        pieces(env, t, its)


# ------------------------------------------------------------------------------ the whole ghf_crs_compress
@pytest.mark.parametrize("part", range(3))
def test_crs_compress_of_the_materialised_histograms(env, part):
    """the family entries that exist as bytes, in thirds: the file equals orc.crs_compress(data), both decodes give it back"""
    ghf, ctx, torch = env
    mine = [(i, label, h) for i, label, h in hf.pinned() if hf.n_live(h) >= 2][part::3]
    assert len(mine) >= 100
    for i, label, h in mine:
        data = hf.materialise(i, h)
        ref = orc.crs_compress(data)
        d_in = to_dev(torch, data)
        idx = ctx.index_alloc(data.size)
        a = Arena()
        cap = int(ctx.L.ghf_crs_compress_bound(data.size))
        r_out, r_car, r_k6 = a.add(cap), a.add(data.size), a.add(data.size, skew=5)
        a.alloc(torch)
        d_out, nbytes, d_tree = ctx.crs_compress(d_in, d_out=a.view(r_out), index=idx)
        tb = 2 * (2 * hf.n_live(h) - 1)
        left = int(ref[tb])
        n1 = ctx.crs_decode(d_out, ref.size + (1 if left else 0), left, d_tree, idx, d_out=a.view(r_car))[1]
        files = Streams(torch, [np.concatenate((ref, ref[tb + 1 : tb + 2])) if left else ref])
        n2 = ctx.crs_decode(files.view(0), files.sizes[0], left, d_tree, None, d_out=a.view(r_k6))[1]
        ctx.sync()
        ctx.index_free(idx)
        assert a.fetch(), (label, "guard bytes")
        assert int(nbytes.item()) == ref.size and np.array_equal(a.got(r_out, ref.size), ref), (label, first_diff(a.got(r_out, ref.size), ref))
        assert int(n1.item()) == int(n2.item()) == data.size, label
        assert np.array_equal(a.got(r_car), data) and np.array_equal(a.got(r_k6), data), label


# ------------------------------------------------------------------------------ refusals
def one_item(depth_lo, depth_hi, mode="flat", min_n=200):
    """the first item of that mode and size among the trees of these depths"""
    for t in zs.pool():
        if depth_lo <= t.max_len <= depth_hi:
            for it in zs.items(t):
                if it.mode == mode and it.n >= min_n:
                    return it
    raise AssertionError((depth_lo, depth_hi, mode))


class Packed:
    """an item packed on the GPU with a live side-car, and a good decode of it to show that the context still works"""

    def __init__(self, env, it):
        ghf, ctx, torch = env
        self.env, self.it, t = env, it, it.tree
        self.tree = parsed_tree(ghf, t)
        self.d_tree = ctx.tree_to_device(self.tree)
        self.code = model_code(ghf, t)
        self.d_code = ctx.code_to_device(self.code)
        self.head = t.tree_bytes + 2
        self.start = torch.tensor([8 * self.head], dtype=torch.int64, device="cuda")
        self.d_in = to_dev(torch, it.data)
        self.cap = emit_cap(8 * self.head + it.total_bits)
        self.sbytes = self.head + int(it.body.size)
        self.idx = ctx.index_alloc(it.n)
        self.d_stream = torch.zeros(self.cap, dtype=torch.uint8, device="cuda")
        ctx.encode_plan(self.d_in, self.d_code)
        ctx.encode_emit(self.d_in, self.d_code, self.d_stream, start_bit=self.start, flags=ghf.EMIT_LONG_CODES, index=self.idx)
        ctx.sync()
        self.still_works()

    def still_works(self):
        ghf, ctx, torch = self.env
        out, nb = ctx.crs_decode(self.d_stream, self.sbytes, self.it.left_bits, self.d_tree, self.idx)
        ctx.sync()
        assert int(nb.item()) == self.it.n and np.array_equal(out[: self.it.n].cpu().numpy(), self.it.data), self.it

    def refused(self, what, status, queue, room=0, may_write=0):
        """queue(d_out) must end in `status` and leave the guarded output as it was (but for its first `may_write` bytes)"""
        ghf, ctx, torch = self.env
        a = Arena()
        r = a.add(room or self.it.n + 16)
        a.alloc(torch)
        got = call_status(ghf, ctx, lambda: queue(a.view(r)))
        assert got == status, (self.it, what, got)
        assert a.fetch() and (a.got(r)[may_write:] == GUARD).all(), (self.it, what, "the output was written")
        self.still_works()

    def close(self):
        self.env[1].index_free(self.idx)


@pytest.mark.parametrize("depths", [(2, 12), (13, 32), (33, 64)], ids=lambda d: "len%d..%d" % d)
def test_a_malformed_device_tree_is_refused(env, depths):
    ghf, ctx, torch = env
    p = Packed(env, one_item(*depths))
    nl = p.tree.n_leaves
    for field, value in (("max_len", 0), ("max_len", 65), ("n_leaves", 1), ("n_leaves", 257), ("root", 255), ("root", 256 + nl - 1)):
        bad = ghf.Tree.from_buffer_copy(bytes(p.tree))
        setattr(bad, field, value)
        d_bad = ctx.tree_to_device(bad)
        p.refused("%s = %d" % (field, value), E_FORMAT,
                  lambda d_out: ctx.crs_decode(p.d_stream, p.sbytes, p.it.left_bits, d_bad, p.idx, d_out=d_out[: p.it.n]))
    p.close()


@pytest.mark.parametrize("depths", [(2, 12), (13, 32), (33, 64)], ids=lambda d: "len%d..%d" % d)
def test_a_code_the_packer_cannot_pack_is_refused(env, depths):
    ghf, ctx, torch = env
    p = Packed(env, one_item(*depths))
    it = p.it

    room = (p.cap + it.n + 64 + 15) & ~15  # (a length[] one too long asks for up to a bit per symbol more)

    def emit(d_code, flags):
        def queue(d_out):
            ctx.encode_plan(p.d_in, d_code)
            ctx.encode_emit(p.d_in, d_code, d_out, start_bit=p.start, flags=flags)
        return queue

    too_long = ghf.Code.from_buffer_copy(bytes(p.code))
    too_long.length[int(it.tree.live[0])] = it.tree.max_len + 1
    p.refused("a length[] above max_len", E_FORMAT, emit(ctx.code_to_device(too_long), ghf.EMIT_LONG_CODES), room)
    if it.tree.max_len > 32:
        p.refused("deeper than 32 without GHF_EMIT_LONG_CODES", E_FORMAT, emit(p.d_code, 0), room)
        p.refused("deeper than 32 with GHF_EMIT_LAST", E_FORMAT, emit(p.d_code, ghf.EMIT_LONG_CODES | ghf.EMIT_LAST), room)
    p.close()


@pytest.mark.parametrize("depths", [(2, 12), (13, 32), (33, 64)], ids=lambda d: "len%d..%d" % d)
def test_a_flipped_body_bit_is_caught_by_the_side_car(env, depths):
    """the bit is chosen with the model's decoder: the 64 codes of segment 0 then end elsewhere than the side-car says.  K7
    decodes its segments side by side and checks each end behind the segment's stores, so GHF_E_CORRUPT -- unlike every
    GHF_E_FORMAT above -- comes with decoded bytes in the output (include/ghf.h at ghf_decode promises "nothing is written" for
    GHF_E_FORMAT only): what is held is that nothing lands behind the n bytes the side-car speaks of"""
    ghf, ctx, torch = env
    p = Packed(env, one_item(*depths))
    at = zs.flipped_bit(p.it, 0xF11B + depths[0])
    bad = p.d_stream.clone()
    bad[p.head + at // 8] ^= 0x80 >> (at % 8)
    p.refused("body bit %d flipped" % at, E_CORRUPT,
              lambda d_out: ctx.crs_decode(bad, p.sbytes, p.it.left_bits, p.d_tree, p.idx, d_out=d_out[: p.it.n]), may_write=p.it.n)
    p.close()


@pytest.mark.parametrize("depths", [(2, 12), (13, 32), (33, 64)], ids=lambda d: "len%d..%d" % d)
def test_left_bits_off_by_one_is_caught_by_k6(env, depths):
    """chosen with the model's decoder: under the wrong left_bits the last code provably does not end where the stream does"""
    ghf, ctx, torch = env
    it = next(it for t in zs.pool() if depths[0] <= t.max_len <= depths[1] and t.length[t.leftmost] >= 2
              for it in zs.items(t) if it.mode == "ends" and len(zs.wrong_left_bits(it)) == 2)
    p = Packed(env, it)
    files = Streams(torch, [it.decoder_input])
    for left in zs.wrong_left_bits(it):
        sbytes = p.head + (it.total_bits + it.left_bits - left + 7) // 8  # (one less than 0 would need another byte: not reached)
        assert sbytes == p.sbytes
        p.refused("left_bits %d for %d, decoded size" % (left, it.left_bits), E_CORRUPT,
                  lambda d_out: ctx.crs_decoded_size(files.view(0), sbytes, left, p.d_tree))
        p.refused("left_bits %d for %d, decode" % (left, it.left_bits), E_CORRUPT,
                  lambda d_out: ctx.crs_decode(files.view(0), sbytes, left, p.d_tree, None, d_out=d_out[: it.n + 8]))
    p.close()
