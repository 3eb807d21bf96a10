"""GPU (-m gpu): the one-workgroup-per-item kernels across their round seams, against the exact model of
tests/batch_seams.py -- every packer at every carry and at every size of the body's last unit (tier P), the side-car
decoders at their round of 16 384 symbols and at every output offset (tier S), the decoders that find the boundaries
themselves with a code, or the end mark, at every position of the edge at 131 072 bits (tier R), and the run-record decoders
at their round of 32 768 symbols (tier U).  Nothing expected comes from the library: bodies are orc_encode_body's, images
orc.compress's or header || body, side-cars and run records are summed from the oracle's code lengths.  Every output sits
between 0xA5 guard bytes that are compared with it; a whole tier of a code is one launch per call.  A mismatch names the
call, the code with its shape, the item (fill, carry or over, size), the round the first wrong byte lies in and the byte."""
import ctypes as C

import numpy as np
import pytest

import batch_seams as bs
import pkgload
from guarded import GUARD, Arena, first_diff

pytestmark = pytest.mark.gpu

OK, E_CAP, E_CORRUPT = bs.OK, bs.E_CAP, bs.E_CORRUPT
FILL = 0xCD  # what the side-car arrays hold before a compress call
CODES = list(range(len(bs.codes())))
ids_of = lambda k: "%d_%d-%s" % (bs.codes()[k].shape + (bs.codes()[k].label.replace("/", "."),))  # noqa: E731


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def i64(torch, values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64).cuda()


def codes_to_device(torch, codes):
    """ctypes code structs (orc.OrcCode: ghf_code's layout) -> a CUDA uint8 tensor [len(codes), sizeof(ghf_code)]"""
    t = torch.from_numpy(np.stack([np.frombuffer(bytes(c), dtype=np.uint8) for c in codes]).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


class Inputs:
    """host arrays in one device buffer: at odd addresses with three filler bytes between them (aligned=False), or each at
    a 16-byte boundary with 64 guard bytes behind it; a None entry is a null pointer of 0 bytes; sizes overrides what is passed"""

    def __init__(self, torch, arrays, aligned=False, sizes=None):
        self.count, offs, at = len(arrays), [], 0
        for a in arrays:
            at = at + 15 & ~15 if aligned else at | 1
            offs.append(at)
            at += (0 if a is None else a.size) + (64 if aligned else 3)
        packed = np.full(at + 64, GUARD if aligned else 0x5A, dtype=np.uint8)
        for o, a in zip(offs, arrays):
            if a is not None:
                packed[o : o + a.size] = a
        self.d = torch.from_numpy(packed).cuda()
        assert self.d.data_ptr() % 16 == 0
        self.sizes = [(0 if a is None else int(a.size)) if sizes is None or sizes[k] is None else int(sizes[k]) for k, a in enumerate(arrays)]
        self.ptrs = i64(torch, [0 if a is None else self.d.data_ptr() + o for o, a in zip(offs, arrays)])
        self.bytes = i64(torch, self.sizes)


class Packed:
    """one compress launch -- `call`: "shared", "planes", "forms" or "own" -- into slots of cap = the call's bound with 64
    guard bytes behind each, the side-car arrays filled with FILL before it"""

    def __init__(self, env, call, datas, d_codes, max_item, e=1, raw=0, fetch=True):
        ghf, ctx, torch = env
        L = ghf.lib()
        self.env, self.e, self.max_item = env, e, max_item
        self.inp = Inputs(torch, datas)
        self.count, self.slots = len(datas), len(datas) * e
        self.cap = {"shared": ghf.compress_batch_shared_bound, "own": ghf.compress_batch_bound}[call](max_item) if e == 1 else \
            ghf.compress_batch_planes_shared_bound(max_item, e)
        self.stride = (self.cap + 15 & ~15) + 64
        self.d_out = torch.full((self.slots * self.stride + 16,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.d_out.data_ptr() % 16 == 0
        self.out_ptrs = i64(torch, [self.d_out.data_ptr() + j * self.stride for j in range(self.slots)])
        self.out_caps = i64(torch, [self.cap] * self.slots)
        self.out_bytes = torch.full((self.slots,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((self.slots,), -1, dtype=torch.int32, device="cuda")
        self.bidx = ctx.batch_index_alloc(self.slots, max_item // e)
        chunk_bytes, seg_bytes = 8 * self.slots * self.bidx.blocks_per_item, 4 * self.slots * self.bidx.segs_per_item
        assert L.ghf_memset_d(ctx.h, self.bidx.d_chunk_bit, FILL, chunk_bytes) == 0
        assert L.ghf_memset_d(ctx.h, self.bidx.d_seg_bit, FILL, seg_bytes) == 0
        head = (ctx.h, self.inp.ptrs.data_ptr(), self.inp.bytes.data_ptr(), max_item, self.count)
        outs = (self.out_ptrs.data_ptr(), self.out_caps.data_ptr(), self.out_bytes.data_ptr())
        tail = (C.byref(self.bidx), self.status.data_ptr())
        if call == "shared":
            rc = L.ghf_compress_batch_shared(*head, d_codes.data_ptr(), *outs, *tail)
        elif call == "own":
            self.d_codes = torch.zeros((self.count, C.sizeof(ghf.Code)), dtype=torch.uint8, device="cuda")
            rc = L.ghf_compress_batch(*head, *outs, self.d_codes.data_ptr(), *tail)
        elif call == "planes":
            rc = L.ghf_compress_batch_planes_shared(*head, e, d_codes.data_ptr(), *outs, *tail)
        else:
            rc = L.ghf_compress_batch_planes_forms(*head, e, d_codes.data_ptr(), raw, *outs, *tail)
        assert rc == 0, (call, rc)
        ctx.sync()  # raises if the context's status word was latched
        self.h_bytes, self.h_status = self.out_bytes.cpu().numpy(), self.status.cpu().numpy()
        if fetch:
            self.h_out = self.d_out.cpu().numpy()
            chunk, seg = np.zeros(chunk_bytes // 8, dtype=np.uint64), np.zeros(seg_bytes // 4, dtype=np.uint32)
            assert L.ghf_copy_d2h(ctx.h, chunk.ctypes.data, self.bidx.d_chunk_bit, chunk.nbytes) == 0
            assert L.ghf_copy_d2h(ctx.h, seg.ctypes.data, self.bidx.d_seg_bit, seg.nbytes) == 0
            ctx.sync()
            self.h_chunk, self.h_seg = chunk.reshape(self.slots, -1), seg.reshape(self.slots, -1)

    def free(self):
        self.env[1].batch_index_free(self.bidx)


def blame(length, data, lead, at):
    """where byte `at` of a packed slot lies: the round, and the carries at the seams"""
    rb = np.add.reduceat(np.asarray(length)[data], range(0, data.size, bs.ROUND))
    ends = lead + np.cumsum(rb)
    r = int(np.searchsorted(ends, 8 * at, side="right"))
    return "round %d of %d (carry at the seams: %s)" % (min(r, rb.size - 1), rb.size, [int(x) % 128 for x in ends[:-1]])


def check_packed(b, call, wants):
    """wants[j] = (name, expected slot bytes, (chunk_bit, seg_bit) or None, blame arguments or None) by slot: every byte of
    every slot and its guard, d_out_bytes, d_item_status, the side-car slices (None: the slice stays as it was)"""
    want = np.full(b.h_out.size, GUARD, dtype=np.uint8)
    for j, (name, body, index, who) in enumerate(wants):
        assert (int(b.h_status[j]), int(b.h_bytes[j])) == (OK, body.size), (call, name, "status, bytes", int(b.h_status[j]), int(b.h_bytes[j]), body.size)
        want[j * b.stride : j * b.stride + body.size] = body
    if not np.array_equal(b.h_out, want):
        at = int(np.flatnonzero(b.h_out != want)[0])
        j, off = divmod(at, b.stride)
        name, body, index, who = wants[j]
        where = "the guard behind the body" if off >= body.size else blame(*who, off) if who else "a raw plane"
        raise AssertionError((call, name, "first wrong byte %d of %d (cap %d): %s" % (off, body.size, b.cap, where)))
    for j, (name, body, index, who) in enumerate(wants):
        if index is None:
            assert np.all(b.h_chunk[j].view(np.uint8) == FILL) and np.all(b.h_seg[j].view(np.uint8) == FILL), (call, name, "side-car of a raw slot")
        else:
            chunk, seg = index
            assert np.array_equal(b.h_chunk[j, : chunk.size], chunk) and np.array_equal(b.h_seg[j, : seg.size], seg), (call, name, "side-car")
            assert np.all(b.h_chunk[j, chunk.size :].view(np.uint8) == FILL) and np.all(b.h_seg[j, seg.size :].view(np.uint8) == FILL), (call, name, "behind the side-car")


def check_records(env, b, call, records):
    """ghf_batch_seek_pack on the side-cars of `b`: records[j] = (name, expected record) or None (a raw slot: unspecified)"""
    ghf, ctx, torch = env
    stride = ghf.batch_seek_bound(int(b.bidx.max_item_bytes)) + 32
    d_rec = torch.full((b.slots * stride + 64,), GUARD, dtype=torch.uint8, device="cuda")
    ptrs = i64(torch, [d_rec.data_ptr() + j * stride for j in range(b.slots)])
    caps = i64(torch, [stride - 32] * b.slots)
    rec_bytes = torch.full((b.slots,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((b.slots,), -1, dtype=torch.int32, device="cuda")
    rc = ghf.lib().ghf_batch_seek_pack(ctx.h, C.byref(b.bidx), b.inp.bytes.data_ptr(), b.count, b.e, ptrs.data_ptr(), caps.data_ptr(),
                                       rec_bytes.data_ptr(), status.data_ptr())
    assert rc == 0, rc
    ctx.sync()
    h, st, nb = d_rec.cpu().numpy(), status.cpu().numpy(), rec_bytes.cpu().numpy()
    for j, r in enumerate(records):
        if r is not None:
            name, rec = r
            got = h[j * stride : (j + 1) * stride]
            assert (int(st[j]), int(nb[j])) == (OK, rec.size), (call, name, "ghf_batch_seek_pack", int(st[j]), int(nb[j]))
            assert np.array_equal(got[: rec.size], rec), (call, name, "ghf_batch_seek_pack", first_diff(got[: rec.size], rec))
            assert np.all(got[rec.size :] == GUARD), (call, name, "ghf_batch_seek_pack wrote behind its record")


# ==================================================================================================== P. every packer, every carry
def flat_wants(items):
    return [(repr(it), it.body, it.index, (it.code.length, it.data, 0)) for it in items]


@pytest.mark.parametrize("k", CODES, ids=ids_of)
def test_shared_packer_at_every_carry_and_every_last_unit(env, k):
    """ghf_compress_batch_shared: 4 fills x 128 carries at seam 1 (127 - c at seam 2) and the 16 last-unit items, one launch"""
    ghf, ctx, torch = env
    code = bs.codes()[k]
    items = bs.p_items(code) + list(bs.tails(code))
    assert len(items) == (4 * 128 if bs.steer_pair(code) else 4) + 16
    b = Packed(env, "shared", [it.data for it in items], codes_to_device(torch, [code.code]), max(it.n for it in items))
    try:
        check_packed(b, "ghf_compress_batch_shared", flat_wants(items))
        check_records(env, b, "ghf_compress_batch_shared", [(repr(it), it.record) for it in items])
    finally:
        b.free()


def plane_wants(tensors, raw):
    wants, records = [], []
    for t in tensors:
        for p, pl in enumerate(t.planes):
            name = "%s, plane %d: %r" % (t.name, p, pl)
            if raw >> p & 1:
                wants.append((name, pl.data, None, None))
                records.append(None)
            else:
                wants.append((name, pl.body, pl.index, (pl.code.length, pl.data, 0)))
                records.append((name, pl.record))
    return wants, records


@pytest.mark.parametrize("e", bs.WIDTHS)
@pytest.mark.parametrize("k", CODES, ids=ids_of)
def test_plane_packers_at_every_carry_and_every_last_unit(env, k, e):
    """ghf_compress_batch_planes_shared, then ghf_compress_batch_planes_forms with one plane raw, on the same tensors: plane
    p under code (k + p) % 10, every plane of a tensor at a carry of its own"""
    ghf, ctx, torch = env
    tensors = bs.p_planes(k, e)
    d_codes = codes_to_device(torch, [pl.code.code for pl in tensors[0].planes])
    datas = [t.data for t in tensors]
    max_item = max(d.size for d in datas)
    for call, raw in (("planes", 0), ("forms", bs.raw_of(k, e))):
        b = Packed(env, call, datas, d_codes, max_item, e=e, raw=raw)
        try:
            wants, records = plane_wants(tensors, raw)
            name = "ghf_compress_batch_planes_" + ("shared" if call == "planes" else "forms(raw_planes=%#x)" % raw)
            check_packed(b, name, wants)
            check_records(env, b, name, records)
        finally:
            b.free()
        del b


@pytest.mark.parametrize("k", CODES, ids=ids_of)
def test_the_packer_with_the_items_own_code_behind_its_header(env, k):
    """ghf_compress_batch: the image is orc.compress(item), the first carry the header's (0 or 64 by the parity of max_len)"""
    ghf, ctx, torch = env
    code = bs.codes()[k]
    items = [it for it in bs.own_items() if it.base is code]
    assert len(items) in (4 * 128, 4)
    b = Packed(env, "own", [it.data for it in items], None, bs.N_P)
    try:
        check_packed(b, "ghf_compress_batch", [(repr(it), it.image, it.index, (it.length, it.data, it.lead)) for it in items])
        got = b.d_codes.cpu().numpy()
        for i, it in list(enumerate(items))[::64]:
            assert ghf.Code.from_buffer_copy(got[i].tobytes()).as_dict() == it.code.as_dict(), ("ghf_compress_batch", it, "d_codes")
    finally:
        b.free()


# =========================================================================================== the decoders' outputs, guarded
class Outputs:
    """one guarded output per item, `skews[i]` bytes behind a 16-byte boundary"""

    def __init__(self, torch, sizes, skews):
        self.a = Arena()
        self.regions = [self.a.add(n, skew=s) for n, s in zip(sizes, skews)]
        self.a.alloc(torch)
        self.ptrs = i64(torch, [self.a.view(r).data_ptr() for r in self.regions])
        for r, s in zip(self.regions, skews):
            assert self.a.view(r).data_ptr() % 16 == s % 16
        self.caps = i64(torch, sizes)
        self.out_bytes = torch.full((len(sizes),), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((len(sizes),), -1, dtype=torch.int32, device="cuda")

    @property
    def tail(self):
        return self.ptrs.data_ptr(), self.caps.data_ptr(), self.out_bytes.data_ptr(), self.status.data_ptr()

    def check(self, call, names, wants):
        """wants[i] = (status, d_out_bytes, the bytes of the whole region: data and what stays GUARD)"""
        clean = self.a.fetch()
        st, nb = self.status.cpu().numpy(), self.out_bytes.cpu().numpy()
        for i, (name, (status, nbytes, data)) in enumerate(zip(names, wants)):
            assert (int(st[i]), int(nb[i])) == (status, nbytes), (call, name, "status, bytes", int(st[i]), int(nb[i]), "want", status, nbytes)
            got = self.a.got(self.regions[i])
            if not np.array_equal(got, data):
                at = int(np.flatnonzero(got != data)[0])
                off = self.a.regions[self.regions[i]][0] % 16
                raise AssertionError((call, name, "output %d bytes behind a 16-byte boundary" % off,
                                      "first wrong byte %d of %d: round %d of the decoder's output" % (at, data.size, at // self.per)))
        assert clean, (call, "guard bytes between the outputs")


def sizes_only(torch, count):
    return torch.full((count,), -1, dtype=torch.int64, device="cuda"), torch.full((count,), -1, dtype=torch.int32, device="cuda")


# ======================================================================================= S. the side-car decoders at their round
@pytest.mark.parametrize("k", bs.S_CODES, ids=ids_of)
def test_side_car_decoders_at_their_round_and_every_output_offset(env, k):
    """ghf_decode_batch_shared on the bodies ghf_compress_batch_shared packs, and ghf_decode_batch on header || body with the
    oracle's tables and a side-car written from the oracle's lengths: sizes 16384 k + {0, 1, 63, 64, 65}, the `deep` and the
    `ones` fill, every output offset 0..15 (include/ghf.h asks no alignment of any decode output: there is no refusal case)"""
    ghf, ctx, torch = env
    L = ghf.lib()
    code = bs.codes()[k]
    items = [it for it in bs.s_items(code) for _ in range(16)]
    skews = [s for _ in bs.s_items(code) for s in range(16)]
    names = ["%r, offset %d" % (it, s) for it, s in zip(items, skews)]
    sizes = [it.n for it in items]
    wants = [(OK, it.n, it.data) for it in items]
    d_code = codes_to_device(torch, [code.code])
    b = Packed(env, "shared", [it.data for it in items], d_code, max(sizes), fetch=False)
    try:
        assert b.h_status.tolist() == [OK] * len(items) and b.h_bytes.tolist() == [it.body.size for it in items]
        o = Outputs(torch, sizes, skews)
        o.per = bs.SIDE_ROUND
        rc = L.ghf_decode_batch_shared(ctx.h, b.out_ptrs.data_ptr(), b.out_bytes.data_ptr(), d_code.data_ptr(), C.byref(b.bidx),
                                       i64(torch, sizes).data_ptr(), len(items), *o.tail)
        assert rc == 0, rc
        ctx.sync()
        o.check("ghf_decode_batch_shared", names, wants)
        # k_decode_batch: its own copy of the segment loop, per-item tables
        im = Inputs(torch, [it.image for it in items], aligned=True)
        chunk = np.zeros(len(items) * b.bidx.blocks_per_item, dtype=np.uint64)
        seg = np.zeros(len(items) * b.bidx.segs_per_item, dtype=np.uint32)
        for i, it in enumerate(items):
            c, s = it.index
            chunk[i * b.bidx.blocks_per_item :][: c.size] = c + np.uint64(8 * code.header.size)
            seg[i * b.bidx.segs_per_item :][: s.size] = s
        assert L.ghf_copy_h2d(ctx.h, b.bidx.d_chunk_bit, chunk.ctypes.data, chunk.nbytes) == 0
        assert L.ghf_copy_h2d(ctx.h, b.bidx.d_seg_bit, seg.ctypes.data, seg.nbytes) == 0
        ctx.sync()
        o = Outputs(torch, sizes, skews)
        o.per = bs.SIDE_ROUND
        d_codes = codes_to_device(torch, [code.code]).expand(len(items), -1).contiguous()
        rc = L.ghf_decode_batch(ctx.h, im.ptrs.data_ptr(), im.bytes.data_ptr(), d_codes.data_ptr(), C.byref(b.bidx),
                                i64(torch, sizes).data_ptr(), len(items), *o.tail)
        assert rc == 0, rc
        ctx.sync()
        o.check("ghf_decode_batch", names, wants)
    finally:
        b.free()


@pytest.mark.parametrize("e", bs.WIDTHS)
@pytest.mark.parametrize("k", (0, 1))
def test_plane_side_car_decoders_at_their_round_and_every_output_offset(env, k, e):
    """ghf_decode_batch_planes_shared and ghf_decode_batch_planes_forms (one plane raw) on what their packers pack: plane p
    under (1, 1) or (2, 32) in turn"""
    ghf, ctx, torch = env
    L = ghf.lib()
    base = bs.s_planes(k, e)
    tensors = [t for t in base for _ in range(16)]
    skews = [s for _ in base for s in range(16)]
    names = ["%r, offset %d" % (t, s) for t, s in zip(tensors, skews)]
    datas = [t.data for t in base for _ in range(16)]
    sizes = [d.size for d in datas]
    wants = [(OK, d.size, d) for d in datas]
    d_codes = codes_to_device(torch, [pl.code.code for pl in base[0].planes])
    n_elems = i64(torch, [t.n for t in tensors])
    for call, raw in (("planes", 0), ("forms", bs.raw_of(k, e))):
        b = Packed(env, call, datas, d_codes, max(sizes), e=e, raw=raw, fetch=False)
        try:
            assert b.h_status.tolist() == [OK] * b.slots
            assert b.h_bytes.tolist() == [pl.n if raw >> p & 1 else pl.body.size for t in tensors for p, pl in enumerate(t.planes)]
            o = Outputs(torch, sizes, skews)
            o.per = bs.SIDE_ROUND * e
            head = (ctx.h, b.out_ptrs.data_ptr(), b.out_bytes.data_ptr(), d_codes.data_ptr(), C.byref(b.bidx), n_elems.data_ptr(), len(tensors), e)
            if call == "planes":
                rc = L.ghf_decode_batch_planes_shared(*head, *o.tail)
            else:
                rc = L.ghf_decode_batch_planes_forms(*head, raw, *o.tail)
            assert rc == 0, rc
            ctx.sync()
            o.check("ghf_decode_batch_planes_" + ("shared" if call == "planes" else "forms(raw_planes=%#x)" % raw), names, wants)
        finally:
            b.free()
        del b, o


# ================================================================================ R. the decoders that find the boundaries
class Stats:
    """the two words of ghf_decode_images_batch_stats around one call"""

    def __init__(self, env):
        self.ctx, torch = env[1], env[2]
        self.words = torch.zeros(2, dtype=torch.int64, device="cuda")

    def __enter__(self):
        self.ctx.decode_images_batch_stats(self.words)
        return self

    def __exit__(self, *exc):
        self.ctx.decode_images_batch_stats(None)

    def check(self, call, want_rounds):
        rounds, passes = self.words.cpu().tolist()
        assert rounds == want_rounds and rounds <= passes <= 256 * rounds, (call, "rounds, passes", rounds, passes, "want rounds", want_rounds)


def r_wants(items):
    out = []
    for it in items:
        status, nbytes, stored, _ = it.verdict
        cap = it.n if it.cap is None else it.cap
        data = np.full(cap, GUARD, dtype=np.uint8)
        data[:stored] = it.data[:stored]
        out.append((status, nbytes, data))
    return out


@pytest.mark.parametrize("k", CODES, ids=ids_of)
def test_boundary_decoders_at_every_position_of_the_edge(env, k):
    """ghf_decode_bodies_batch_shared on orc_encode_body's bytes and ghf_decode_images_batch on header || body, sizes only and
    with outputs: a data code, then the end mark, at every position of the edge at bit 131 072 (of the body); bytes that
    stop inside the mark; a cap the first symbol of round 1 crosses; rounds of many slices at odd output phases"""
    ghf, ctx, torch = env
    L = ghf.lib()
    code = bs.codes()[k]
    items = list(bs.r_items(code)[0])
    names = [repr(it) for it in items]
    d_code = codes_to_device(torch, [code.code])
    hdr = int(code.header.size)
    caps = [it.n if it.cap is None else it.cap for it in items]
    skews = [1 + i % 15 for i in range(len(items))]
    bodies = Inputs(torch, [it.body for it in items], aligned=True, sizes=[it.stream_bytes for it in items])
    images = Inputs(torch, [it.image for it in items], aligned=True, sizes=[hdr + it.stream_bytes for it in items])
    for call, src in (("ghf_decode_bodies_batch_shared", bodies), ("ghf_decode_images_batch", images)):
        def launch(tail):
            if call == "ghf_decode_images_batch":
                return L.ghf_decode_images_batch(ctx.h, src.ptrs.data_ptr(), src.bytes.data_ptr(), len(items), tail[0], tail[1], tail[2], None, tail[3])
            return L.ghf_decode_bodies_batch_shared(ctx.h, src.ptrs.data_ptr(), src.bytes.data_ptr(), d_code.data_ptr(), len(items), *tail)

        out_bytes, status = sizes_only(torch, len(items))
        with Stats(env) as stats:
            assert launch((None, None, out_bytes.data_ptr(), status.data_ptr())) == 0
            ctx.sync()
        for i, it in enumerate(items):
            got = (int(status[i]), int(out_bytes[i]))
            assert got == it.sizes_verdict[:2], (call, "sizes only", names[i], got, "want", it.sizes_verdict[:2])
        stats.check(call + ", sizes only", sum(it.sizes_verdict[3] for it in items))
        o = Outputs(torch, caps, skews)
        o.per = 1 << 30
        with Stats(env) as stats:
            assert launch(o.tail) == 0
            ctx.sync()
        o.check(call, names, r_wants(items))
        stats.check(call, sum(it.verdict[3] for it in items))


@pytest.mark.parametrize("e", bs.WIDTHS)
@pytest.mark.parametrize("k", CODES, ids=ids_of)
def test_plane_boundary_decoders_at_every_position_of_the_edge(env, k, e):
    """ghf_decode_bodies_batch_planes_shared and .._planes_forms (one plane raw): plane 0 = the items of code k that decode
    whole, the planes beside it drawn under code (k + p) % 10; sizes only and with outputs"""
    ghf, ctx, torch = env
    L = ghf.lib()
    tensors = bs.r_planes(k, e)
    assert tensors
    names = [repr(t) for t in tensors]
    datas = [t.data for t in tensors]
    sizes = [d.size for d in datas]
    d_codes = codes_to_device(torch, [pl.code.code for pl in tensors[0].planes])
    skews = [1 + i % 15 for i in range(len(tensors))]
    for call, raw in (("ghf_decode_bodies_batch_planes_shared", 0), ("ghf_decode_bodies_batch_planes_forms", bs.raw_of(k, e))):
        src = Inputs(torch, [pl.data if raw >> p & 1 else pl.body for t in tensors for p, pl in enumerate(t.planes)], aligned=True)
        head = (ctx.h, src.ptrs.data_ptr(), src.bytes.data_ptr(), d_codes.data_ptr(), len(tensors), e) + ((raw,) if raw else ())
        fn = getattr(L, call)
        out_bytes, status = sizes_only(torch, len(tensors))
        with Stats(env) as stats:
            assert fn(*head, None, None, out_bytes.data_ptr(), status.data_ptr()) == 0
            ctx.sync()
        assert status.cpu().tolist() == [OK] * len(tensors) and out_bytes.cpu().tolist() == sizes, (call, "sizes only", tensors[0])
        want_rounds = sum(int(pl.cum[pl.n]) // bs.EDGE_BITS + 1 if hasattr(pl, "cum") else int(pl.code.length[pl.data].sum()) // bs.EDGE_BITS + 1
                          for t in tensors for p, pl in enumerate(t.planes) if not raw >> p & 1)
        stats.check(call + ", sizes only", want_rounds)
        o = Outputs(torch, sizes, skews)
        o.per = 1 << 30
        with Stats(env) as stats:
            assert fn(*head, *o.tail) == 0
            ctx.sync()
        o.check(call, names, [(OK, d.size, d) for d in datas])
        stats.check(call, want_rounds)


# ============================================================================================ U. the run-record decoders
def damaged_want(data, stored_bytes):
    want = np.full(data.size, GUARD, dtype=np.uint8)
    want[stored_bytes] = data[stored_bytes]
    return (E_CORRUPT, 0, want)


@pytest.mark.parametrize("k", bs.U_CODES, ids=ids_of)
def test_run_record_decoder_at_its_round(env, k):
    """ghf_decode_bodies_batch_shared_seek on the oracle's bodies and records: sizes 32768 k + {0, 1, 127, 128, 129}; under
    (2, 32) also 65 537 deepest symbols, every run 4096 bits; a record whose first run of round 1 is one bit long: CORRUPT
    with round 0 stored and nothing of round 1"""
    ghf, ctx, torch = env
    L = ghf.lib()
    code = bs.codes()[k]
    bad = bs.u_damaged(code)
    items = list(bs.u_items(code)) + [bad]
    names = [repr(it) for it in items]
    d_code = codes_to_device(torch, [code.code])
    bo = Inputs(torch, [it.body for it in items], aligned=True)
    ro = Inputs(torch, [it.record for it in items[:-1]] + [bs.damaged_record(bad)], aligned=True)
    head = (ctx.h, bo.ptrs.data_ptr(), bo.bytes.data_ptr(), ro.ptrs.data_ptr(), ro.bytes.data_ptr(), d_code.data_ptr(), len(items))
    out_bytes, status = sizes_only(torch, len(items))
    assert L.ghf_decode_bodies_batch_shared_seek(*head, None, None, out_bytes.data_ptr(), status.data_ptr()) == 0
    ctx.sync()
    assert status.cpu().tolist() == [OK] * len(items) and out_bytes.cpu().tolist() == [it.n for it in items]  # (sizes come from the records' headers)
    o = Outputs(torch, [it.n for it in items], [1 + i % 15 for i in range(len(items))])
    o.per = bs.RUN_ROUND
    assert L.ghf_decode_bodies_batch_shared_seek(*head, *o.tail) == 0
    ctx.sync()
    o.check("ghf_decode_bodies_batch_shared_seek", names, [(OK, it.n, it.data) for it in items[:-1]] + [damaged_want(bad.data, slice(0, bs.RUN_ROUND))])


@pytest.mark.parametrize("e", bs.WIDTHS)
@pytest.mark.parametrize("k", (0, 1))
def test_plane_run_record_decoders_at_their_round(env, k, e):
    """ghf_decode_bodies_batch_planes_shared_seek and .._planes_forms_seek (one plane raw, without a record).  The damaged
    record is plane 0's (the forms call's raw plane is never plane 0): round 0 of plane 0 is stored and nothing else"""
    ghf, ctx, torch = env
    L = ghf.lib()
    cc = bs.codes()
    tensors = bs.u_planes(k, e)
    bad = bs.Tensor("U%d/E%d/damaged" % (k, e), [bs.u_damaged(cc[bs.U_CODES[(k + p) % 2]]) for p in range(e)])
    tensors = tensors + [bad]
    names = [repr(t) for t in tensors]
    datas = [t.data for t in tensors]
    sizes = [d.size for d in datas]
    d_codes = codes_to_device(torch, [pl.code.code for pl in tensors[0].planes])
    stored = np.zeros(bad.n * e, dtype=bool)
    stored[: bs.RUN_ROUND * e : e] = True
    wants = [(OK, d.size, d) for d in datas[:-1]] + [damaged_want(datas[-1], stored)]
    for call, raw in (("ghf_decode_bodies_batch_planes_shared_seek", 0), ("ghf_decode_bodies_batch_planes_forms_seek", bs.raw_of(k, e))):
        assert not raw & 1
        bo = Inputs(torch, [pl.data if raw >> p & 1 else pl.body for t in tensors for p, pl in enumerate(t.planes)], aligned=True)
        recs = [None if raw >> p & 1 else pl.record for t in tensors for p, pl in enumerate(t.planes)]
        recs[-e] = bs.damaged_record(bad.planes[0])
        ro = Inputs(torch, recs, aligned=True)
        head = (ctx.h, bo.ptrs.data_ptr(), bo.bytes.data_ptr(), ro.ptrs.data_ptr(), ro.bytes.data_ptr(), d_codes.data_ptr(), len(tensors), e)
        head += (raw,) if raw else ()
        fn = getattr(L, call)
        out_bytes, status = sizes_only(torch, len(tensors))
        assert fn(*head, None, None, out_bytes.data_ptr(), status.data_ptr()) == 0
        ctx.sync()
        assert status.cpu().tolist() == [OK] * len(tensors) and out_bytes.cpu().tolist() == sizes, (call, "sizes only")
        o = Outputs(torch, sizes, [1 + i % 15 for i in range(len(tensors))])
        o.per = bs.RUN_ROUND * e
        assert fn(*head, *o.tail) == 0
        ctx.sync()
        o.check(call, names, wants)
