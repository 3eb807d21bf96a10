"""GPU: ghf_histogram_batch / ghf_compress_batch_shared / ghf_decode_batch_shared -- many small items under ONE code.

Expected values come from the CPU oracle through oracle.lib() (orc_histogram, orc_build_code, orc_encode_body,
orc_write_header, orc_decompress; pinned to the reference by tests/test_oracle_golden.py) and, where it has been built,
the compiled reference's own decoder.  The library's other paths (ghf_encode_emit, ghf_decode_images_batch) are
cross-checks only.  Inputs and decode outputs sit at odd addresses between guard bytes."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import pkgload
from cases import CASES
from header_cases import bad_codes, vet_branch_codes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT, E_NOCODE = 0, 1, 3, 5, 6, 7, 10
GUARD = 0xA5
MAX_ITEM = 1 << 20
COVER_ALL = 1
# the vector and segment edges; round edges and the carried unit
EDGE_SIZES = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8191, 8193]


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


def small_items(count, seed):
    """`count` seeded items of 1..8192 bytes, mixed kinds; every seventh folded to a few values (as tests/test_gpu_batch.py)"""
    out = []
    for i in range(count):
        n = int(dg.splitmix64(np.uint64(seed + i)) % np.uint64(8192)) + 1
        kind = ["uniform", "zipf", "sym16", "text"][i % 4]
        d = dg.make(kind, n, seed=seed + 7 * i)
        if i % 7 == 0:
            d = d % np.uint8(1 + i % 5)
        out.append(d)
    return out


# ---- the oracle's side ------------------------------------------------------------------------------------------------
def orc_hist(datas, max_item=MAX_ITEM):
    h = np.zeros(257, dtype=np.int64)
    for d in datas:
        if d is not None and 0 < d.size <= max_item:
            h[:256] += orc.histogram(d)[:256]
    h[256] = 1
    return h


def orc_body(data, code):
    a = np.ascontiguousarray(data, dtype=np.uint8)
    cap = 4 * a.size + 16
    out = np.zeros(cap, dtype=np.uint8)
    n = orc.lib().orc_encode_body(a.ctypes.data, a.size, C.byref(code), out.ctypes.data, cap)
    assert n != C.c_size_t(-1).value
    return out[:n].copy()


def code_to_device(torch, code):
    """any ctypes code struct (ghf.Code, orc.OrcCode: the same layout) -> a CUDA uint8 tensor (256-byte aligned)"""
    t = torch.from_numpy(np.frombuffer(bytes(code), dtype=np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


class Inputs:
    """items packed at odd addresses with three filler bytes between them; a None item is a null pointer of 100 bytes"""

    def __init__(self, torch, datas):
        self.datas = datas
        self.count = len(datas)
        offs, at = [], 0
        for d in datas:
            at |= 1
            offs.append(at)
            at += (0 if d is None else d.size) + 3
        packed = np.full(at + 16, 0x5A, dtype=np.uint8)
        for o, d in zip(offs, datas):
            if d is not None:
                packed[o : o + d.size] = d
        self.d_in = torch.from_numpy(packed).cuda()
        assert self.d_in.data_ptr() % 16 == 0
        self.sizes = [100 if d is None else int(d.size) for d in datas]
        self.in_ptrs = i64(torch, [0 if d is None else self.d_in.data_ptr() + o for o, d in zip(offs, datas)])
        self.in_bytes = i64(torch, self.sizes)


def histogram_batch(ghf, ctx, torch, inp, max_item, flags=0):
    d_hist = torch.full((257,), -0x0123456789ABCDEF, dtype=torch.int64).cuda()  # garbage: the call overwrites it
    rc = ghf.lib().ghf_histogram_batch(ctx.h, inp.in_ptrs.data_ptr(), inp.in_bytes.data_ptr(), max_item, inp.count, flags,
                                       d_hist.data_ptr())
    assert rc == 0, rc
    return d_hist


class Shared:
    """one ghf_compress_batch_shared call over `inp` under d_code, with everything the checks need kept on the host"""

    def __init__(self, ghf, ctx, torch, inp, d_code, max_item, caps=None, with_index=True, out_shift=None):
        self.ghf, self.ctx, self.torch, self.inp, self.d_code, self.max_item = ghf, ctx, torch, inp, d_code, max_item
        self.count, self.datas, self.sizes = inp.count, inp.datas, inp.sizes
        bound = ghf.compress_batch_shared_bound(max_item)
        self.caps = [bound] * self.count if caps is None else list(caps)
        self.stride = (max(self.caps) + 15 & ~15) + 64
        self.d_out = torch.full((self.count * self.stride + 16,), GUARD, dtype=torch.uint8).cuda()
        shift = out_shift or {}
        self.out_ptrs = i64(torch, [self.d_out.data_ptr() + i * self.stride + shift.get(i, 0) for i in range(self.count)])
        self.out_caps = i64(torch, self.caps)
        self.out_bytes = torch.full((self.count,), -1, dtype=torch.int64).cuda()
        self.status = torch.full((self.count,), -1, dtype=torch.int32).cuda()
        self.bidx = ctx.batch_index_alloc(self.count, max_item) if with_index else None

    def run(self):
        rc = self.ghf.lib().ghf_compress_batch_shared(
            self.ctx.h, self.inp.in_ptrs.data_ptr(), self.inp.in_bytes.data_ptr(), self.max_item, self.count,
            self.d_code.data_ptr(), self.out_ptrs.data_ptr(), self.out_caps.data_ptr(), self.out_bytes.data_ptr(),
            None if self.bidx is None else C.byref(self.bidx), self.status.data_ptr())
        assert rc == 0, rc
        self.ctx.sync()  # raises if the context's status word was latched: per-item failures must not do that
        self.h_out = self.d_out.cpu().numpy()
        self.h_bytes = self.out_bytes.cpu().numpy()
        self.h_status = self.status.cpu().numpy()
        return self

    def body(self, i):
        return self.h_out[i * self.stride : i * self.stride + int(self.h_bytes[i])]

    def slot(self, i):
        return self.h_out[i * self.stride : (i + 1) * self.stride]

    def free(self):
        if self.bidx is not None:
            self.ctx.batch_index_free(self.bidx)
            self.bidx = None


def decode_shared(b, n_symbols=None, stream_bytes=None, d_code=None, d_stream=None, caps=None, bidx=None):
    """ghf_decode_batch_shared on the bodies of `b`: every output at an unaligned address between guard bytes.
    -> (status, out_bytes, list of decoded arrays, list of (front guard, back guard) arrays)"""
    ghf, ctx, torch = b.ghf, b.ctx, b.torch
    n_symbols = b.sizes if n_symbols is None else n_symbols
    ostride = (b.max_item + 15 & ~15) + 64
    d_out = torch.full((b.count * ostride + 64,), GUARD, dtype=torch.uint8).cuda()
    ooff = [i * ostride + 17 + (i % 15) for i in range(b.count)]  # misalignments 1..15 (+ 17)
    out_ptrs = i64(torch, [d_out.data_ptr() + o for o in ooff])
    out_caps = i64(torch, [b.max_item] * b.count if caps is None else caps)
    out_bytes = torch.full((b.count,), -1, dtype=torch.int64).cuda()
    status = torch.full((b.count,), -1, dtype=torch.int32).cuda()
    sp = b.out_ptrs if d_stream is None else i64(torch, [d_stream.data_ptr() + i * b.stride for i in range(b.count)])
    sb = b.out_bytes if stream_bytes is None else i64(torch, stream_bytes)
    cd = b.d_code if d_code is None else d_code
    rc = ghf.lib().ghf_decode_batch_shared(ctx.h, sp.data_ptr(), sb.data_ptr(), cd.data_ptr(), C.byref(b.bidx if bidx is None else bidx),
                                           i64(torch, n_symbols).data_ptr(), b.count, out_ptrs.data_ptr(), out_caps.data_ptr(),
                                           out_bytes.data_ptr(), status.data_ptr())
    assert rc == 0, rc
    ctx.sync()
    h = d_out.cpu().numpy()
    outs, guards = [], []
    for i in range(b.count):
        n = int(n_symbols[i])
        outs.append(h[ooff[i] : ooff[i] + n])
        lo = i * ostride
        guards.append((h[lo : ooff[i]], h[ooff[i] + n : lo + ostride]))
    return status.cpu().numpy(), out_bytes.cpu().numpy(), outs, guards


class World:
    """a batch, its histogram and code from the library, the same from the oracle, and the compressed bodies"""

    def __init__(self, env, datas, max_item):
        ghf, ctx, torch = env
        self.datas, self.max_item = datas, max_item
        self.inp = Inputs(torch, datas)
        self.d_hist = histogram_batch(ghf, ctx, torch, self.inp, max_item)
        self.d_code = ctx.build_code(self.d_hist)
        ctx.sync()
        self.h_hist = self.d_hist.cpu().numpy()
        self.want_hist = orc_hist(datas, max_item)
        self.code = orc.build_code(self.want_hist)  # the oracle's: what every expected body is made with
        self.bodies = [orc_body(d, self.code) for d in datas]
        # caps: every third item gets exactly its size, so that "nothing at or beyond the cap" bites
        bound = ghf.compress_batch_shared_bound(max_item)
        caps = [self.bodies[i].size if i % 3 == 0 else bound for i in range(len(datas))]
        self.b = Shared(ghf, ctx, torch, self.inp, self.d_code, max_item, caps=caps).run()


@pytest.fixture(scope="module")
def small(env):
    datas = [dg.make(["uniform", "zipf", "sym16", "text"][k % 4], n, seed=300 + k) for k, n in enumerate(EDGE_SIZES)]
    w = World(env, datas + small_items(300, seed=12000), 8193)
    yield w
    w.b.free()


@pytest.fixture(scope="module")
def big(env):
    """65 539 bytes, and one item of 1 MiB: 256 rounds"""
    w = World(env, [dg.make("zipf", 65539, seed=401), dg.make("uniform", MAX_ITEM, seed=402), dg.make("text", 5000, seed=403)], MAX_ITEM)
    yield w
    w.b.free()


# ------------------------------------------------------------------------------ 1. histogram
def test_histogram_sums_the_valid_items_and_overwrites(env, small):
    ghf, ctx, torch = env
    assert np.array_equal(small.h_hist, small.want_hist)  # from garbage: the call overwrote d_hist
    # an empty item, a null pointer and an oversize item in the middle change nothing
    datas = list(small.datas[:40])
    datas[10:10] = [np.zeros(0, dtype=np.uint8), None, dg.make("uniform", 8194, seed=5)]
    inp = Inputs(torch, datas)
    got = histogram_batch(ghf, ctx, torch, inp, 8193)
    ctx.sync()
    assert np.array_equal(got.cpu().numpy(), orc_hist(small.datas[:40]))


def test_histogram_cover_all_turns_zeros_into_ones(env):
    ghf, ctx, torch = env
    datas = [dg.make("sym16", n, seed=70 + n) for n in (1, 100, 4097)]
    inp = Inputs(torch, datas)
    want = orc_hist(datas)
    assert np.count_nonzero(want == 0) >= 200
    plain = histogram_batch(ghf, ctx, torch, inp, 8192)
    cover = histogram_batch(ghf, ctx, torch, inp, 8192, flags=COVER_ALL)
    ctx.sync()
    assert np.array_equal(plain.cpu().numpy(), want)
    assert np.array_equal(cover.cpu().numpy(), np.where(want == 0, 1, want))


def test_histogram_workgroups_take_more_than_one_item(env):
    """more than twice the persistent grid (2048 workgroups) of tiny items"""
    ghf, ctx, torch = env
    rng = np.random.default_rng(77)
    sizes = rng.integers(1, 41, size=4200)
    blob = dg.make("zipf", int(sizes.sum()), seed=78)
    cuts = np.concatenate(([0], np.cumsum(sizes)))
    datas = [blob[cuts[i] : cuts[i + 1]] for i in range(sizes.size)]
    inp = Inputs(torch, datas)
    got = histogram_batch(ghf, ctx, torch, inp, 64)
    ctx.sync()
    want = np.concatenate((np.bincount(blob, minlength=256), [1]))
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------ 2. bodies equal the oracle
def _check_bodies(w):
    b = w.b
    assert np.array_equal(w.h_hist, w.want_hist)
    got_code = b.ctx.code_to_host(w.d_code).as_dict()
    assert got_code == w.code.as_dict()  # ghf_build_code on the batch histogram == orc_build_code
    assert np.all(b.h_status == OK), b.h_status.tolist()
    for i, want in enumerate(w.bodies):
        assert int(b.h_bytes[i]) == want.size, (i, w.datas[i].size)
        assert np.array_equal(b.body(i), want), (i, w.datas[i].size)
        assert np.all(b.slot(i)[b.caps[i] :] == GUARD), i  # nothing at or beyond the cap


def test_small_bodies_equal_the_oracle(env, small):
    assert [d.size for d in small.datas[: len(EDGE_SIZES)]] == EDGE_SIZES and len(small.datas) == 312
    _check_bodies(small)


def test_big_bodies_equal_the_oracle(env, big):
    assert [d.size for d in big.datas] == [65539, MAX_ITEM, 5000]
    _check_bodies(big)


# ------------------------------------------------------------------------------ 3. header || body is a .crs2
def _images(w):
    hdr = orc.header_bytes(w.code)
    return [np.concatenate((hdr, w.b.body(i))) for i in range(w.b.count)]


def _decode_images(env, images):
    """ghf_decode_images_batch over all images in one call (sizes pass, then decode pass) -> list of arrays"""
    ghf, ctx, torch = env
    stride = (max(im.size for im in images) + 15 & ~15) + 16
    h = np.zeros(len(images) * stride, dtype=np.uint8)
    for i, im in enumerate(images):
        h[i * stride : i * stride + im.size] = im
    d = torch.from_numpy(h).cuda()
    ptrs = i64(torch, [d.data_ptr() + i * stride for i in range(len(images))])
    nbytes = i64(torch, [im.size for im in images])
    sizes = ctx.decode_images_batch(ptrs, nbytes)
    r = ctx.decode_images_batch(ptrs, nbytes, out=True, caps=sizes["out_bytes"])
    ctx.sync()
    assert sizes["status"].cpu().tolist() == [OK] * len(images) == r["status"].cpu().tolist()
    ho, nb = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
    return [ho[i * r["out_stride"] :][: int(nb[i])] for i in range(len(images))]


@pytest.mark.parametrize("which", ["small", "big"])
def test_stored_header_and_body_is_a_crs2(env, small, big, which, tmp_path):
    w = small if which == "small" else big
    images = _images(w)
    for i, im in enumerate(images):
        assert np.array_equal(orc.decompress(im, cap=w.datas[i].size + 8), w.datas[i]), i
    for i, back in enumerate(_decode_images(env, images)):
        assert np.array_equal(back, w.datas[i]), i
    if orc.have_ref():  # the reference's own decoder on a handful
        for i in ([0, 3, 8, 11, 100, 311] if which == "small" else [0, 2]):
            images[i].tofile(str(tmp_path / "x.crs2"))
            orc.ref_run(["d", str(tmp_path / "x.crs2"), str(tmp_path / "x.de")])
            assert np.array_equal(np.fromfile(str(tmp_path / "x.de"), dtype=np.uint8), w.datas[i]), i


# ------------------------------------------------------------------------------ 4. the single-stream packer agrees
def _check_against_emit(env, w, sample):
    ghf, ctx, torch = env
    b = w.b
    for i in sample:
        d = w.datas[i]
        d_in = torch.from_numpy(d).cuda()
        idx = ctx.index_alloc(d.size)
        cap = ghf.compress_batch_shared_bound(d.size) + 64
        d_out = torch.full((cap,), GUARD, dtype=torch.uint8).cuda()
        start = torch.zeros(1, dtype=torch.int64).cuda()
        ctx.encode_plan(d_in, w.d_code)
        end = ctx.encode_emit(d_in, w.d_code, d_out, start_bit=start, flags=ghf.EMIT_LAST, index=idx)
        ctx.sync()
        nb = int(b.h_bytes[i])
        assert int(end[0].item()) == 8 * nb, i
        assert np.array_equal(d_out[:nb].cpu().numpy(), b.body(i)), i
        want_chunk, want_seg = ctx.index_to_host(idx)
        view = ghf.batch_index_item(b.bidx, i, d.size)
        assert (view.n_chunks, view.n_segs) == (idx.n_chunks, idx.n_segs)
        got_chunk, got_seg = ctx.index_to_host(view)
        assert np.array_equal(got_chunk, want_chunk), i
        assert np.array_equal(got_seg, want_seg), i
        ctx.index_free(idx)


def test_sampled_small_items_equal_encode_emit_with_side_car(env, small):
    _check_against_emit(env, small, [0, 2, 5, 8, 9, 11, 50, 123, 200, 311])


def test_big_items_equal_encode_emit_with_side_car(env, big):
    _check_against_emit(env, big, [0, 1])


# ------------------------------------------------------------------------------ 5. round trip
@pytest.mark.parametrize("which", ["small", "big"])
def test_round_trip(env, small, big, which):
    w = small if which == "small" else big
    status, out_bytes, outs, guards = decode_shared(w.b)
    assert np.all(status == OK), status.tolist()
    for i, d in enumerate(w.datas):
        assert int(out_bytes[i]) == d.size, i
        assert np.array_equal(outs[i], d), i
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i


# ------------------------------------------------------------------------------ 6. codes of up to 32 bits
def test_codes_of_32_bits(env):
    """the two-word stage_put path and the search beyond the 12-bit table: ghf_compress_batch can never meet such a code"""
    ghf, ctx, torch = env
    hist = orc.histogram(CASES["fib32_maxlen32"]())
    code = orc.build_code(hist)
    assert code.max_len == 32
    d_code = ctx.build_code(torch.from_numpy(hist).cuda())
    ctx.sync()
    assert ctx.code_to_host(d_code).as_dict() == code.as_dict()
    rarest = next(s for s in range(256) if code.length[s] == 32)
    used = [s for s in range(256) if code.length[s]]
    rng = np.random.default_rng(32)
    mixed = np.array(used, dtype=np.uint8)[rng.integers(0, len(used), size=9001)]
    datas = [np.full(4097, rarest, dtype=np.uint8), mixed]
    inp = Inputs(torch, datas)
    b = Shared(ghf, ctx, torch, inp, d_code, 9001).run()
    try:
        assert b.h_status.tolist() == [OK, OK]
        assert int(b.h_bytes[0]) == 4 * 4097 + -(-code.length[256] // 8)
        for i, d in enumerate(datas):
            assert np.array_equal(b.body(i), orc_body(d, code)), i
        status, out_bytes, outs, guards = decode_shared(b)
        assert status.tolist() == [OK, OK]
        for i, d in enumerate(datas):
            assert int(out_bytes[i]) == d.size and np.array_equal(outs[i], d), i
            assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    finally:
        b.free()


# ------------------------------------------------------------------------------ 7. per-item failures, compress
def test_compress_failures_are_per_item(env):
    ghf, ctx, torch = env
    max_item = 4999
    good = [d[:max_item] for d in small_items(7, seed=4100)]
    good = [np.where(d == 0xEE, np.uint8(0x11), d) for d in good]
    nocode = good[0].copy()
    nocode[nocode.size // 2] = 0xEE
    short = dg.make("text", 3000, seed=77)
    exact = dg.make("text", 3001, seed=79)
    big = dg.make("zipf", 5000, seed=78)  # one byte too long
    datas = [good[0], np.zeros(0, dtype=np.uint8), good[1], short, good[2], big, good[3], None, good[4], nocode, good[5], good[6], exact]
    hist = orc_hist([d for d in datas if d is not nocode], max_item)
    assert hist[0xEE] == 0
    code = orc.build_code(hist)
    assert code.length[0xEE] == 0
    d_code = code_to_device(torch, code)
    bound = ghf.compress_batch_shared_bound(max_item)
    caps = [bound] * len(datas)
    caps[3] = orc_body(short, code).size - 1  # one byte short
    caps[12] = orc_body(exact, code).size     # exactly enough
    inp = Inputs(torch, datas)
    b = Shared(ghf, ctx, torch, inp, d_code, max_item, caps=caps, out_shift={10: 8}).run()  # run() ends with ctx.sync(): it stays OK
    try:
        want = [OK, E_EMPTY, OK, E_CAP, OK, E_INVAL, OK, E_INVAL, OK, E_NOCODE, E_INVAL, OK, OK]
        assert b.h_status.tolist() == want
        for i, d in enumerate(datas):
            if want[i] == OK:
                assert np.array_equal(b.body(i), orc_body(d, code)), i
                assert np.all(b.slot(i)[caps[i] :] == GUARD), i
            else:
                assert int(b.h_bytes[i]) == 0, i
                assert np.all(b.slot(i) == GUARD), i  # a refused item writes nothing at all
    finally:
        b.free()


def test_compress_refuses_a_code_that_is_not_complete_on_every_item(env, small):
    ghf, ctx, torch = env
    datas = small.datas[12:18]
    inp = Inputs(torch, datas)
    good = ghf.Code.from_buffer_copy(bytes(small.code))
    cases = bad_codes(good, ghf.Code.from_buffer_copy)
    sixty = ghf.Code.from_buffer_copy(bytes(good))
    sixty.length[next(s for s in range(256) if good.length[s] == good.max_len)] = 60  # must not reach the packer
    no_end = ghf.Code.from_buffer_copy(bytes(good))
    no_end.max_len = 0
    for name, c in cases + [("a length of 60", sixty), ("max_len 0", no_end)]:
        b = Shared(ghf, ctx, torch, inp, code_to_device(torch, c), 8193).run()
        try:
            assert b.h_status.tolist() == [E_FORMAT] * len(datas), name
            assert np.all(b.h_bytes == 0), name
            assert np.all(b.h_out == GUARD), name  # nothing is written
        finally:
            b.free()


# ------------------------------------------------------------------------------ 8. per-item failures, decode
def length_changing_flip(data, code, body):
    """A bit of `body` whose flip makes segment 20 miss its recorded end: decoding its 64 symbols from the flipped bits (on
    the host, with the oracle's code) uses another number of bits.  (As in tests/test_gpu_batch.py, for a body at bit 0.)"""
    c = code.as_dict()
    length, codeword = c["length"], c["codeword"]
    book = {(length[s], codeword[s]): s for s in range(257) if length[s]}
    bits = np.unpackbits(body)
    lens = np.asarray(length, dtype=np.int64)[data]
    starts = np.concatenate(([0], np.cumsum(lens)))
    seg = 20  # symbols [1280, 1344)
    a, e = int(starts[64 * seg]), int(starts[64 * seg + 64])
    for k in range(5, 40):
        cand = int(starts[64 * seg + k])  # the first bit of the k-th code of the segment
        work = bits.copy()
        work[cand] ^= 1
        at, ok = a, True
        for _ in range(64):
            v, l = 0, 0
            while (l, v) not in book and l < 33:
                v, l = (v << 1) | int(work[at + l]), l + 1
            if (l, v) not in book:
                ok = False
                break
            at += l
        if not ok or at != e:
            return cand
    raise AssertionError("no length-changing flip found")


def test_decode_failures_are_per_item(env):
    ghf, ctx, torch = env
    datas = small_items(10, seed=5200)
    datas[2] = dg.make("zipf", 6000, seed=91)
    datas[6] = dg.make("text", 7000, seed=92)
    w = World(env, datas, 8192)
    b = w.b
    try:
        assert np.all(b.h_status == OK)
        h = b.h_out.copy()
        flip_bit = length_changing_flip(datas[2], w.code, w.bodies[2])
        h[2 * b.stride + flip_bit // 8] ^= 0x80 >> (flip_bit % 8)
        d_stream = torch.from_numpy(h).cuda()
        stream_bytes = [int(x) for x in b.h_bytes]
        end_len = w.code.length[256]
        total_bits = int(np.asarray(list(w.code.length))[datas[6]].sum()) + end_len
        assert end_len > 8 and stream_bytes[6] == -(-total_bits // 8)
        stream_bytes[6] = (total_bits - 1) // 8  # without the byte of the end mark's last bit: the cut lies inside the mark
        caps = [8192] * len(datas)
        caps[4] = datas[4].size - 1
        n_symbols = [d.size for d in datas]
        n_symbols[8] = 0
        # a side-car slice whose chunk_bit points beyond the stream: a copy of the index with item 9's first block moved
        bent = ctx.batch_index_alloc(b.count, 8192)
        L = ghf.lib()
        chunk = np.zeros(b.count * bent.blocks_per_item, dtype=np.uint64)
        seg = np.zeros(b.count * bent.segs_per_item, dtype=np.uint32)
        assert L.ghf_copy_d2h(ctx.h, chunk.ctypes.data, b.bidx.d_chunk_bit, chunk.nbytes) == 0
        assert L.ghf_copy_d2h(ctx.h, seg.ctypes.data, b.bidx.d_seg_bit, seg.nbytes) == 0
        ctx.sync()
        chunk[9 * bent.blocks_per_item] = 8 * stream_bytes[9] + 1
        assert L.ghf_copy_h2d(ctx.h, bent.d_chunk_bit, chunk.ctypes.data, chunk.nbytes) == 0
        assert L.ghf_copy_h2d(ctx.h, bent.d_seg_bit, seg.ctypes.data, seg.nbytes) == 0
        ctx.sync()
        status, out_bytes, outs, guards = decode_shared(b, n_symbols=n_symbols, stream_bytes=stream_bytes, d_stream=d_stream,
                                                        caps=caps, bidx=bent)
        ctx.batch_index_free(bent)
        want = [OK, OK, E_CORRUPT, OK, E_CAP, OK, E_CORRUPT, OK, E_EMPTY, E_CORRUPT]
        assert status.tolist() == want
        for i, d in enumerate(datas):
            if want[i] == OK:
                assert int(out_bytes[i]) == d.size and np.array_equal(outs[i], d), i
            else:
                assert int(out_bytes[i]) == 0, i
            assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
        # an incomplete code: GHF_E_FORMAT for all items
        c = ghf.Code.from_buffer_copy(bytes(w.code))
        c.length[next(s for s in range(256) if c.length[s])] += 1  # the Kraft sum is no longer 1
        status, out_bytes, outs, guards = decode_shared(b, d_code=code_to_device(torch, c))
        assert status.tolist() == [E_FORMAT] * b.count and np.all(out_bytes == 0)
        for i in range(b.count):
            assert np.all(outs[i] == GUARD) and np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    finally:
        b.free()


@pytest.mark.parametrize("refusal", ["empty", "cap"])
def test_a_broken_shared_code_comes_before_an_items_own_refusal(env, refusal):
    """the order of the verdicts of k_decode_batch_shared and k_decode_bodies_batch_shared: the code is vetted before the
    item is looked at, so a code broken by its length bounds or by its Kraft sum (the two ways batch_code_ok refuses) gives
    GHF_E_FORMAT on every item, the one with a refusal of its own included, and no byte of any output is written.  Three
    items of 65 bytes: one whole segment and a ragged one.  (ghf_decode_bodies_batch_shared takes no symbol counts: there
    item 1's own refusal is the cap of 64 in both cases.)"""
    ghf, ctx, torch = env
    datas = [dg.make("zipf", 65, seed=6200 + i) for i in range(3)]
    w = World(env, datas, 4096)
    b = w.b
    try:
        assert np.all(b.h_status == OK)
        n_symbols, caps = [65, 65, 65], [4096] * 3
        if refusal == "empty":
            n_symbols[1] = 0
        else:
            caps[1] = 64
        mine = E_EMPTY if refusal == "empty" else E_CAP

        def bodies(d_code):  # ghf_decode_bodies_batch_shared into 65-byte slots between guard bytes, item 1 capped at 64
            d_out = torch.full((3 * 128,), GUARD, dtype=torch.uint8).cuda()
            out_ptrs = i64(torch, [d_out.data_ptr() + 128 * i + 17 + i for i in range(3)])
            out_bytes = torch.full((3,), -1, dtype=torch.int64).cuda()
            status = torch.full((3,), -1, dtype=torch.int32).cuda()
            out_caps = i64(torch, [65, 64, 65])
            rc = ghf.lib().ghf_decode_bodies_batch_shared(ctx.h, b.out_ptrs.data_ptr(), b.out_bytes.data_ptr(), d_code.data_ptr(), 3,
                                                          out_ptrs.data_ptr(), out_caps.data_ptr(), out_bytes.data_ptr(),
                                                          status.data_ptr())
            assert rc == 0, rc
            ctx.sync()
            return status.cpu().numpy(), out_bytes.cpu().numpy(), d_out.cpu().numpy()

        # the good code: item 1's own refusal is real, its neighbours decode
        status, out_bytes, outs, guards = decode_shared(b, n_symbols=n_symbols, caps=caps)
        assert status.tolist() == [OK, mine, OK] and out_bytes.tolist() == [65, 0, 65]
        assert np.array_equal(outs[0], datas[0]) and np.array_equal(outs[2], datas[2])
        status, out_bytes, h = bodies(b.d_code)
        assert status.tolist() == [OK, E_CAP, OK] and out_bytes.tolist() == [65, 0, 65]
        assert np.array_equal(h[17:82], datas[0]) and np.array_equal(h[256 + 19 :][:65], datas[2])
        for name, c in vet_branch_codes(ghf.Code.from_buffer_copy(bytes(w.code)), ghf.Code.from_buffer_copy):
            d_code = code_to_device(torch, c)
            status, out_bytes, outs, guards = decode_shared(b, n_symbols=n_symbols, caps=caps, d_code=d_code)
            print(name, status.tolist(), out_bytes.tolist())
            assert status.tolist() == [E_FORMAT] * 3 and out_bytes.tolist() == [0, 0, 0], name
            for i in range(3):
                assert np.all(outs[i] == GUARD) and np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (name, i)
            status, out_bytes, h = bodies(d_code)
            print(name, "bodies", status.tolist(), out_bytes.tolist())
            assert status.tolist() == [E_FORMAT] * 3 and out_bytes.tolist() == [0, 0, 0], name
            assert np.all(h == GUARD), name
    finally:
        b.free()


# ------------------------------------------------------------------------------ 9. call-level errors
def test_call_level_argument_errors(env, small):
    ghf, ctx, torch = env
    L = ghf.lib()
    datas = small.datas[12:16]
    inp = Inputs(torch, datas)
    b = Shared(ghf, ctx, torch, inp, small.d_code, 8193)
    d_hist = torch.full((257,), 7, dtype=torch.int64).cuda()
    try:
        P = lambda t: None if t is None else t.data_ptr()
        hist = lambda ptrs=inp.in_ptrs, nb=inp.in_bytes, mx=8193, count=4, flags=0, out=d_hist: L.ghf_histogram_batch(
            ctx.h, P(ptrs), P(nb), mx, count, flags, P(out))
        comp = lambda ptrs=inp.in_ptrs, mx=8193, count=4, code=small.d_code.data_ptr(), outp=b.out_ptrs, bidx=b.bidx, st=b.status: \
            L.ghf_compress_batch_shared(ctx.h, P(ptrs), P(inp.in_bytes), mx, count, code, P(outp), P(b.out_caps), P(b.out_bytes),
                                        None if bidx is None else C.byref(bidx), P(st))
        dec = lambda sp=b.out_ptrs, code=small.d_code.data_ptr(), bidx=b.bidx, count=4, st=b.status: \
            L.ghf_decode_batch_shared(ctx.h, P(sp), P(b.out_bytes), code, None if bidx is None else C.byref(bidx), P(inp.in_bytes),
                                      count, P(b.out_ptrs), P(b.out_caps), P(b.out_bytes), P(st))
        # count == 0 queues nothing
        assert hist(count=0) == OK and comp(count=0) == OK and dec(count=0) == OK
        ctx.sync()
        assert np.all(d_hist.cpu().numpy() == 7) and np.all(b.status.cpu().numpy() == -1) and np.all(b.d_out.cpu().numpy() == GUARD)
        # null arrays, max_item_bytes, unknown flags
        assert hist(ptrs=None) == E_INVAL and hist(nb=None) == E_INVAL and hist(out=None) == E_INVAL
        assert hist(mx=0) == E_INVAL and hist(mx=MAX_ITEM + 1) == E_INVAL and hist(flags=2) == E_INVAL
        assert comp(ptrs=None) == E_INVAL and comp(outp=None) == E_INVAL and comp(st=None) == E_INVAL
        assert comp(mx=0) == E_INVAL and comp(mx=MAX_ITEM + 1) == E_INVAL
        assert dec(sp=None) == E_INVAL and dec(st=None) == E_INVAL and dec(bidx=None) == E_INVAL
        # a null or misaligned d_code
        assert comp(code=None) == E_INVAL and comp(code=small.d_code.data_ptr() + 8) == E_INVAL
        assert dec(code=None) == E_INVAL and dec(code=small.d_code.data_ptr() + 4) == E_INVAL
        # an index whose geometry does not cover (count, max_item_bytes)
        few = ctx.batch_index_alloc(2, 8193)
        narrow = ctx.batch_index_alloc(4, 8192)
        bent = ghf.BatchIndex.from_buffer_copy(bytes(b.bidx))
        bent.segs_per_item += 1
        assert comp(bidx=few) == E_INVAL and comp(bidx=narrow) == E_INVAL and comp(bidx=bent) == E_INVAL
        assert dec(bidx=few) == E_INVAL and dec(bidx=bent) == E_INVAL
        ctx.batch_index_free(few)
        ctx.batch_index_free(narrow)
        ctx.sync()
        assert np.all(d_hist.cpu().numpy() == 7) and np.all(b.status.cpu().numpy() == -1) and np.all(b.d_out.cpu().numpy() == GUARD)
        assert comp(bidx=None) == OK  # the index is optional for compress, and the context is still usable
        ctx.sync()
        assert b.status.cpu().tolist() == [OK] * 4
    finally:
        b.free()


# ------------------------------------------------------------------------------ 10. python wrappers
def test_python_wrappers_round_trip(env):
    ghf, ctx, torch = env
    datas = small_items(16, seed=7400)
    tensors = [torch.from_numpy(d).cuda() for d in datas]
    bidx = ctx.batch_index_alloc(len(datas), 8192)
    try:
        d_hist = ctx.histogram_batch(tensors, max_item_bytes=8192)
        d_code = ctx.build_code(d_hist)
        r = ctx.compress_batch_shared(tensors, d_code, max_item_bytes=8192, index=bidx)
        dec = ctx.decode_batch_shared(r["out_ptrs"], r["out_bytes"], d_code, bidx, r["in_bytes"])
        packed = torch.from_numpy(np.concatenate(datas)).cuda()
        h2 = ctx.histogram_batch(packed, sizes=[d.size for d in datas], flags=ghf.HIST_COVER_ALL)
        ctx.sync()
        want_hist = orc_hist(datas)
        assert np.array_equal(d_hist.cpu().numpy(), want_hist)
        assert np.array_equal(h2.cpu().numpy(), np.where(want_hist == 0, 1, want_hist))
        code = orc.build_code(want_hist)
        assert r["status"].cpu().tolist() == [OK] * 16 == dec["status"].cpu().tolist()
        h, nb, ho = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy(), dec["out"].cpu().numpy()
        for i, d in enumerate(datas):
            assert np.array_equal(h[i * r["out_stride"] :][: nb[i]], orc_body(d, code)), i
            assert np.array_equal(ho[i * dec["out_stride"] :][: d.size], d), i
    finally:
        ctx.batch_index_free(bidx)
