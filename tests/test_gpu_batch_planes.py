"""GPU: ghf_histogram_batch_planes / ghf_build_codes / ghf_compress_batch_planes_shared / ghf_decode_batch_planes_shared /
ghf_decode_bodies_batch_planes_shared -- many small items of typed elements under ONE code per byte plane.

Expected values come from the CPU oracle on data[p::E] (orc.histogram, orc_build_code, orc_encode_body, orc_decompress;
pinned to the reference by tests/test_oracle_golden.py), as tests/test_gpu_batch_shared.py does it; the flat
ghf_compress_batch_shared on the materialised plane bytes gives the expected side-car.  Inputs and decode outputs sit at
odd addresses between 0xA5 guards.  Every case runs for E in {2, 4, 8}.

The size claim (test_planes_store_less_than_one_flat_code): 64 items of 2048 standard-normal bf16 values from
default_rng(7), 262 144 raw bytes: 203 805 body bytes under one flat GHF_HIST_COVER_ALL code, 175 235 under two plane
codes (0.860), both computed by the oracle."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import pkgload
from header_cases import bad_codes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT, E_NOCODE = 0, 1, 3, 5, 6, 7, 10
GUARD = 0xA5
COVER_ALL = 1
CODE_LIMIT = 1
ES = [2, 4, 8]
# element counts: the vector and segment edges; round edges and the carried unit
EDGE_ELEMS = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8193]
FLAT_BYTES, PLANES_BYTES = 203805, 175235  # the size claim, recorded (see the module docstring)


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


def normal_elems(rng, n, e):
    """n standard-normal values as bf16 (the high half of the fp32), fp32 or fp64 -> uint8[n * e]"""
    x = rng.standard_normal(n)
    if e == 2:
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()
    return x.astype(np.float32 if e == 4 else np.float64).view(np.uint8).copy()


# ---- the oracle's side ------------------------------------------------------------------------------------------------
def valid(d, e, max_item):
    return d is not None and 0 < d.size <= max_item and d.size % e == 0


def orc_hists(datas, e, max_item, cover=False):
    h = np.zeros((e, 257), dtype=np.int64)
    for d in datas:
        if valid(d, e, max_item):
            for p in range(e):
                h[p, :256] += orc.histogram(np.ascontiguousarray(d[p::e]))[:256]
    if cover:
        h[h == 0] = 1
    h[:, 256] = 1
    return h


def orc_body(data, code):
    a = np.ascontiguousarray(data, dtype=np.uint8)
    cap = 4 * a.size + 16
    out = np.zeros(cap, dtype=np.uint8)
    n = orc.lib().orc_encode_body(a.ctypes.data, a.size, C.byref(code), out.ctypes.data, cap)
    assert n != C.c_size_t(-1).value
    return out[:n].copy()


def codes_to_device(torch, codes):
    """ctypes code structs (ghf.Code, orc.OrcCode: the same layout) -> a CUDA uint8 tensor [E, sizeof(Code)]"""
    t = torch.from_numpy(np.stack([np.frombuffer(bytes(c), dtype=np.uint8) for c in codes]).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


class Inputs:
    """items packed at odd addresses with three filler bytes between them; a None item is a null pointer of 96 bytes"""

    def __init__(self, torch, datas):
        self.datas, self.count = datas, len(datas)
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
        self.sizes = [96 if d is None else int(d.size) for d in datas]
        self.in_ptrs = i64(torch, [0 if d is None else self.d_in.data_ptr() + o for o, d in zip(offs, datas)])
        self.in_bytes = i64(torch, self.sizes)


def histogram_planes(ghf, ctx, torch, inp, e, max_item, flags=0):
    d_hists = torch.full((e, 257), -0x0123456789ABCDEF, dtype=torch.int64).cuda()  # garbage: the call overwrites it
    rc = ghf.lib().ghf_histogram_batch_planes(ctx.h, inp.in_ptrs.data_ptr(), inp.in_bytes.data_ptr(), max_item, inp.count, e, flags,
                                              d_hists.data_ptr())
    assert rc == 0, rc
    return d_hists


class Planes:
    """one ghf_compress_batch_planes_shared call over `inp` under d_codes, with everything the checks need kept on the host"""

    def __init__(self, ghf, ctx, torch, inp, d_codes, e, max_item, caps=None, with_index=True):
        self.ghf, self.ctx, self.torch, self.inp, self.d_codes, self.e, self.max_item = ghf, ctx, torch, inp, d_codes, e, max_item
        self.count, self.slots, self.datas = inp.count, inp.count * e, inp.datas
        bound = ghf.compress_batch_planes_shared_bound(max_item, e)
        self.caps = [bound] * self.slots if caps is None else list(caps)
        self.stride = (max(self.caps) + 15 & ~15) + 64
        self.d_out = torch.full((self.slots * self.stride + 16,), GUARD, dtype=torch.uint8).cuda()
        self.out_ptrs = i64(torch, [self.d_out.data_ptr() + j * self.stride for j in range(self.slots)])
        self.out_caps = i64(torch, self.caps)
        self.out_bytes = torch.full((self.slots,), -1, dtype=torch.int64).cuda()
        self.status = torch.full((self.slots,), -1, dtype=torch.int32).cuda()
        self.bidx = ctx.batch_index_alloc(self.slots, max_item // e) if with_index else None

    def run(self):
        rc = self.ghf.lib().ghf_compress_batch_planes_shared(
            self.ctx.h, self.inp.in_ptrs.data_ptr(), self.inp.in_bytes.data_ptr(), self.max_item, self.count, self.e,
            self.d_codes.data_ptr(), self.out_ptrs.data_ptr(), self.out_caps.data_ptr(), self.out_bytes.data_ptr(),
            None if self.bidx is None else C.byref(self.bidx), self.status.data_ptr())
        assert rc == 0, rc
        self.ctx.sync()  # raises if the context's status word was latched: per-slot failures must not do that
        self.h_out = self.d_out.cpu().numpy()
        self.h_bytes = self.out_bytes.cpu().numpy()
        self.h_status = self.status.cpu().numpy()
        return self

    def body(self, j):
        return self.h_out[j * self.stride : j * self.stride + int(self.h_bytes[j])]

    def slot(self, j):
        return self.h_out[j * self.stride : (j + 1) * self.stride]

    def free(self):
        if self.bidx is not None:
            self.ctx.batch_index_free(self.bidx)
            self.bidx = None


def decode(b, live, n_elems=None, stream_bytes=None, d_codes=None, d_stream=None, caps=None, sizes_only=False):
    """ghf_decode_batch_planes_shared (live side-car) or ghf_decode_bodies_batch_planes_shared on the bodies of `b`: every
    output at an unaligned address between guard bytes.  -> (status, out_bytes, decoded arrays, (front, back) guards)"""
    ghf, ctx, torch, e = b.ghf, b.ctx, b.torch, b.e
    want = [s if s % e == 0 else 0 for s in b.inp.sizes] if n_elems is None else [n * e for n in n_elems]
    ostride = (b.max_item + 15 & ~15) + 64
    d_out = torch.full((b.count * ostride + 64,), GUARD, dtype=torch.uint8).cuda()
    ooff = [i * ostride + 17 + (i % 15) for i in range(b.count)]  # misalignments 1..15 (+ 17)
    out_ptrs = i64(torch, [d_out.data_ptr() + o for o in ooff])
    out_caps = i64(torch, [b.max_item] * b.count if caps is None else caps)
    out_bytes = torch.full((b.count,), -1, dtype=torch.int64).cuda()
    status = torch.full((b.count,), -1, dtype=torch.int32).cuda()
    sp = b.out_ptrs if d_stream is None else i64(torch, [d_stream.data_ptr() + j * b.stride for j in range(b.slots)])
    sb = b.out_bytes if stream_bytes is None else i64(torch, stream_bytes)
    cd = b.d_codes if d_codes is None else d_codes
    if live:
        rc = ghf.lib().ghf_decode_batch_planes_shared(ctx.h, sp.data_ptr(), sb.data_ptr(), cd.data_ptr(), C.byref(b.bidx),
                                                      i64(torch, [w // e for w in want]).data_ptr(), b.count, e, out_ptrs.data_ptr(),
                                                      out_caps.data_ptr(), out_bytes.data_ptr(), status.data_ptr())
    else:
        rc = ghf.lib().ghf_decode_bodies_batch_planes_shared(ctx.h, sp.data_ptr(), sb.data_ptr(), cd.data_ptr(), b.count, e,
                                                             None if sizes_only else out_ptrs.data_ptr(), out_caps.data_ptr(),
                                                             out_bytes.data_ptr(), status.data_ptr())
    assert rc == 0, rc
    ctx.sync()
    h = d_out.cpu().numpy()
    outs, guards = [], []
    for i in range(b.count):
        n = 0 if sizes_only else int(want[i])
        outs.append(h[ooff[i] : ooff[i] + n])
        guards.append((h[i * ostride : ooff[i]], h[ooff[i] + n : (i + 1) * ostride]))
    return status.cpu().numpy(), out_bytes.cpu().numpy(), outs, guards


class World:
    """a batch, its histograms and codes from the library, the same from the oracle, and the compressed bodies"""

    def __init__(self, env, datas, e, max_item, cover=False):
        ghf, ctx, torch = env
        self.datas, self.e, self.max_item = datas, e, max_item
        self.inp = Inputs(torch, datas)
        self.d_hists = histogram_planes(ghf, ctx, torch, self.inp, e, max_item, COVER_ALL if cover else 0)
        self.d_codes = ctx.build_codes(self.d_hists)
        ctx.sync()
        self.h_hists = self.d_hists.cpu().numpy()
        self.want_hists = orc_hists(datas, e, max_item, cover)
        self.codes = [orc.build_code(np.ascontiguousarray(self.want_hists[p])) for p in range(e)]  # the oracle's
        self.planes = [[np.ascontiguousarray(d[p::e]) for p in range(e)] for d in datas]
        self.bodies = [orc_body(pl[p], self.codes[p]) for pl in self.planes for p in range(e)]  # by slot
        # caps: every third slot gets exactly its size, so that "nothing at or beyond the cap" bites
        bound = ghf.compress_batch_planes_shared_bound(max_item, e)
        caps = [self.bodies[j].size if j % 3 == 0 else bound for j in range(len(self.bodies))]
        self.b = Planes(ghf, ctx, torch, self.inp, self.d_codes, e, max_item, caps=caps).run()


_worlds = {}


def world(env, name, e):
    """the three shared batches, built once per width and kept for the module"""
    if (name, e) not in _worlds:
        if name == "edge":
            # (no byte value above 239: GHF_HIST_COVER_ALL has zeros to turn into ones)
            datas = [np.minimum(dg.make(["uniform", "zipf", "sym16", "text"][k % 4], n * e, seed=900 + 16 * e + k), np.uint8(239))
                     for k, n in enumerate(EDGE_ELEMS)]
            _worlds[name, e] = World(env, datas, e, 8193 * e)
        elif name == "normal":  # 16 items of 2048 standard-normal elements
            rng = np.random.default_rng(7)
            _worlds[name, e] = World(env, [normal_elems(rng, 2048, e) for _ in range(16)], e, 2048 * e, cover=True)
        else:  # 3 items of 40 000 elements: the bodies decoder takes several rounds per plane
            rng = np.random.default_rng(11)
            _worlds[name, e] = World(env, [normal_elems(rng, 40000, e) for _ in range(3)], e, 40000 * e, cover=True)
    return _worlds[name, e]


@pytest.fixture(scope="module", autouse=True)
def _free_worlds():
    yield
    for w in _worlds.values():
        w.b.free()
    _worlds.clear()


# ------------------------------------------------------------------------------ 1. histograms
@pytest.mark.parametrize("e", ES)
def test_histograms_equal_the_oracle_per_plane(env, e):
    ghf, ctx, torch = env
    w = world(env, "edge", e)
    assert [d.size // e for d in w.datas] == EDGE_ELEMS
    assert np.array_equal(w.h_hists, w.want_hists)  # from garbage: the call overwrote d_hists
    cover = histogram_planes(ghf, ctx, torch, w.inp, e, w.max_item, flags=COVER_ALL)
    # an odd-sized item, an empty one, a null pointer and an over-long one in the middle change nothing
    datas = list(w.datas)
    datas[5:5] = [dg.make("uniform", 7 * e + 1, seed=5), np.zeros(0, dtype=np.uint8), None, dg.make("uniform", 8194 * e, seed=6)]
    assert all(x is None or not valid(x, e, w.max_item) for x in datas[5:9])
    got = histogram_planes(ghf, ctx, torch, Inputs(torch, datas), e, w.max_item)
    ctx.sync()
    assert np.count_nonzero(w.want_hists == 0) > 0
    assert np.array_equal(cover.cpu().numpy(), orc_hists(w.datas, e, w.max_item, cover=True))
    assert np.array_equal(got.cpu().numpy(), w.want_hists)


def test_histogram_workgroups_take_more_than_one_item(env):
    """more than twice the persistent grid (2048 workgroups) of tiny items"""
    ghf, ctx, torch = env
    rng = np.random.default_rng(77)
    sizes = 4 * rng.integers(1, 11, size=4200)
    blob = dg.make("zipf", int(sizes.sum()), seed=78)
    cuts = np.concatenate(([0], np.cumsum(sizes)))
    datas = [blob[cuts[i] : cuts[i + 1]] for i in range(sizes.size)]
    got = histogram_planes(ghf, ctx, torch, Inputs(torch, datas), 4, 64)
    ctx.sync()
    assert np.array_equal(got.cpu().numpy(), orc_hists(datas, 4, 64))


# ------------------------------------------------------------------------------ 2. the code builds
@pytest.mark.parametrize("e", ES)
def test_build_codes_equals_separate_builds(env, e):
    ghf, ctx, torch = env
    w = world(env, "edge", e)
    size = C.sizeof(ghf.Code)
    for flags in (0, CODE_LIMIT):
        many = ctx.build_codes(w.d_hists, flags=flags)
        ones = [ctx.build_code(w.d_hists[p], flags=flags) for p in range(e)]  # flags == 0: ghf_build_code, else ghf_build_code_ex
        ctx.sync()
        h = many.cpu().numpy()
        for p in range(e):
            assert np.array_equal(h[p], ones[p].cpu().numpy().reshape(-1)[:size]), (p, flags)
    got = w.d_codes.cpu().numpy()
    for p in range(e):
        assert ghf.Code.from_buffer_copy(got[p].tobytes()).as_dict() == w.codes[p].as_dict(), p  # == orc_build_code


# ------------------------------------------------------------------------------ 3. bodies, images, side-car
def _check_bodies(w):
    b = w.b
    assert np.array_equal(w.h_hists, w.want_hists)
    assert np.all(b.h_status == OK), b.h_status.tolist()
    for j, want in enumerate(w.bodies):
        assert int(b.h_bytes[j]) == want.size, j
        assert np.array_equal(b.body(j), want), j
        assert np.all(b.slot(j)[b.caps[j] :] == GUARD), j  # nothing at or beyond the cap


@pytest.mark.parametrize("e", ES)
def test_edge_bodies_equal_the_oracle_and_are_crs2_behind_their_header(env, e):
    w = world(env, "edge", e)
    _check_bodies(w)
    for i, pl in enumerate(w.planes):
        for p in range(e):
            image = np.concatenate((orc.header_bytes(w.codes[p]), w.b.body(i * e + p)))
            assert np.array_equal(orc.decompress(image, cap=pl[p].size + 8), pl[p]), (i, p)


@pytest.mark.parametrize("e", ES)
def test_side_car_slices_equal_the_flat_call_on_the_plane_bytes(env, e):
    ghf, ctx, torch = env
    w = world(env, "edge", e)
    b = w.b
    L = ghf.lib()

    def arrays(bidx, slots):
        chunk = np.zeros(slots * bidx.blocks_per_item, dtype=np.uint64)
        seg = np.zeros(slots * bidx.segs_per_item, dtype=np.uint32)
        assert L.ghf_copy_d2h(ctx.h, chunk.ctypes.data, bidx.d_chunk_bit, chunk.nbytes) == 0
        assert L.ghf_copy_d2h(ctx.h, seg.ctypes.data, bidx.d_seg_bit, seg.nbytes) == 0
        ctx.sync()
        return chunk.reshape(slots, -1), seg.reshape(slots, -1)

    got_chunk, got_seg = arrays(b.bidx, b.slots)
    for p in range(e):
        flat_in = Inputs(torch, [pl[p] for pl in w.planes])
        fidx = ctx.batch_index_alloc(b.count, w.max_item // e)
        r_ptrs, r = flat_in.in_ptrs, None
        bound = ghf.compress_batch_shared_bound(w.max_item // e)
        d_out = torch.empty(b.count * bound, dtype=torch.uint8).cuda()
        out_ptrs = i64(torch, [d_out.data_ptr() + i * bound for i in range(b.count)])
        st = torch.full((b.count,), -1, dtype=torch.int32).cuda()
        nb = torch.zeros(b.count, dtype=torch.int64).cuda()
        d_code = w.d_codes[p].clone()  # (a tensor of its own: the flat call wants its code 16-byte aligned)
        rc = L.ghf_compress_batch_shared(ctx.h, r_ptrs.data_ptr(), flat_in.in_bytes.data_ptr(), w.max_item // e, b.count,
                                         d_code.data_ptr(), out_ptrs.data_ptr(), i64(torch, [bound] * b.count).data_ptr(),
                                         nb.data_ptr(), C.byref(fidx), st.data_ptr())
        assert rc == 0
        ctx.sync()
        assert st.cpu().tolist() == [OK] * b.count
        want_chunk, want_seg = arrays(fidx, b.count)
        ctx.batch_index_free(fidx)
        for i, pl in enumerate(w.planes):
            n = pl[p].size
            nblk, nseg = -(-n // 4096), -(-n // 64)
            assert np.array_equal(got_chunk[i * e + p][:nblk], want_chunk[i][:nblk]), (i, p)
            assert np.array_equal(got_seg[i * e + p][:nseg], want_seg[i][:nseg]), (i, p)


# ------------------------------------------------------------------------------ 4. round trips
@pytest.mark.parametrize("which", ["edge", "normal", "long"])
@pytest.mark.parametrize("e", ES)
def test_round_trips_through_both_decoders(env, e, which):
    w = world(env, which, e)
    _check_bodies(w)
    if which == "normal" and e == 2:  # the hard corners: a high plane beyond the 12-bit table, a low plane of 7..10-bit codes
        assert w.codes[1].max_len > 12 and w.codes[0].min_len >= 7 and w.codes[0].max_len <= 10
    for live in (True, False):
        status, out_bytes, outs, guards = decode(w.b, live)
        assert np.all(status == OK), (live, status.tolist())
        for i, d in enumerate(w.datas):
            assert int(out_bytes[i]) == d.size, (live, i)
            assert np.array_equal(outs[i], d), (live, i)
            assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (live, i)
    status, out_bytes, _, guards = decode(w.b, False, sizes_only=True)
    assert np.all(status == OK) and out_bytes.tolist() == [d.size for d in w.datas]
    assert all(np.all(g[0] == GUARD) and np.all(g[1] == GUARD) for g in guards)


def test_bodies_decoder_counts_its_rounds_and_passes(env):
    ghf, ctx, torch = env
    w = world(env, "long", 2)
    stats = torch.zeros(2, dtype=torch.int64).cuda()
    ctx.decode_images_batch_stats(stats)
    try:
        decode(w.b, False, sizes_only=True)
    finally:
        ctx.decode_images_batch_stats(None)
    rounds, passes = stats.cpu().tolist()
    assert rounds > 2 * w.b.count and passes >= rounds  # several rounds per plane: 40 000 symbols of ~8 bits in rounds of 131 072 bits


# ------------------------------------------------------------------------------ 5. per-slot failures, compress
@pytest.mark.parametrize("e", ES)
def test_compress_failures_are_per_slot(env, e):
    ghf, ctx, torch = env
    rng = np.random.default_rng(50 + e)
    max_item = 3000 * e
    good = [dg.make(["zipf", "text", "sym16"][k % 3], (500 + 411 * k) * e, seed=4100 + k) for k in range(6)]
    good = [np.where(d == 0xEE, np.uint8(0x11), d) for d in good]
    nocode = good[0].copy()
    nocode[e * 100 + (e - 1)] = 0xEE  # in the last plane only
    short = dg.make("text", 1000 * e, seed=77)
    datas = [good[0], dg.make("uniform", 7 * e + 1, seed=1), good[1], np.zeros(0, dtype=np.uint8), good[2], None, good[3],
             dg.make("zipf", 3001 * e, seed=78), good[4], short, good[5], nocode]
    hists = orc_hists([d for d in datas if d is not nocode], e, max_item)
    assert hists[e - 1, 0xEE] == 0
    codes = [orc.build_code(np.ascontiguousarray(hists[p])) for p in range(e)]
    bound = ghf.compress_batch_planes_shared_bound(max_item, e)
    caps = [bound] * (len(datas) * e)
    caps[9 * e + 1] = orc_body(short[1::e], codes[1]).size - 1  # one byte short on one slot
    per_item = [OK, E_INVAL, OK, E_EMPTY, OK, E_INVAL, OK, E_INVAL, OK, OK, OK, OK]
    want = [s for s in per_item for _ in range(e)]
    want[9 * e + 1] = E_CAP
    want[11 * e + e - 1] = E_NOCODE
    b = Planes(ghf, ctx, torch, Inputs(torch, datas), codes_to_device(torch, codes), e, max_item, caps=caps).run()  # ends with ctx.sync(): OK
    try:
        assert b.h_status.tolist() == want
        for j in range(b.slots):
            if want[j] == OK:
                assert np.array_equal(b.body(j), orc_body(datas[j // e][j % e :: e], codes[j % e])), j
                assert np.all(b.slot(j)[caps[j] :] == GUARD), j
            else:
                assert int(b.h_bytes[j]) == 0 and np.all(b.slot(j) == GUARD), j  # a refused slot writes nothing at all
    finally:
        b.free()
    # one incomplete code: GHF_E_FORMAT on that plane's slots only, nothing written there
    datas = good[:4]
    hists = orc_hists(datas, e, max_item)
    codes = [orc.build_code(np.ascontiguousarray(hists[p])) for p in range(e)]
    for name, bad in bad_codes(ghf.Code.from_buffer_copy(bytes(codes[e - 1])), ghf.Code.from_buffer_copy)[:2]:
        b = Planes(ghf, ctx, torch, Inputs(torch, datas), codes_to_device(torch, codes[: e - 1] + [bad]), e, max_item).run()
        try:
            assert b.h_status.tolist() == ([OK] * (e - 1) + [E_FORMAT]) * len(datas), name
            for j in range(b.slots):
                if j % e == e - 1:
                    assert int(b.h_bytes[j]) == 0 and np.all(b.slot(j) == GUARD), (name, j)
                else:
                    assert np.array_equal(b.body(j), orc_body(datas[j // e][j % e :: e], codes[j % e])), (name, j)
        finally:
            b.free()


# ------------------------------------------------------------------------------ 6. per-item failures, decode
@pytest.mark.parametrize("e", ES)
def test_decode_failures_are_per_item(env, e):
    ghf, ctx, torch = env
    datas = [dg.make(["zipf", "text"][k % 2], n * e, seed=5200 + k) for k, n in enumerate([700, 3000, 1500, 3000, 900, 2000])]
    w = World(env, datas, e, 3000 * e)
    b = w.b
    try:
        assert np.all(b.h_status == OK)
        n_elems = [d.size // e for d in datas]
        stream_bytes = [int(x) for x in b.h_bytes]
        j = 1 * e + (e - 1)  # the last plane of item 1: without the byte of the end mark's last bit
        total_bits = int(np.asarray(list(w.codes[e - 1].length))[w.planes[1][e - 1]].sum()) + w.codes[e - 1].length[256]
        assert stream_bytes[j] == -(-total_bits // 8)
        stream_bytes[j] = (total_bits - 1) // 8
        caps = [3000 * e] * len(datas)
        caps[4] = datas[4].size - 1
        for live in (True, False):
            ne = list(n_elems)
            if live:
                ne[2] = 0
            status, out_bytes, outs, guards = decode(b, live, n_elems=ne, stream_bytes=stream_bytes, caps=caps)
            want = [OK, E_CORRUPT, E_EMPTY if live else OK, OK, E_CAP, OK]
            assert status.tolist() == want, live
            for i, d in enumerate(datas):
                if want[i] == OK:
                    assert int(out_bytes[i]) == d.size and np.array_equal(outs[i][: d.size], d), (live, i)
                else:
                    assert int(out_bytes[i]) == 0, (live, i)
                assert np.all(guards[i][0] == GUARD), (live, i)
                back = guards[i][1] if want[i] != E_CAP else np.concatenate((outs[i], guards[i][1]))[caps[i] :]
                assert np.all(back == GUARD), (live, i)  # nothing at or beyond the cap
        # the bodies decoder: a plane body taken from an item of another length
        h = b.h_out.copy()
        sb = [int(x) for x in b.h_bytes]
        src, dst = 0 * e + 0, 5 * e + 0
        h[dst * b.stride : (dst + 1) * b.stride] = h[src * b.stride : (src + 1) * b.stride]
        sb[dst] = sb[src]
        status, out_bytes, outs, guards = decode(b, False, stream_bytes=sb, d_stream=torch.from_numpy(h).cuda())
        assert status.tolist() == [OK] * 5 + [E_CORRUPT] and int(out_bytes[5]) == 0
        assert all(np.all(g[0] == GUARD) and np.all(g[1] == GUARD) for g in guards)
        # one incomplete code: GHF_E_FORMAT on every item, nothing written
        bad = bad_codes(ghf.Code.from_buffer_copy(bytes(w.codes[e - 1])), ghf.Code.from_buffer_copy)[1][1]
        d_bad = codes_to_device(torch, list(w.codes[: e - 1]) + [bad])
        for live in (True, False):
            status, out_bytes, outs, guards = decode(b, live, d_codes=d_bad)
            assert status.tolist() == [E_FORMAT] * b.count and np.all(out_bytes == 0), live
            for i in range(b.count):
                assert np.all(outs[i] == GUARD) and np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (live, i)
    finally:
        b.free()


# ------------------------------------------------------------------------------ 7. the size claim
def test_planes_store_less_than_one_flat_code(env):
    """64 items of 2048 standard-normal bf16 values: the bodies under two plane codes are strictly smaller than under one
    flat GHF_HIST_COVER_ALL code.  Both sides are the oracle's; the GPU's bodies equal the planes side."""
    ghf, ctx, torch = env
    rng = np.random.default_rng(7)
    datas = [normal_elems(rng, 2048, 2) for _ in range(64)]
    flat_hist = np.zeros(257, dtype=np.int64)
    for d in datas:
        flat_hist[:256] += orc.histogram(d)[:256]
    flat_hist[flat_hist == 0] = 1
    flat_hist[256] = 1
    flat_code = orc.build_code(flat_hist)
    flat = sum(orc_body(d, flat_code).size for d in datas)
    w = World(env, datas, 2, 4096, cover=True)
    try:
        _check_bodies(w)  # the GPU's bodies are the oracle's
        planes = sum(x.size for x in w.bodies)
        print("flat %d bytes, planes %d bytes, ratio %.4f" % (flat, planes, planes / flat))
        assert planes < flat
        assert (flat, planes) == (FLAT_BYTES, PLANES_BYTES)  # the recorded numbers
    finally:
        w.b.free()


# ------------------------------------------------------------------------------ 8. call-level errors
def test_call_level_argument_errors(env):
    ghf, ctx, torch = env
    L = ghf.lib()
    w = world(env, "edge", 4)
    inp = w.inp
    b = Planes(ghf, ctx, torch, inp, w.d_codes, 4, w.max_item)
    d_hists = torch.full((4, 257), 7, dtype=torch.int64).cuda()
    codes = w.d_codes.data_ptr()
    try:
        P = lambda t: None if t is None else t.data_ptr()
        hist = lambda ptrs=inp.in_ptrs, mx=w.max_item, count=b.count, e=4, flags=0, out=d_hists: L.ghf_histogram_batch_planes(
            ctx.h, P(ptrs), P(inp.in_bytes), mx, count, e, flags, P(out))
        comp = lambda ptrs=inp.in_ptrs, mx=w.max_item, count=b.count, e=4, cd=codes, outp=b.out_ptrs, bidx=b.bidx, st=b.status: \
            L.ghf_compress_batch_planes_shared(ctx.h, P(ptrs), P(inp.in_bytes), mx, count, e, cd, P(outp), P(b.out_caps), P(b.out_bytes),
                                               None if bidx is None else C.byref(bidx), P(st))
        dec = lambda sp=b.out_ptrs, cd=codes, bidx=b.bidx, count=b.count, e=4, st=b.status: \
            L.ghf_decode_batch_planes_shared(ctx.h, P(sp), P(b.out_bytes), cd, None if bidx is None else C.byref(bidx), P(inp.in_bytes),
                                             count, e, P(b.out_ptrs), P(b.out_caps), P(b.out_bytes), P(st))
        bod = lambda sp=b.out_ptrs, cd=codes, count=b.count, e=4, st=b.status: \
            L.ghf_decode_bodies_batch_planes_shared(ctx.h, P(sp), P(b.out_bytes), cd, count, e, P(b.out_ptrs), P(b.out_caps),
                                                    P(b.out_bytes), P(st))
        bld = lambda n=4, h=d_hists, cd=codes, flags=0: L.ghf_build_codes(ctx.h, P(h), n, cd, flags)
        assert hist(count=0) == OK and comp(count=0) == OK and dec(count=0) == OK and bod(count=0) == OK  # queues nothing
        for e in (0, 1, 3, 6, 16):
            assert hist(e=e) == E_INVAL and comp(e=e) == E_INVAL and dec(e=e) == E_INVAL and bod(e=e) == E_INVAL, e
        assert hist(mx=w.max_item + 2) == E_INVAL and comp(mx=w.max_item + 2) == E_INVAL  # not a multiple of 4
        assert hist(mx=0) == E_INVAL and comp(mx=0) == E_INVAL and hist(mx=(1 << 20) + 4) == E_INVAL and comp(mx=(1 << 20) + 4) == E_INVAL
        assert hist(ptrs=None) == E_INVAL and hist(out=None) == E_INVAL and hist(flags=2) == E_INVAL
        assert comp(ptrs=None) == E_INVAL and comp(outp=None) == E_INVAL and comp(st=None) == E_INVAL
        assert dec(sp=None) == E_INVAL and dec(st=None) == E_INVAL and dec(bidx=None) == E_INVAL
        assert bod(sp=None) == E_INVAL and bod(st=None) == E_INVAL
        for f in (comp, dec, bod):
            assert f(cd=None) == E_INVAL and f(cd=codes + 8) == E_INVAL
        assert bld(n=0) == E_INVAL and bld(n=9) == E_INVAL and bld(h=None) == E_INVAL and bld(cd=None) == E_INVAL and bld(flags=4) == E_INVAL
        few = ctx.batch_index_alloc(b.slots - 1, w.max_item // 4)
        narrow = ctx.batch_index_alloc(b.slots, w.max_item // 4 - 1)
        assert comp(bidx=few) == E_INVAL and comp(bidx=narrow) == E_INVAL and dec(bidx=few) == E_INVAL
        ctx.batch_index_free(few)
        ctx.batch_index_free(narrow)
        ctx.sync()
        assert np.all(d_hists.cpu().numpy() == 7) and np.all(b.status.cpu().numpy() == -1) and np.all(b.d_out.cpu().numpy() == GUARD)
        assert comp(bidx=None) == OK  # the index is optional for compress, and the context is still usable
        ctx.sync()
        assert b.status.cpu().tolist() == [OK] * b.slots
    finally:
        b.free()


# ------------------------------------------------------------------------------ 9. python wrappers
@pytest.mark.parametrize("e", ES)
def test_python_wrappers_round_trip(env, e):
    ghf, ctx, torch = env
    rng = np.random.default_rng(70 + e)
    datas = [normal_elems(rng, 300 + 97 * k, e) for k in range(9)]
    tensors = [torch.from_numpy(d).cuda() for d in datas]
    max_item = max(d.size for d in datas)
    bidx = ctx.batch_index_alloc(len(datas) * e, max_item // e)
    try:
        d_hists = ctx.histogram_batch_planes(tensors, e, flags=ghf.HIST_COVER_ALL)
        d_codes = ctx.build_codes(d_hists)
        r = ctx.compress_batch_planes_shared(tensors, d_codes, e, index=bidx)
        dec = ctx.decode_batch_planes_shared(r["out_ptrs"], r["out_bytes"], d_codes, bidx, r["n_elems"], e)
        sizes = ctx.decode_bodies_batch_planes_shared(r["out_ptrs"], r["out_bytes"], d_codes, e)
        bod = ctx.decode_bodies_batch_planes_shared(r["out_ptrs"], r["out_bytes"], d_codes, e, out=True, caps=sizes["out_bytes"])
        ctx.sync()
        want = orc_hists(datas, e, max_item, cover=True)
        assert np.array_equal(d_hists.cpu().numpy(), want)
        codes = [orc.build_code(np.ascontiguousarray(want[p])) for p in range(e)]
        assert r["status"].cpu().tolist() == [OK] * (9 * e) and dec["status"].cpu().tolist() == [OK] * 9 == bod["status"].cpu().tolist()
        assert sizes["out_bytes"].cpu().tolist() == [d.size for d in datas]
        h, nb = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
        ho, hb = dec["out"].cpu().numpy(), bod["out"].cpu().numpy()
        for i, d in enumerate(datas):
            for p in range(e):
                j = i * e + p
                assert np.array_equal(h[j * r["out_stride"] :][: nb[j]], orc_body(d[p::e], codes[p])), j
            assert np.array_equal(ho[i * dec["out_stride"] :][: d.size], d), i
            assert np.array_equal(hb[i * bod["out_stride"] :][: d.size], d), i
    finally:
        ctx.batch_index_free(bidx)
