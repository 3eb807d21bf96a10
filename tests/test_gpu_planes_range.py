"""GPU: an element range of byte planes (ghf_planes_merge_range / ghf_decode_planes_range).

The expected bytes of every case are the numpy (or torch) slice x[first * E : (first + count) * E] of the input; no
reference is needed."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import pkgload

pytestmark = pytest.mark.gpu

E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT = 1, 3, 5, 6, 7
GUARD = 0xA5
PAD = 64  # guard bytes in front of and behind d_out
WIDTHS = (2, 4, 8)
# ghf_internal.h: planes_tile_elems(E) and kPlanesGroups, as in tests/test_gpu_planes.py.  G * T + 7 gives every workgroup one
# whole tile and a ragged end, (G + 1) * T + 7 makes the slabs two tiles long.
T = {2: 2048, 4: 1024, 8: 1024}
G = 256 * 16
SKEWS = tuple(range(16))
BASE = 48  # whole vectors in front of the range: first = BASE + skew
N_ELEMS = 3 * 4096 + 1061  # decode cases: a ragged last block, no multiple of 16 or 64
REC = np.dtype([("start", "<u8"), ("run", "<u2", (8,))])  # a record of the seek table, behind its 64-byte header


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    assert pkg.ghf.PLANES_TILE == T and pkg.ghf.PLANES_GROUPS == G
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


@pytest.fixture(scope="module")
def d_uniform(env):
    """one run of uniform bytes on the device for every merge case (the largest is 32 MiB + 8 KiB + a few hundred bytes)"""
    _, _, torch = env
    n = max((BASE + 15 + (G + 1) * T[e] + 7) * e for e in WIDTHS)
    assert n < 64 << 20
    return torch.from_numpy(dg.uniform_bytes(n, seed=0x52414E47)).cuda()


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def normal_elems(n, e, seed=7):
    """n seeded standard-normal values as bytes: bf16 (the upper half of the fp32 value) / fp32 / fp64"""
    x = np.random.default_rng(seed).standard_normal(n)
    if e == 8:
        return x.view(np.uint8).copy()
    f = x.astype(np.float32)
    if e == 4:
        return f.view(np.uint8).copy()
    return (f.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()


def guarded(torch, nbytes):
    return torch.full((PAD + nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda")


def guards_intact(buf, nbytes):
    return bool((buf[:PAD] == GUARD).all().item()) and bool((buf[PAD + nbytes :] == GUARD).all().item())


def untouched(torch, buf):
    torch.cuda.synchronize()
    return bool((buf == GUARD).all().item())


# ---------------------------------------------------------------- 1. the skewed merge
def planes_of(torch, d_x, e, n):
    """the planes of elements [0, n) of d_x, allocated e * plane_stride long with the smallest stride the call takes.  (The
    allocator rounds sizes up, so a read just outside the last plane's window would not fault here: that the kernel stays
    inside [first & ~15, (first + count + 15) & ~15) rests on the argument in its comment, not on this test.)"""
    stride = (n + 15) & ~15
    d_planes = torch.full((e * stride,), GUARD, dtype=torch.uint8, device="cuda")
    d_planes.view(e, stride)[:, :n] = d_x[: n * e].view(n, e).t()
    return d_planes, stride


def check_merge_range(ctx, torch, d_x, e, first, count):
    d_planes, stride = planes_of(torch, d_x, e, first + count)
    assert stride == (first + count + 15) & ~15 and d_planes.numel() == e * stride
    buf = guarded(torch, count * e)
    ctx.planes_merge_range(d_planes, stride, first, count, e, d_out=buf[PAD:])
    ctx.sync()
    assert torch.equal(buf[PAD : PAD + count * e], d_x[first * e : (first + count) * e]), (e, first, count)
    assert guards_intact(buf, count * e), (e, first, count)


@pytest.mark.parametrize("count_of", [lambda t: 1, lambda t: 17, lambda t: t + 1, lambda t: 3 * t + 5],
                         ids=["1", "17", "T+1", "3T+5"])
@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_every_skew(env, d_uniform, e, count_of):
    ghf, ctx, torch = env
    for s in SKEWS:
        check_merge_range(ctx, torch, d_uniform, e, BASE + s, count_of(T[e]))


@pytest.mark.parametrize("tiles", [G, G + 1], ids=["one_tile_per_group", "two_tiles_per_group"])
@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_full_grid(env, d_uniform, e, tiles):
    ghf, ctx, torch = env
    for s in (0, 5, 15):
        check_merge_range(ctx, torch, d_uniform, e, BASE + s, tiles * T[e] + 7)


@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_at_skew_0_is_planes_merge(env, d_uniform, e):
    ghf, ctx, torch = env
    n = 3 * T[e] + 5
    d_planes, stride = planes_of(torch, d_uniform, e, n)
    a = ctx.planes_merge(d_planes, stride, n, e)
    b = ctx.planes_merge_range(d_planes, stride, 0, n, e)
    ctx.sync()
    assert torch.equal(a[: n * e], b[: n * e]) and torch.equal(a[: n * e], d_uniform[: n * e])


def test_merge_range_refusals(env, d_uniform):
    ghf, ctx, torch = env
    L = ctx.L
    e, first, count = 4, 53, 1000
    d_planes, stride = planes_of(torch, d_uniform, e, first + count)
    buf = guarded(torch, count * e)
    pl, out = d_planes.data_ptr(), buf.data_ptr() + PAD
    top = (1 << 64) - 1
    cases = [
        (E_INVAL, (None, stride, first, count, e, out)),
        (E_INVAL, (pl, stride, first, count, e, None)),
        (E_INVAL, (pl, stride, first, count, 3, out)),
        (E_INVAL, (pl, stride, first, count, 16, out)),
        (E_INVAL, (pl + 4, stride, first, count, e, out)),
        (E_INVAL, (pl, stride + 8, first, count, e, out)),
        (E_INVAL, (pl, stride, first, count, e, out + 1)),
        (E_INVAL, (pl, top & ~15, top - 7, 16, e, out)),      # first + count wraps
        (E_INVAL, (pl, top & ~15, 0, 1 << 62, e, out)),       # count * E wraps
        (E_EMPTY, (pl, stride, first, 0, e, out)),
        (E_CAP, (pl, stride - 16, first, count, e, out)),
        (E_CAP, (pl, stride, first + 16, count, e, out)),
    ]
    for want, args in cases:
        assert L.ghf_planes_merge_range(ctx.h, *args) == want, args
        assert untouched(torch, buf), args
        assert L.ghf_sync(ctx.h) == 0
    check_merge_range(ctx, torch, d_uniform, e, first, count)


# ---------------------------------------------------------------- 2. the composed call
DATA = {"bf16": (2, "normal"), "fp32": (4, "normal"), "fp64": (8, "normal"), "uniform2": (2, "uniform")}
# (the issue's names for these: no head / head only / ... -- the call decodes every plane from the start of the block that
# holds `first`, so no k_decode_head runs; the cases stay for the starts and ends they put inside and on the edges of blocks)
RANGES = [(0, N_ELEMS), (0, 1), (N_ELEMS - 1, 1), (4096, 100), (4100, 50), (100, 3996), (N_ELEMS - 3000, 3000)] + \
         [(1000 + s, 2 * 2048 + 77) for s in SKEWS]


class World:
    """one tensor compressed once with ghf_compress_planes and side-cars, its seek tables through host bytes and back"""

    def __init__(self, ghf, ctx, torch, name):
        self.e, kind = DATA[name]
        e, n = self.e, N_ELEMS
        self.x = normal_elems(n, e) if kind == "normal" else dg.uniform_bytes(n * e, seed=0x55)
        self.d_x = to_dev(torch, self.x)
        self.idx = ctx.planes_index_alloc(n, e)
        r = ctx.compress_planes(self.d_x, e, n_elems=n, indexes=self.idx)
        ctx.sync()
        self.codes = r["codes"]
        self.sizes = [int(v) for v in r["out_bytes"].cpu().numpy()]
        self.slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
        self.tables = []  # host bytes
        for p in range(e):
            d_table = ctx.seek_pack(self.idx[p])
            ctx.sync()
            self.tables.append(d_table.cpu().numpy().copy())
        self.infos = [ghf.seek_parse(t) for t in self.tables]
        assert all(i.n_symbols == n and i.n_blocks == 4 for i in self.infos)
        self.d_tables = [to_dev(torch, t) for t in self.tables]

    def source(self, which):
        return {"indexes": self.idx} if which == "indexes" else {"infos": self.infos, "d_tables": self.d_tables}

    def want(self, first, count):
        return self.x[first * self.e : (first + count) * self.e]


_worlds = {}


@pytest.fixture(scope="module")
def world(env):
    ghf, ctx, torch = env

    def get(name):
        if name not in _worlds:
            _worlds[name] = World(ghf, ctx, torch, name)
        return _worlds[name]

    yield get
    for w in _worlds.values():
        ctx.planes_index_free(w.idx)
    _worlds.clear()


def decode_range_checked(ctx, torch, w, first, count, **source):
    buf = guarded(torch, count * w.e)
    ctx.decode_planes_range(w.slots, w.sizes, w.codes, w.e, first, count, d_out=buf[PAD:], cap=count * w.e, **source)
    ctx.sync()
    h = buf.cpu().numpy()
    assert np.array_equal(h[PAD : PAD + count * w.e], w.want(first, count)), (first, count, list(source))
    assert (h[:PAD] == GUARD).all() and (h[PAD + count * w.e :] == GUARD).all(), (first, count, list(source))
    return h[PAD : PAD + count * w.e]


@pytest.mark.parametrize("which", ["indexes", "tables"])
@pytest.mark.parametrize("name", list(DATA))
def test_decode_planes_range(env, world, name, which):
    ghf, ctx, torch = env
    w = world(name)
    for first, count in RANGES:
        got = decode_range_checked(ctx, torch, w, first, count, **w.source(which))
        if (first, count) == (0, N_ELEMS):  # the whole range is ghf_decode_planes
            whole, nbytes = ctx.decode_planes(w.slots, w.sizes, w.codes, N_ELEMS, w.e, indexes=w.idx)
            ctx.sync()
            assert int(nbytes.item()) == N_ELEMS * w.e
            assert np.array_equal(whole[: N_ELEMS * w.e].cpu().numpy(), got)


def test_decode_planes_range_refusals(env, world):
    ghf, ctx, torch = env
    L = ctx.L
    w = world("fp32")
    e, n = w.e, N_ELEMS
    first, count = 1005, 5000
    buf = guarded(torch, count * e)
    out, cap = buf.data_ptr() + PAD, count * e
    vp, sz = C.c_void_p, C.c_size_t
    ptrs = (vp * e)(*[s.data_ptr() for s in w.slots])
    sizes = (sz * e)(*w.sizes)
    codes = w.codes.data_ptr()
    infos = (ghf.SeekInfo * e)(*w.infos)
    tptrs = (vp * e)(*[t.data_ptr() for t in w.d_tables])
    tbytes = (sz * e)(*[t.size for t in w.tables])

    def copy_of(arr, typ):
        c = (typ * e)()
        C.memmove(c, arr, C.sizeof(c))
        return c

    odd_ptrs = copy_of(ptrs, vp)
    odd_ptrs[1] = ptrs[1] + 8
    null_ptrs = copy_of(ptrs, vp)
    null_ptrs[e - 1] = None
    odd_tptrs = copy_of(tptrs, vp)
    odd_tptrs[2] = tptrs[2] + 8
    null_tptrs = copy_of(tptrs, vp)
    null_tptrs[0] = None
    bad_idx = copy_of(w.idx, ghf.Index)  # malformed: the counts are not those of n_symbols
    bad_idx[1].n_segs += 1
    short_idx = copy_of(w.idx, ghf.Index)  # a well-formed side-car of another size
    short_idx[e - 1].n_symbols = 4096
    short_idx[e - 1].n_segs = 64
    short_idx[e - 1].n_chunks = 1
    short_infos = copy_of(infos, ghf.SeekInfo)
    short_infos[e - 1].n_symbols = 4096
    short_infos[e - 1].n_blocks = 1
    huge_infos = copy_of(infos, ghf.SeekInfo)  # all agree on 2^62 elements: count * E wraps before the tables are looked at
    for p in range(e):
        huge_infos[p].n_symbols = 1 << 62
    bad_tbytes = copy_of(tbytes, sz)  # the LAST plane's table is 24 bytes short
    bad_tbytes[e - 1] -= 24
    by_idx = (w.idx, None, None, None)
    by_tab = (None, infos, tptrs, tbytes)
    cases = [
        (E_INVAL, (None, sizes, codes) + by_idx + (e, first, count, out, cap)),
        (E_INVAL, (ptrs, None, codes) + by_idx + (e, first, count, out, cap)),
        (E_INVAL, (ptrs, sizes, None) + by_idx + (e, first, count, out, cap)),
        (E_INVAL, (ptrs, sizes, codes) + by_idx + (e, first, count, None, cap)),
        (E_INVAL, (ptrs, sizes, codes) + by_idx + (3, first, count, out, cap)),
        (E_INVAL, (ptrs, sizes, codes) + by_tab + (16, first, count, out, cap)),
        (E_INVAL, (odd_ptrs, sizes, codes) + by_idx + (e, first, count, out, cap)),
        (E_INVAL, (null_ptrs, sizes, codes) + by_tab + (e, first, count, out, cap)),
        (E_INVAL, (ptrs, sizes, codes, None, infos, odd_tptrs, tbytes, e, first, count, out, cap)),
        (E_INVAL, (ptrs, sizes, codes, None, infos, null_tptrs, tbytes, e, first, count, out, cap)),
        (E_INVAL, (ptrs, sizes, codes) + by_idx + (e, first, count, out + 4, cap)),
        (E_INVAL, (ptrs, sizes, codes, w.idx, infos, tptrs, tbytes, e, first, count, out, cap)),  # both sources
        (E_INVAL, (ptrs, sizes, codes, None, None, None, None, e, first, count, out, cap)),       # neither
        (E_INVAL, (ptrs, sizes, codes, None, infos, None, tbytes, e, first, count, out, cap)),    # half a source
        (E_INVAL, (ptrs, sizes, codes, bad_idx, None, None, None, e, first, count, out, cap)),
        (E_INVAL, (ptrs, sizes, codes, short_idx, None, None, None, e, 0, 100, out, cap)),
        (E_INVAL, (ptrs, sizes, codes, None, short_infos, tptrs, tbytes, e, 0, 100, out, cap)),
        (E_INVAL, (ptrs, sizes, codes) + by_idx + (e, n - 10, 11, out, cap)),
        (E_INVAL, (ptrs, sizes, codes) + by_tab + (e, n + 1, 0, out, cap)),
        (E_INVAL, (ptrs, sizes, codes, None, huge_infos, tptrs, tbytes, e, 0, 1 << 62, out, cap)),
        (E_FORMAT, (ptrs, sizes, codes, None, infos, tptrs, bad_tbytes, e, first, count, out, cap)),
        (E_FORMAT, (ptrs, sizes, codes, None, infos, tptrs, bad_tbytes, e, first, count, out, cap - 1)),  # FORMAT before CAP
        (E_CAP, (ptrs, sizes, codes) + by_idx + (e, first, count, out, cap - 1)),
        (E_CAP, (ptrs, sizes, codes) + by_tab + (e, first, count, out, cap - 1)),
        (0, (ptrs, sizes, codes) + by_idx + (e, first, 0, out, cap)),  # count == 0: GHF_OK, nothing queued
        (0, (ptrs, sizes, codes) + by_tab + (e, n, 0, out, 0)),
    ]
    for i, (want, args) in enumerate(cases):
        assert L.ghf_decode_planes_range(ctx.h, *args) == want, i
        assert untouched(torch, buf), i
        assert L.ghf_sync(ctx.h) == 0, i  # nothing latched
    for which in ("indexes", "tables"):  # the context goes on working
        decode_range_checked(ctx, torch, w, first, count, **w.source(which))


def test_a_damaged_table_is_reported_and_nothing_reaches_the_output(env, world):
    """one run_bits of the LAST plane's table: the planes in front of it decode, the merge stores nothing.  A handled error
    path, as in tests/test_gpu_seek.py: every start bit is checked against the stream before anything is read there."""
    ghf, ctx, torch = env
    w = world("fp32")
    e = w.e

    def tables_with(block, run):
        t = w.tables[e - 1].copy()
        t[64:].view(REC)["run"][block, run] += 1
        return w.d_tables[: e - 1] + [to_dev(torch, t)]

    # damage in block 1, ranges that cover it: one from its middle, one from its start (the call decodes block 1 from its
    # start either way -- it never enters a block in its middle --, so both expand the damaged record)
    bad = tables_with(1, 3)
    for first, count in ((4096 + 1001, 5000), (4096, 100)):
        buf = guarded(torch, count * e)
        ctx.decode_planes_range(w.slots, w.sizes, w.codes, e, first, count, infos=w.infos, d_tables=bad, d_out=buf[PAD:],
                                cap=count * e)
        assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
        assert untouched(torch, buf)
        assert ctx.L.ghf_clear_status(ctx.h) == 0
        decode_range_checked(ctx, torch, w, first, count, **w.source("tables"))  # the good tables work
    # the same damage in block 0 is never looked at by a range in blocks 2 .. 3
    bad0 = tables_with(0, 3)
    decode_range_checked(ctx, torch, w, 2 * 4096 + 5, 4096 + 500, infos=w.infos, d_tables=bad0)
