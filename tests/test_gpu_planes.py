"""GPU: byte planes of typed elements (ghf_planes_split / ghf_planes_merge / ghf_compress_planes / ghf_decode_planes).

Expected values come from numpy slicing (plane p of x is x[p::E]) and from the oracle (oracle.compress / build_code /
decompress) alone; where the compiled reference is present its own decoder reads one plane image per element width."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import pkgload
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

E_INVAL, E_EMPTY, E_CAP, E_CORRUPT = 1, 3, 5, 7
GUARD = 0xA5
WIDTHS = (2, 4, 8)
# ghf_internal.h: planes_tile_elems(E) = the elements one wave moves at a time (2048 at E = 2, else 1024), and kPlanesGroups =
# 4096 one-wave workgroups in one resident round.  G * T + 7 gives every workgroup one whole tile and a ragged end; one tile
# more makes the slabs two tiles long, so a workgroup's loop goes round a second time.
T = {2: 2048, 4: 1024, 8: 1024}
G = 256 * 16
COMPRESS_N = (1, 64, 4097, 65536 + 3)


def split_sizes(e):
    t = T[e]
    return [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 3 * t + 5, G * t + 7, (G + 1) * t + 7]


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
def uniform():
    """one run of uniform bytes for every split / merge case (the largest is 32 MiB + 8 KiB + 56 bytes, under 64 MiB)"""
    n = max(split_sizes(e)[-1] * e for e in WIDTHS)
    assert n < 64 << 20
    a = dg.uniform_bytes(n, seed=0x504C414E)
    a.setflags(write=False)
    return a


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()  # a copy: the shared inputs stay read-only


def normal_elems(n, e, seed=7):
    """n seeded standard-normal values as bytes: bf16 (the upper half of the fp32 value) / fp32 / fp64"""
    x = np.random.default_rng(seed).standard_normal(n)
    if e == 8:
        return x.view(np.uint8).copy()
    f = x.astype(np.float32)
    if e == 4:
        return f.view(np.uint8).copy()
    return (f.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()


_want = {}


def want_for(e, n, seed=7):
    """(bytes, [oracle image of plane p], [oracle tables of plane p]) -- computed once per case"""
    key = (e, n, seed)
    if key not in _want:
        x = normal_elems(n, e, seed)
        planes = [np.ascontiguousarray(x[p::e]) for p in range(e)]
        _want[key] = (x, [orc.compress(pl) for pl in planes], [orc.build_code(orc.histogram(pl)).as_dict() for pl in planes])
    return _want[key]


# ---------------------------------------------------------------- 1. split and merge are exact and write nothing else
@pytest.mark.parametrize("e", WIDTHS)
def test_split_and_merge_are_exact_between_guard_bytes(env, uniform, e):
    ghf, ctx, torch = env
    for n in split_sizes(e):
        x = uniform[: n * e]
        d_in = to_dev(torch, x)
        stride = ((n + 15) & ~15) + 48  # > n: room for guard bytes behind every plane
        d_planes = torch.full((e * stride + 64,), GUARD, dtype=torch.uint8, device="cuda")
        ctx.planes_split(d_in, e, n_elems=n, d_planes=d_planes, plane_stride=stride)
        d_back = torch.full((n * e + 64,), GUARD, dtype=torch.uint8, device="cuda")
        ctx.planes_merge(d_planes, stride, n, e, d_out=d_back)
        ctx.sync()
        h = d_planes.cpu().numpy()
        body = h[: e * stride].reshape(e, stride)
        for p in range(e):
            assert np.array_equal(body[p, :n], x[p::e]), (n, p)
        assert (body[:, n:] == GUARD).all() and (h[e * stride :] == GUARD).all(), n
        hb = d_back.cpu().numpy()
        assert np.array_equal(hb[: n * e], x), n
        assert (hb[n * e :] == GUARD).all(), n


# ---------------------------------------------------------------- 2. every plane image is the oracle's, byte for byte
def compress_planes(ghf, ctx, torch, x, e, indexes=None):
    n = x.size // e
    r = ctx.compress_planes(to_dev(torch, x), e, n_elems=n, indexes=indexes)
    ctx.sync()  # GHF_OK: raises otherwise
    return r, r["out"].cpu().numpy(), [int(v) for v in r["out_bytes"].cpu().numpy()], r["codes"].cpu().numpy()


def check_against_oracle(ghf, r, h_out, sizes, h_codes, images, tables):
    for p, (img, tab) in enumerate(zip(images, tables)):
        at = p * r["slot_bytes"]
        assert sizes[p] == img.size, (p, sizes[p], img.size)
        assert np.array_equal(h_out[at : at + sizes[p]], img), p
        assert ghf.Code.from_buffer_copy(h_codes[p].tobytes()).as_dict() == tab, p


@pytest.mark.parametrize("n", COMPRESS_N)
@pytest.mark.parametrize("e", WIDTHS)
def test_compress_planes_is_byte_exact_per_plane(env, e, n):
    ghf, ctx, torch = env
    x, images, tables = want_for(e, n)
    r, h_out, sizes, h_codes = compress_planes(ghf, ctx, torch, x, e)
    assert r["slot_bytes"] == ghf.planes_slot_bytes(n)
    check_against_oracle(ghf, r, h_out, sizes, h_codes, images, tables)


def test_planes_of_bf16_are_smaller_than_the_interleaved_stream(env):
    """the ratio claim, on the oracle's numbers: default_rng(7).standard_normal(65536) as bf16"""
    ghf, ctx, torch = env
    n = 65536
    x, images, _ = want_for(2, n)
    assert [im.size for im in images] == [66648, 23084] and orc.compress(x).size == 103009
    r, _, sizes, _ = compress_planes(ghf, ctx, torch, x, 2)
    _, nbytes, _ = ctx.compress(to_dev(torch, x))
    ctx.sync()
    flat = int(nbytes.item())
    print("bf16 planes", sizes, "interleaved", flat)
    assert sum(sizes) == 89732 and flat == 103009
    assert sum(sizes) < flat


# ---------------------------------------------------------------- 3. round trips
@pytest.mark.parametrize("n", COMPRESS_N)
@pytest.mark.parametrize("e", WIDTHS)
def test_round_trip_with_and_without_side_cars(env, e, n):
    ghf, ctx, torch = env
    x, images, _ = want_for(e, n)
    idx = ctx.planes_index_alloc(n, e)
    r, _, sizes, _ = compress_planes(ghf, ctx, torch, x, e, indexes=idx)
    assert sizes == [im.size for im in images]
    slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
    for indexes in (idx, None):
        d_out = torch.full((n * e + 64,), GUARD, dtype=torch.uint8, device="cuda")
        _, nbytes = ctx.decode_planes(slots, sizes, r["codes"], n, e, indexes=indexes, d_out=d_out, cap=n * e)
        ctx.sync()
        h = d_out.cpu().numpy()
        assert int(nbytes.item()) == n * e
        assert np.array_equal(h[: n * e], x), "indexed" if indexes is not None else "without side-car"
        assert (h[n * e :] == GUARD).all()
    ctx.planes_index_free(idx)


@pytest.mark.parametrize("e", WIDTHS)
def test_each_plane_is_an_ordinary_stream(env, e, tmp_path):
    ghf, ctx, torch = env
    n = 4097
    x, images, _ = want_for(e, n)
    idx = ctx.planes_index_alloc(n, e)
    r, h_out, sizes, _ = compress_planes(ghf, ctx, torch, x, e, indexes=idx)
    for p in range(e):
        at = p * r["slot_bytes"]
        image = h_out[at : at + sizes[p]].copy()  # out of its slot
        want = x[p::e]
        assert np.array_equal(orc.decompress(image, cap=n + 8), want), p
        d_img = to_dev(torch, image)
        back, nb = ctx.decode(d_img, image.size, r["codes"][p], idx[p])  # with the tables and side-car of the call
        ctx.sync()
        assert int(nb.item()) == n and np.array_equal(back[:n].cpu().numpy(), want), p
        code, _ = ghf.parse_header(image)  # with nothing but its own bytes
        back, nb = ctx.decode(d_img, image.size, ctx.code_to_device(code), None, cap=n + 64)
        ctx.sync()
        assert int(nb.item()) == n and np.array_equal(back[:n].cpu().numpy(), want), p
    if orc.have_ref():  # the reference's own decoder on the high plane
        at = (e - 1) * r["slot_bytes"]
        h_out[at : at + sizes[e - 1]].tofile(str(tmp_path / "p.crs2"))
        orc.ref_run(["d", str(tmp_path / "p.crs2"), str(tmp_path / "p.de")])
        assert np.array_equal(np.fromfile(str(tmp_path / "p.de"), dtype=np.uint8), x[e - 1 :: e])
    ctx.planes_index_free(idx)


# ---------------------------------------------------------------- 4. the workspace is reused: nothing of the last call sticks
def test_second_call_on_the_same_context_sees_the_new_bytes(env):
    """Guards the IMAGES of a second call on the same workspace addresses, whatever keeps them right.  It does not single
    out the two forget() calls of ghf_compress_planes: ghf_compress re-runs the histogram, which overwrites the one-entry
    cache before the plan consults it, so the images would be right without them; the forgetting is defence for callers
    that follow with staged calls on an address inside the workspace."""
    ghf, ctx, torch = env
    e, n = 4, 4097
    for seed in (7, 8):  # same n_elems, same workspace addresses, other bytes
        x, images, tables = want_for(e, n, seed)
        r, h_out, sizes, h_codes = compress_planes(ghf, ctx, torch, x, e)
        check_against_oracle(ghf, r, h_out, sizes, h_codes, images, tables)
    assert not np.array_equal(want_for(e, n, 7)[1][e - 1], want_for(e, n, 8)[1][e - 1])


# ---------------------------------------------------------------- 5. refusals; the context stays usable after each
def good_round_trip(ghf, ctx, torch):
    assert ctx.L.ghf_clear_status(ctx.h) == 0
    e, n = 2, 4097
    x, images, _ = want_for(e, n)
    idx = ctx.planes_index_alloc(n, e)
    r, _, sizes, _ = compress_planes(ghf, ctx, torch, x, e, indexes=idx)
    slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
    back, nb = ctx.decode_planes(slots, sizes, r["codes"], n, e, indexes=idx)
    ctx.sync()
    assert int(nb.item()) == n * e and np.array_equal(back[: n * e].cpu().numpy(), x)
    ctx.planes_index_free(idx)


def refused(ghf, status, fn, *args, **kw):
    with pytest.raises(ghf.GhfError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, ei.value


def test_a_bad_elem_bytes_is_refused_by_a_live_context(env):
    """every width but 2, 4 and 8 is GHF_E_INVAL on all four device calls, with a real context and otherwise good
    arguments: nothing is written, and the context goes on working"""
    ghf, ctx, torch = env
    L = ctx.L
    e, n = 4, 4097
    x, _, _ = want_for(e, n)
    idx = ctx.planes_index_alloc(n, e)
    d_in = to_dev(torch, x)
    r, _, sizes, _ = compress_planes(ghf, ctx, torch, x, e, indexes=idx)
    slot, stride = r["slot_bytes"], (n + 255) & ~255
    ptrs = (C.c_void_p * 16)(*[r["out"].data_ptr() + (p % e) * slot for p in range(16)])
    szs = (C.c_size_t * 16)(*[sizes[p % e] for p in range(16)])
    codes16 = r["codes"].repeat(4, 1).contiguous()
    d_good_planes, _ = ctx.planes_split(d_in, e, n_elems=n)
    big = 16 * max(stride, slot) + 64
    for bad in (0, 1, 3, 16):
        g_planes = torch.full((big,), GUARD, dtype=torch.uint8, device="cuda")
        g_out = torch.full((big,), GUARD, dtype=torch.uint8, device="cuda")
        g_bytes = torch.full((16,), -1, dtype=torch.int64, device="cuda")
        assert L.ghf_planes_split(ctx.h, d_in.data_ptr(), n, bad, g_planes.data_ptr(), stride) == E_INVAL, bad
        assert L.ghf_planes_merge(ctx.h, d_good_planes.data_ptr(), stride, n, bad, g_out.data_ptr()) == E_INVAL, bad
        assert L.ghf_compress_planes(ctx.h, d_in.data_ptr(), n, bad, g_out.data_ptr(), slot, g_bytes.data_ptr(), None, None) == E_INVAL, bad
        assert L.ghf_compress_planes(ctx.h, d_in.data_ptr(), n, bad, g_out.data_ptr(), slot, g_bytes.data_ptr(),
                                     codes16.data_ptr(), idx) == E_INVAL, bad
        for indexes in (idx, None):
            assert L.ghf_decode_planes(ctx.h, ptrs, szs, codes16.data_ptr(), indexes, n, bad, g_out.data_ptr(), big,
                                       g_bytes.data_ptr()) == E_INVAL, bad
        torch.cuda.synchronize()
        assert bool((g_planes == GUARD).all().item()) and bool((g_out == GUARD).all().item()), bad
        assert bool((g_bytes == -1).all().item()), bad
        assert ctx.L.ghf_sync(ctx.h) == 0  # nothing latched either
        good_round_trip(ghf, ctx, torch)
    ctx.planes_index_free(idx)


def test_refusals_leave_the_output_alone_and_the_context_usable(env):
    ghf, ctx, torch = env
    e, n = 4, 4097
    x, images, _ = want_for(e, n)
    idx = ctx.planes_index_alloc(n, e)
    d_in = to_dev(torch, x)
    r, _, sizes, _ = compress_planes(ghf, ctx, torch, x, e, indexes=idx)
    slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]

    def guarded():
        return torch.full((n * e + 64,), GUARD, dtype=torch.uint8, device="cuda")

    def untouched(d_out):
        ctx.torch.cuda.synchronize()
        return bool((d_out == GUARD).all().item())

    # an index that covers another number of symbols: GHF_E_INVAL, nothing queued
    bad = (ghf.Index * e)()
    for p in range(e):
        C.memmove(C.byref(bad[p]), C.byref(idx[p]), C.sizeof(ghf.Index))
    bad[1].n_symbols = n - 1
    d_out = guarded()
    refused(ghf, E_INVAL, ctx.decode_planes, slots, sizes, r["codes"], n, e, indexes=bad, d_out=d_out, cap=n * e)
    assert untouched(d_out)
    good_round_trip(ghf, ctx, torch)
    # cap one byte short
    d_out = guarded()
    refused(ghf, E_CAP, ctx.decode_planes, slots, sizes, r["codes"], n, e, indexes=idx, d_out=d_out, cap=n * e - 1)
    assert untouched(d_out)
    good_round_trip(ghf, ctx, torch)
    # slot_bytes 16 short
    refused(ghf, E_CAP, ctx.compress_planes, d_in, e, n_elems=n, slot_bytes=ghf.planes_slot_bytes(n) - 16)
    good_round_trip(ghf, ctx, torch)
    # a misaligned d_in
    d_odd = torch.zeros(n * e + 16, dtype=torch.uint8, device="cuda")[1 : 1 + n * e]
    refused(ghf, E_INVAL, ctx.compress_planes, d_odd, e, n_elems=n)
    refused(ghf, E_INVAL, ctx.planes_split, d_odd, e, n_elems=n)
    good_round_trip(ghf, ctx, torch)
    # no elements
    refused(ghf, E_EMPTY, ctx.compress_planes, d_in, e, n_elems=0)
    refused(ghf, E_EMPTY, ctx.decode_planes, slots, sizes, r["codes"], 0, e, indexes=None, d_out=guarded(), cap=n * e)
    good_round_trip(ghf, ctx, torch)
    # without side-cars, plane 1 is the valid image of a shorter plane: the sizes disagree, GHF_E_CORRUPT, no merge
    short = np.ascontiguousarray(x[1::e][: n - 5])
    s_out, s_nb, s_code = ctx.compress(to_dev(torch, short))
    ctx.sync()
    assert int(s_nb.item()) == orc.compress(short).size
    codes = r["codes"].clone()
    codes[1] = s_code
    slots2, sizes2 = list(slots), list(sizes)
    slots2[1], sizes2[1] = s_out, int(s_nb.item())
    d_out = guarded()
    refused(ghf, E_CORRUPT, ctx.decode_planes, slots2, sizes2, codes, n, e, indexes=None, d_out=d_out, cap=n * e)
    assert untouched(d_out)
    good_round_trip(ghf, ctx, torch)
    ctx.planes_index_free(idx)
