"""GPU: byte planes against a base tensor (ghf_histogram_planes_delta / ghf_planes_split_delta / ghf_planes_merge_delta /
ghf_planes_merge_range_delta / ghf_compress_planes_delta / ghf_decode_planes_delta / ghf_decode_planes_range_delta; DESIGN.md
section 19).

Expected values come from numpy (the delta is x ^ b, its plane p is (x ^ b)[p::E]) and from the oracle (oracle.histogram /
build_code / compress / header_bytes / decompress) alone.  The sizes, ranges and geometry are those of the tests of the plain
calls (tests/test_gpu_planes.py, test_gpu_planes_coded.py, test_gpu_planes_range.py), imported from there."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import pkgload
import test_gpu_planes as tp
import test_gpu_planes_coded as tc
import test_gpu_planes_range as tr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT, E_NOCODE = 0, 1, 3, 5, 6, 7, 10
GUARD = 0xA5
GUARD_WORD = tc.GUARD_WORD
PAD = 64  # guard bytes in front of and behind an output; keeps it 16-byte aligned
WIDTHS = (2, 4, 8)
T, G = tp.T, tp.G
COMPRESS_N = (1, 64, 4097, 65536 + 3)
assert COMPRESS_N == tp.COMPRESS_N == tc.COMPRESS_N
N_ELEMS = tr.N_ELEMS
STEP = 1e-3


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    assert pkg.ghf.PLANES_TILE == T and pkg.ghf.PLANES_GROUPS == G
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()  # a copy: the shared inputs stay read-only


@pytest.fixture(scope="module")
def pair():
    """two runs of uniform bytes with different seeds, long enough for every split / merge / histogram case"""
    n = max(max(tp.split_sizes(e)[-1] * e for e in WIDTHS), max((tr.BASE + 15 + (G + 1) * T[e] + 7) * e for e in WIDTHS),
            max(tc.two_round_elems(e) * e for e in WIDTHS))
    assert n < 64 << 20
    x, b = dg.uniform_bytes(n, seed=0x44454C58), dg.uniform_bytes(n, seed=0x44454C42)
    x.setflags(write=False)
    b.setflags(write=False)
    return x, b


@pytest.fixture(scope="module")
def d_pair(env, pair):
    _, _, torch = env
    return to_dev(torch, pair[0]), to_dev(torch, pair[1])


def as_bytes(v, e):
    """float values as bytes: bf16 (the upper half of the fp32 value) / fp32 / fp64"""
    if e == 8:
        return np.ascontiguousarray(v, dtype=np.float64).view(np.uint8).copy()
    f = np.ascontiguousarray(v, dtype=np.float32)
    if e == 4:
        return f.view(np.uint8).copy()
    return (f.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()


_stepped = {}


def stepped(n, e, seed=7):
    """(new, base) as bytes: base = n seeded standard-normal values, new = the same after a step of relative size 1e-3
    (w + 1e-3 * g in the element's own precision; bf16 is cut from the fp32 values) -- computed once per case"""
    key = (n, e, seed)
    if key not in _stepped:
        dt = np.float64 if e == 8 else np.float32
        w = np.random.default_rng(seed).standard_normal(n).astype(dt)
        g = np.random.default_rng(seed + 1).standard_normal(n).astype(dt)
        w2 = (w + dt(STEP) * g).astype(dt)
        new, base = as_bytes(w2, e), as_bytes(w, e)
        new.setflags(write=False)
        base.setflags(write=False)
        _stepped[key] = (new, base)
    return _stepped[key]


def planes_of(a, e):
    return [np.ascontiguousarray(a[p::e]) for p in range(e)]


_want = {}


def want_for(e, n, seed=7):
    """(new, base, delta, [oracle image of plane p of the delta], [oracle tables of plane p]) -- computed once per case"""
    key = (e, n, seed)
    if key not in _want:
        new, base = stepped(n, e, seed)
        delta = new ^ base
        delta.setflags(write=False)
        pl = planes_of(delta, e)
        _want[key] = (new, base, delta, [orc.compress(p) for p in pl], [orc.build_code(orc.histogram(p)).as_dict() for p in pl])
    return _want[key]


def guarded(torch, nbytes):
    return torch.full((PAD + nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda")


def guards_intact(buf, nbytes):
    return bool((buf[:PAD] == GUARD).all().item()) and bool((buf[PAD + nbytes :] == GUARD).all().item())


def untouched(torch, buf):
    torch.cuda.synchronize()
    return bool((buf == GUARD).all().item())


def preloaded(torch, d_base_bytes):
    """a guarded buffer whose payload already holds the base: the d_out of an in-place call"""
    buf = guarded(torch, d_base_bytes.numel())
    buf[PAD : PAD + d_base_bytes.numel()] = d_base_bytes
    return buf


# ---------------------------------------------------------------- 1. split and merge
@pytest.mark.parametrize("e", WIDTHS)
def test_split_delta_and_merge_delta_are_exact_between_guard_bytes(env, pair, d_pair, e):
    ghf, ctx, torch = env
    (x_all, b_all), (d_x_all, d_b_all) = pair, d_pair
    for n in tp.split_sizes(e):
        x, b = x_all[: n * e], b_all[: n * e]
        delta = x ^ b
        d_x, d_b = d_x_all[: n * e], d_b_all[: n * e]
        stride = ((n + 15) & ~15) + 48  # > n: room for guard bytes behind every plane
        d_planes = torch.full((e * stride + 64,), GUARD, dtype=torch.uint8, device="cuda")
        ctx.planes_split_delta(d_x, d_b, e, n_elems=n, d_planes=d_planes, plane_stride=stride)
        back = guarded(torch, n * e)
        ctx.planes_merge_delta(d_planes, stride, d_b, n, e, d_out=back[PAD:])
        inplace = preloaded(torch, d_b)
        ctx.planes_merge_delta(d_planes, stride, inplace[PAD:], n, e, d_out=inplace[PAD:])
        ctx.sync()
        h = d_planes.cpu().numpy()
        body = h[: e * stride].reshape(e, stride)
        for p in range(e):
            assert np.array_equal(body[p, :n], delta[p::e]), (n, p)
        assert (body[:, n:] == GUARD).all() and (h[e * stride :] == GUARD).all(), n
        for what, buf in (("merge", back), ("in place", inplace)):
            assert np.array_equal(buf[PAD : PAD + n * e].cpu().numpy(), x), (what, n)
            assert guards_intact(buf, n * e), (what, n)
        assert torch.equal(d_b, d_b_all[: n * e]) and torch.equal(d_x, d_x_all[: n * e])  # the inputs are only read


# ---------------------------------------------------------------- 2. merge range
def check_merge_range_delta(ctx, torch, d_x, d_b, e, first, count):
    """the planes hold elements [0, first + count) of d_x (the delta); the base of the range is d_b[0 .. count * e), as the
    call wants it: indexed like d_out, whatever `first` is"""
    d_planes, stride = tr.planes_of(torch, d_x, e, first + count)
    base = d_b[: count * e]
    want = d_x[first * e : (first + count) * e] ^ base
    buf = guarded(torch, count * e)
    ctx.planes_merge_range_delta(d_planes, stride, base, first, count, e, d_out=buf[PAD:])
    inplace = preloaded(torch, base)
    ctx.planes_merge_range_delta(d_planes, stride, inplace[PAD:], first, count, e, d_out=inplace[PAD:])
    ctx.sync()
    for what, b in (("range", buf), ("in place", inplace)):
        assert torch.equal(b[PAD : PAD + count * e], want), (what, e, first, count)
        assert guards_intact(b, count * e), (what, e, first, count)


@pytest.mark.parametrize("count_of", [lambda t: 1, lambda t: 17, lambda t: t + 1, lambda t: 3 * t + 5],
                         ids=["1", "17", "T+1", "3T+5"])
@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_delta_every_skew(env, d_pair, e, count_of):
    ghf, ctx, torch = env
    for s in tr.SKEWS:
        check_merge_range_delta(ctx, torch, d_pair[0], d_pair[1], e, tr.BASE + s, count_of(T[e]))


@pytest.mark.parametrize("tiles", [G, G + 1], ids=["one_tile_per_group", "two_tiles_per_group"])
@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_delta_full_grid(env, d_pair, e, tiles):
    ghf, ctx, torch = env
    for s in (0, 5, 15):
        check_merge_range_delta(ctx, torch, d_pair[0], d_pair[1], e, tr.BASE + s, tiles * T[e] + 7)


@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_delta_at_skew_0_is_merge_delta_on_the_shifted_planes(env, d_pair, e):
    ghf, ctx, torch = env
    d_x, d_b = d_pair
    first, n = tr.BASE, 3 * T[e] + 5
    d_planes, stride = tr.planes_of(torch, d_x, e, first + n)
    base = d_b[: n * e]
    a = ctx.planes_merge_delta(d_planes[first:], stride, base, n, e)
    b = ctx.planes_merge_range_delta(d_planes, stride, base, first, n, e)
    ctx.sync()
    assert torch.equal(a[: n * e], b[: n * e]) and torch.equal(a[: n * e], d_x[first * e : (first + n) * e] ^ base)


# ---------------------------------------------------------------- 3. histogram
def guarded_hists(ghf, ctx, torch, d_in, d_base, e, n, flags=0):
    """histogram_planes_delta into the middle of a guarded buffer -> (int64[e, 257] on the host, guards untouched)"""
    buf = torch.full((e * ghf.NSYM + 16,), GUARD_WORD, dtype=torch.int64, device="cuda")
    ctx.histogram_planes_delta(d_in, d_base, e, n_elems=n, flags=flags, out=buf[8 : 8 + e * ghf.NSYM])
    ctx.sync()
    h = buf.cpu().numpy()
    return h[8:-8].reshape(e, ghf.NSYM), bool((h[:8] == GUARD_WORD).all() and (h[-8:] == GUARD_WORD).all())


def check_hists(ghf, ctx, torch, x, b, e, what, d_x=None, d_b=None):
    n = x.size // e
    want = tc.plane_hists(x ^ b, e)
    assert (want[:, 256] == 1).all()
    d_x = to_dev(torch, x) if d_x is None else d_x
    d_b = to_dev(torch, b) if d_b is None else d_b
    got, clean = guarded_hists(ghf, ctx, torch, d_x, d_b, e, n)
    assert clean, (what, n)
    assert np.array_equal(got, want), (what, n, np.argwhere(got != want)[:4])
    got, clean = guarded_hists(ghf, ctx, torch, d_x, d_b, e, n, flags=ghf.HIST_COVER_ALL)
    assert clean, (what, n)
    assert np.array_equal(got, tc.covered(want)), (what, n)


@pytest.mark.parametrize("e", WIDTHS)
def test_delta_plane_histograms_are_exact_between_guard_words(env, pair, d_pair, e):
    """uniform against uniform, standard-normal values against their 1e-3 step, and a tensor against itself (every byte of
    the delta is 0: every lane of every wave stands on one bin) at every size, the one included at which every workgroup
    takes two tiles and one of them the ragged end"""
    ghf, ctx, torch = env
    (x_all, b_all), (d_x_all, d_b_all) = pair, d_pair
    for n in tc.HIST_N + (tc.two_round_elems(e),):
        check_hists(ghf, ctx, torch, x_all[: n * e], b_all[: n * e], e, "uniform", d_x_all[: n * e], d_b_all[: n * e])
        new, base = stepped(n, e)
        check_hists(ghf, ctx, torch, new, base, e, "normal step")
        check_hists(ghf, ctx, torch, x_all[: n * e], x_all[: n * e], e, "x == b", d_x_all[: n * e], d_x_all[: n * e].clone())


def test_a_delta_histogram_past_the_u32_flush_is_exact(env):
    """E = 2, one tile short of (FLUSH + 1) tiles for every workgroup plus a ragged end, just under 64 MiB for each of the two
    buffers: every workgroup but the last moves its u32 counters into its u64 sums after FLUSH tiles and then counts one
    tile more.  The low bytes of element k are k % 5 and k % 3, the high bytes are constant: the delta's low byte has the
    period 15 and the expected counts are arithmetic."""
    ghf, ctx, torch = env
    e = 2
    g, tile, flush = tc.hist_geom()
    n_bytes = (g * (flush + 1) - 1) * tile + 3 * 16 + e
    assert n_bytes <= 64 << 20 and (n_bytes // tile) // g == flush
    n = n_bytes // e
    k = torch.arange(n, dtype=torch.int32, device="cuda")
    d_in = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    d_base = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    d_in[0::2] = (k % 5).to(torch.uint8)
    d_in[1::2] = 0xEE
    d_base[0::2] = (k % 3).to(torch.uint8)
    d_base[1::2] = 0x0F
    got, clean = guarded_hists(ghf, ctx, torch, d_in, d_base, e, n)
    want = np.zeros((e, ghf.NSYM), dtype=np.int64)
    for r in range(15):
        want[0, (r % 5) ^ (r % 3)] += (n - r + 14) // 15  # the k in [0, n) with k % 15 == r
    want[1, 0xEE ^ 0x0F] = n
    want[:, 256] = 1
    assert want[0, :256].sum() == n
    assert clean and np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---------------------------------------------------------------- 4. compress
def fetch(r):
    return r["out"].cpu().numpy(), [int(v) for v in r["out_bytes"].cpu().numpy()], r["codes"].cpu().numpy()


@pytest.mark.parametrize("n", COMPRESS_N)
@pytest.mark.parametrize("e", WIDTHS)
def test_compress_delta_is_byte_exact_and_equals_compress_planes_coded_of_the_xor(env, e, n):
    ghf, ctx, torch = env
    new, base, delta, images, tables = want_for(e, n)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    idx, idx2 = ctx.planes_index_alloc(n, e), ctx.planes_index_alloc(n, e)
    r = ctx.compress_planes_delta(d_new, d_base, e, n_elems=n, flags=ghf.PLANES_BUILD_CODES, indexes=idx)
    ctx.sync()
    assert r["slot_bytes"] == ghf.planes_slot_bytes(n)
    h_out, sizes, h_codes = fetch(r)
    tc.check_against_oracle(ghf, r, h_out, sizes, h_codes, images, tables)
    assert torch.equal(d_new, to_dev(torch, new)) and torch.equal(d_base, to_dev(torch, base))  # the inputs are only read
    # the same context, a device buffer that holds new ^ base
    d_xor = torch.bitwise_xor(d_new, d_base)
    assert np.array_equal(d_xor.cpu().numpy(), delta)
    r2 = ctx.compress_planes_coded(d_xor, e, n_elems=n, indexes=idx2)
    ctx.sync()
    h_out2, sizes2, h_codes2 = fetch(r2)
    assert sizes2 == sizes and np.array_equal(h_codes2, h_codes)
    for p in range(e):
        at = p * r["slot_bytes"]
        assert np.array_equal(h_out2[at : at + sizes[p]], h_out[at : at + sizes[p]]), p
        for a, b in zip(ctx.index_to_host(idx[p]), ctx.index_to_host(idx2[p])):
            assert np.array_equal(a, b), p
    ctx.planes_index_free(idx)
    ctx.planes_index_free(idx2)


@pytest.mark.parametrize("e", WIDTHS)
def test_codes_trained_on_one_pair_compress_the_delta_of_another(env, e):
    ghf, ctx, torch = env
    n = 65536 + 3
    new, base, delta, _, _ = want_for(e, n)
    new_a, base_a = stepped(n, e, seed=11)
    delta_a = new_a ^ base_a
    assert not np.array_equal(delta, delta_a)
    codes_a = ctx.build_codes(ctx.histogram_planes_delta(to_dev(torch, new_a), to_dev(torch, base_a), e, flags=ghf.HIST_COVER_ALL))
    idx = ctx.planes_index_alloc(n, e)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    r = ctx.compress_planes_delta(d_new, d_base, e, d_codes=codes_a, flags=0, indexes=idx)
    predicted = ctx.planes_image_bytes(ctx.histogram_planes_delta(d_new, d_base, e), codes_a, e)
    ctx.sync()
    h_out, sizes, _ = fetch(r)
    assert [int(v) for v in predicted.cpu().numpy()] == sizes
    for p in range(e):
        code_a = orc.build_code(tc.covered(orc.histogram(np.ascontiguousarray(delta_a[p::e]))))
        header = orc.header_bytes(code_a)
        image = h_out[p * r["slot_bytes"] :][: sizes[p]]
        assert np.array_equal(image[: header.size], header), p
        assert np.array_equal(orc.decompress(image, cap=n + 8), delta[p::e]), p
    slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
    back, nb = ctx.decode_planes_delta(slots, sizes, codes_a, d_base, n, e, indexes=idx)
    ctx.sync()
    assert int(nb.item()) == n * e and np.array_equal(back[: n * e].cpu().numpy(), new)
    ctx.planes_index_free(idx)


def good_call(ghf, ctx, torch):
    assert ctx.L.ghf_clear_status(ctx.h) == 0
    e, n = 2, 4097
    new, base, _, images, tables = want_for(e, n)
    r = ctx.compress_planes_delta(to_dev(torch, new), to_dev(torch, base), e)
    ctx.sync()
    tc.check_against_oracle(ghf, r, *fetch(r), images, tables)


def test_a_delta_byte_without_a_code_and_a_code_that_is_not_complete_are_refused(env):
    ghf, ctx, torch = env
    e, n = 2, 4097
    new_a, base, delta_a, _, _ = want_for(e, n)
    new_b = new_a.copy()
    new_b[2 * 100 + 1] = base[2 * 100 + 1] ^ 0x7F  # a delta that turns seven bits of a high byte: no small step does that
    code_a_hi = orc.build_code(orc.histogram(np.ascontiguousarray(delta_a[1::e])))
    assert code_a_hi.length[0x7F] == 0  # on the CPU: the code of A's delta has nothing for that byte
    d_a, d_b, d_base = to_dev(torch, new_a), to_dev(torch, new_b), to_dev(torch, base)
    slot = ghf.planes_slot_bytes(n)

    def guarded_out():
        return torch.full((e * slot,), GUARD, dtype=torch.uint8, device="cuda")

    # codes trained on A's delta without GHF_HIST_COVER_ALL: B's new high byte has no code
    codes_a = ctx.build_codes(ctx.histogram_planes_delta(d_a, d_base, e))
    d_out = guarded_out()
    ctx.compress_planes_delta(d_b, d_base, e, d_codes=codes_a, flags=0, d_out=d_out)
    tc.latched(ghf, ctx, E_NOCODE)
    assert untouched(torch, d_out)
    good_call(ghf, ctx, torch)
    # one length of plane 0's code made a bit longer: the Kraft sum falls short of 1
    codes_bad = ctx.build_codes(ctx.histogram_planes_delta(d_a, d_base, e, flags=ghf.HIST_COVER_ALL))
    words = codes_bad.view(torch.int32)
    host = ghf.Code.from_buffer_copy(codes_bad[0].cpu().numpy().tobytes())
    sym = next(s for s in range(256) if host.length[s] < host.max_len)
    words[0, sym] += 1
    d_out = guarded_out()
    ctx.compress_planes_delta(d_b, d_base, e, d_codes=codes_bad, flags=0, d_out=d_out)
    tc.latched(ghf, ctx, E_FORMAT)
    assert untouched(torch, d_out)
    good_call(ghf, ctx, torch)


# ---------------------------------------------------------------- 5. round trips
def compressed(ghf, ctx, torch, e, n):
    """the delta of want_for(e, n) compressed with side-cars -> (r, slots, sizes, idx, d_base)"""
    new, base, _, images, _ = want_for(e, n)
    idx = ctx.planes_index_alloc(n, e)
    d_base = to_dev(torch, base)
    r = ctx.compress_planes_delta(to_dev(torch, new), d_base, e, n_elems=n, indexes=idx)
    ctx.sync()
    sizes = [int(v) for v in r["out_bytes"].cpu().numpy()]
    assert sizes == [im.size for im in images]
    slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
    return r, slots, sizes, idx, d_base


def round_trip_checked(ctx, torch, new, d_base, slots, sizes, codes, n, e, indexes, what):
    for inplace in (False, True):
        buf = preloaded(torch, d_base) if inplace else guarded(torch, n * e)
        base = buf[PAD : PAD + n * e] if inplace else d_base
        _, nbytes = ctx.decode_planes_delta(slots, sizes, codes, base, n, e, indexes=indexes, d_out=buf[PAD:], cap=n * e)
        ctx.sync()
        assert int(nbytes.item()) == n * e, (what, inplace)
        assert np.array_equal(buf[PAD : PAD + n * e].cpu().numpy(), new), (what, inplace)
        assert guards_intact(buf, n * e), (what, inplace)


@pytest.mark.parametrize("n", COMPRESS_N)
@pytest.mark.parametrize("e", WIDTHS)
def test_round_trip_with_side_cars_without_them_and_from_files(env, e, n, tmp_path):
    ghf, ctx, torch = env
    new = want_for(e, n)[0]
    r, slots, sizes, idx, d_base = compressed(ghf, ctx, torch, e, n)
    round_trip_checked(ctx, torch, new, d_base, slots, sizes, r["codes"], n, e, idx, "side-cars")
    round_trip_checked(ctx, torch, new, d_base, slots, sizes, r["codes"], n, e, None, "without side-cars")
    # every plane is an ordinary .crs2 file: written, read back, decoded with nothing but its own bytes
    h_out = r["out"].cpu().numpy()
    for p in range(e):
        h_out[p * r["slot_bytes"] :][: sizes[p]].tofile(str(tmp_path / ("plane%d.crs2" % p)))
    images = [np.fromfile(str(tmp_path / ("plane%d.crs2" % p)), dtype=np.uint8) for p in range(e)]
    f_slots = [to_dev(torch, im) for im in images]
    f_codes = torch.stack([ctx.code_to_device(ghf.parse_header(im)[0]) for im in images]).contiguous()
    round_trip_checked(ctx, torch, new, d_base, f_slots, [im.size for im in images], f_codes, n, e, None, "files")
    ctx.planes_index_free(idx)


@pytest.mark.parametrize("e", WIDTHS)
def test_a_lying_side_car_leaves_the_output_alone_and_in_place_the_base(env, e):
    """the last plane's side-car puts the end of segment 63 of block 4 one bit late (the handled error of
    tests/test_gpu_range_variants.py: the decoder's end-to-end check of the segment fires): GHF_E_CORRUPT latches and the
    merge behind it stores nothing"""
    ghf, ctx, torch = env
    n = 65536 + 3
    new, base = want_for(e, n)[:2]
    r, slots, sizes, idx, d_base = compressed(ghf, ctx, torch, e, n)
    chunk, seg = ctx.index_to_host(idx[e - 1])
    seg = seg.copy()
    seg[4 * 64 + 63] += 1
    d_chunk, d_seg = to_dev(torch, chunk.view(np.uint8)), to_dev(torch, seg.view(np.uint8))
    bad = (ghf.Index * e)()
    for p in range(e):
        C.memmove(C.byref(bad[p]), C.byref(idx[p]), C.sizeof(ghf.Index))
    bad[e - 1].d_chunk_bit, bad[e - 1].d_seg_bit = d_chunk.data_ptr(), d_seg.data_ptr()
    buf = guarded(torch, n * e)
    ctx.decode_planes_delta(slots, sizes, r["codes"], d_base, n, e, indexes=bad, d_out=buf[PAD:], cap=n * e)
    assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
    assert untouched(torch, buf)
    assert ctx.L.ghf_clear_status(ctx.h) == 0
    buf = preloaded(torch, d_base)
    ctx.decode_planes_delta(slots, sizes, r["codes"], buf[PAD : PAD + n * e], n, e, indexes=bad, d_out=buf[PAD:], cap=n * e)
    assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
    assert np.array_equal(buf[PAD : PAD + n * e].cpu().numpy(), base) and guards_intact(buf, n * e)
    assert ctx.L.ghf_clear_status(ctx.h) == 0
    round_trip_checked(ctx, torch, new, d_base, slots, sizes, r["codes"], n, e, idx, "the true side-cars")
    ctx.planes_index_free(idx)


# ---------------------------------------------------------------- 6. range decode
DATA = {"bf16": (2, "normal"), "fp32": (4, "normal"), "fp64": (8, "normal"), "uniform2": (2, "uniform")}
assert DATA == tr.DATA
RANGES = tr.RANGES


class World:
    """one tensor compressed once against its base with side-cars, its seek tables through host bytes and back"""

    def __init__(self, ghf, ctx, torch, name):
        self.e, kind = DATA[name]
        e, n = self.e, N_ELEMS
        if kind == "normal":
            self.x, self.b = stepped(n, e)
        else:
            self.x, self.b = dg.uniform_bytes(n * e, seed=0x55), dg.uniform_bytes(n * e, seed=0x56)
        self.d_b = to_dev(torch, self.b)
        self.idx = ctx.planes_index_alloc(n, e)
        r = ctx.compress_planes_delta(to_dev(torch, self.x), self.d_b, e, n_elems=n, indexes=self.idx)
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

    def base(self, first, count):
        """the range's own base elements in a buffer of their own: 16-byte aligned, indexed like d_out"""
        return self.d_b[first * self.e : (first + count) * self.e].clone()


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
    base = w.base(first, count)
    for inplace in (False, True):
        buf = preloaded(torch, base) if inplace else guarded(torch, count * w.e)
        d_base = buf[PAD : PAD + count * w.e] if inplace else base
        ctx.decode_planes_range_delta(w.slots, w.sizes, w.codes, d_base, w.e, first, count, d_out=buf[PAD:], cap=count * w.e, **source)
        ctx.sync()
        h = buf.cpu().numpy()
        assert np.array_equal(h[PAD : PAD + count * w.e], w.want(first, count)), (first, count, inplace, list(source))
        assert (h[:PAD] == GUARD).all() and (h[PAD + count * w.e :] == GUARD).all(), (first, count, inplace, list(source))


@pytest.mark.parametrize("which", ["indexes", "tables"])
@pytest.mark.parametrize("name", list(DATA))
def test_decode_planes_range_delta(env, world, name, which):
    ghf, ctx, torch = env
    w = world(name)
    for first, count in RANGES:
        decode_range_checked(ctx, torch, w, first, count, **w.source(which))
    # count == 0: GHF_OK, nothing queued, nothing written
    buf = guarded(torch, 64)
    ctx.decode_planes_range_delta(w.slots, w.sizes, w.codes, w.d_b, w.e, 1005, 0, d_out=buf[PAD:], cap=64, **w.source(which))
    assert ctx.L.ghf_sync(ctx.h) == OK and untouched(torch, buf)


# ---------------------------------------------------------------- 7. sizes
def test_delta_planes_are_smaller_than_the_planes_of_the_new_tensor(env):
    """the ratio claim, on the oracle's numbers: w = default_rng(7).standard_normal(65536) as fp32, w2 = w + 1e-3 * g with
    g = default_rng(8).standard_normal(65536); bf16 is the upper 16 bits.  The literals are recomputed from the oracle here;
    the GPU's sizes equal them and equal what planes_image_bytes predicts from the delta histograms."""
    ghf, ctx, torch = env
    n = 65536
    w = np.random.default_rng(7).standard_normal(n).astype(np.float32)
    g = np.random.default_rng(8).standard_normal(n).astype(np.float32)
    w2 = (w + np.float32(1e-3) * g).astype(np.float32)
    pinned = {2: ([18507, 9379], [66650, 23094]), 4: (160497, 223097)}
    for e in (2, 4):
        new, base = as_bytes(w2, e), as_bytes(w, e)
        assert np.array_equal(new, stepped(n, e)[0]) and np.array_equal(base, stepped(n, e)[1])  # the recipe of this file
        delta = new ^ base
        d_sizes = [orc.compress(p).size for p in planes_of(delta, e)]
        p_sizes = [orc.compress(p).size for p in planes_of(new, e)]
        print("E = %d: delta planes %s = %d bytes, planes of the new tensor %s = %d bytes, ratio %.2f"
              % (e, d_sizes, sum(d_sizes), p_sizes, sum(p_sizes), sum(d_sizes) / sum(p_sizes)))
        if e == 2:
            assert (d_sizes, p_sizes) == pinned[2]
        else:
            assert (sum(d_sizes), sum(p_sizes)) == pinned[4]
        assert sum(d_sizes) < sum(p_sizes)
        d_new, d_base = to_dev(torch, new), to_dev(torch, base)
        r = ctx.compress_planes_delta(d_new, d_base, e)
        predicted = ctx.planes_image_bytes(ctx.histogram_planes_delta(d_new, d_base, e), r["codes"], e)
        plain = ctx.compress_planes_coded(d_new, e)
        ctx.sync()
        assert [int(v) for v in r["out_bytes"].cpu().numpy()] == d_sizes
        assert [int(v) for v in predicted.cpu().numpy()] == d_sizes
        assert [int(v) for v in plain["out_bytes"].cpu().numpy()] == p_sizes


# ---------------------------------------------------------------- 8. refusals; the context stays usable after each
def test_a_null_or_misaligned_base_and_bad_widths_are_refused_by_a_live_context(env, world):
    """GHF_E_INVAL at once from all seven calls: a null d_base, a d_base off by 8 bytes, and every width but 2, 4 and 8, with a
    real context and otherwise good arguments.  Nothing is written, nothing latches, and the context goes on working."""
    ghf, ctx, torch = env
    L = ctx.L
    w = world("fp32")
    e, n = w.e, N_ELEMS
    first, count = 1005, 5000
    d_in = to_dev(torch, w.x)
    slot, stride = ghf.planes_slot_bytes(n), (n + 255) & ~255
    d_good_planes, _ = ctx.planes_split_delta(d_in, w.d_b, e, n_elems=n)
    ctx.sync()
    big = 16 * max(stride, slot) + 64
    g_planes = torch.full((big,), GUARD, dtype=torch.uint8, device="cuda")
    g_out = torch.full((big,), GUARD, dtype=torch.uint8, device="cuda")
    g_bytes = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    g_hists = torch.full((16 * ghf.NSYM,), GUARD_WORD, dtype=torch.int64, device="cuda")
    vp, sz = C.c_void_p, C.c_size_t
    ptrs = (vp * 16)(*[w.slots[p % e].data_ptr() for p in range(16)])
    sizes = (sz * 16)(*[w.sizes[p % e] for p in range(16)])
    codes16 = w.codes.repeat(4, 1).contiguous()
    idx16 = (ghf.Index * 16)()
    infos = (ghf.SeekInfo * 16)(*[w.infos[p % e] for p in range(16)])
    tptrs = (vp * 16)(*[w.d_tables[p % e].data_ptr() for p in range(16)])
    tbytes = (sz * 16)(*[w.tables[p % e].size for p in range(16)])
    for p in range(16):
        C.memmove(C.byref(idx16[p]), C.byref(w.idx[p % e]), C.sizeof(ghf.Index))
    good = w.d_b.data_ptr()
    assert good % 16 == 0

    def calls(base, width):
        return [
            lambda: L.ghf_histogram_planes_delta(ctx.h, d_in.data_ptr(), base, n, width, 0, g_hists.data_ptr()),
            lambda: L.ghf_planes_split_delta(ctx.h, d_in.data_ptr(), base, n, width, g_planes.data_ptr(), stride),
            lambda: L.ghf_planes_merge_delta(ctx.h, d_good_planes.data_ptr(), stride, base, n, width, g_out.data_ptr()),
            lambda: L.ghf_planes_merge_range_delta(ctx.h, d_good_planes.data_ptr(), stride, base, first, count, width, g_out.data_ptr()),
            lambda: L.ghf_compress_planes_delta(ctx.h, d_in.data_ptr(), base, n, width, codes16.data_ptr(), ghf.PLANES_BUILD_CODES,
                                                g_out.data_ptr(), slot, g_bytes.data_ptr(), None),
            lambda: L.ghf_compress_planes_delta(ctx.h, d_in.data_ptr(), base, n, width, codes16.data_ptr(), 0, g_out.data_ptr(), slot,
                                                g_bytes.data_ptr(), idx16),
            lambda: L.ghf_decode_planes_delta(ctx.h, ptrs, sizes, codes16.data_ptr(), idx16, base, n, width, g_out.data_ptr(), big,
                                              g_bytes.data_ptr()),
            lambda: L.ghf_decode_planes_delta(ctx.h, ptrs, sizes, codes16.data_ptr(), None, base, n, width, g_out.data_ptr(), big,
                                              g_bytes.data_ptr()),
            lambda: L.ghf_decode_planes_range_delta(ctx.h, ptrs, sizes, codes16.data_ptr(), idx16, None, None, None, base, width, first,
                                                    count, g_out.data_ptr(), big),
            lambda: L.ghf_decode_planes_range_delta(ctx.h, ptrs, sizes, codes16.data_ptr(), None, infos, tptrs, tbytes, base, width,
                                                    first, count, g_out.data_ptr(), big),
        ]

    cases = [(None, e), (good + 8, e)] + [(good, bad) for bad in (0, 1, 3, 16)]
    for base, width in cases:
        for k, call in enumerate(calls(base, width)):
            assert call() == E_INVAL, (base, width, k)
        torch.cuda.synchronize()
        assert bool((g_planes == GUARD).all().item()) and bool((g_out == GUARD).all().item()), (base, width)
        assert bool((g_bytes == -1).all().item()) and bool((g_hists == GUARD_WORD).all().item()), (base, width)
        assert L.ghf_sync(ctx.h) == OK, (base, width)  # nothing latched either
        good_call(ghf, ctx, torch)
    for which in ("indexes", "tables"):
        decode_range_checked(ctx, torch, w, first, count, **w.source(which))


def test_the_other_refusals_of_the_plain_calls_hold_for_the_delta_form(env, world):
    """once each: GHF_E_EMPTY, GHF_E_CAP, a bad index, both sources or neither"""
    ghf, ctx, torch = env
    L = ctx.L
    w = world("fp32")
    e, n = w.e, N_ELEMS
    first, count = 1005, 5000
    d_in = to_dev(torch, w.x)
    base = w.d_b.data_ptr()
    slot, stride = ghf.planes_slot_bytes(n), (n + 255) & ~255
    d_good_planes, _ = ctx.planes_split_delta(d_in, w.d_b, e, n_elems=n)
    ctx.sync()
    g_planes = torch.full((e * stride + 64,), GUARD, dtype=torch.uint8, device="cuda")
    g_out = torch.full((e * max(slot, stride) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    g_bytes = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    g_hists = torch.full((e * ghf.NSYM,), GUARD_WORD, dtype=torch.int64, device="cuda")
    vp, sz = C.c_void_p, C.c_size_t
    ptrs = (vp * e)(*[s.data_ptr() for s in w.slots])
    sizes = (sz * e)(*w.sizes)
    codes = w.codes.data_ptr()
    infos = (ghf.SeekInfo * e)(*w.infos)
    tptrs = (vp * e)(*[t.data_ptr() for t in w.d_tables])
    tbytes = (sz * e)(*[t.size for t in w.tables])
    bad_idx = (ghf.Index * e)()
    C.memmove(bad_idx, w.idx, C.sizeof(bad_idx))
    bad_idx[1].n_symbols = n - 1
    out, cap = g_out.data_ptr(), n * e
    pl = d_good_planes.data_ptr()
    cases = [
        (E_EMPTY, lambda: L.ghf_histogram_planes_delta(ctx.h, d_in.data_ptr(), base, 0, e, 0, g_hists.data_ptr())),
        (E_INVAL, lambda: L.ghf_histogram_planes_delta(ctx.h, d_in.data_ptr(), base, n, e, 2, g_hists.data_ptr())),
        (E_EMPTY, lambda: L.ghf_planes_split_delta(ctx.h, d_in.data_ptr(), base, 0, e, g_planes.data_ptr(), stride)),
        (E_CAP, lambda: L.ghf_planes_split_delta(ctx.h, d_in.data_ptr(), base, n, e, g_planes.data_ptr(), (n & ~15) - 16)),
        (E_EMPTY, lambda: L.ghf_planes_merge_delta(ctx.h, pl, stride, base, 0, e, out)),
        (E_CAP, lambda: L.ghf_planes_merge_delta(ctx.h, pl, (n & ~15) - 16, base, n, e, out)),
        (E_EMPTY, lambda: L.ghf_planes_merge_range_delta(ctx.h, pl, stride, base, first, 0, e, out)),
        (E_CAP, lambda: L.ghf_planes_merge_range_delta(ctx.h, pl, stride, base, stride - count + 16, count, e, out)),
        (E_EMPTY, lambda: L.ghf_compress_planes_delta(ctx.h, d_in.data_ptr(), base, 0, e, codes, 0, out, slot, g_bytes.data_ptr(), None)),
        (E_CAP, lambda: L.ghf_compress_planes_delta(ctx.h, d_in.data_ptr(), base, n, e, codes, 0, out, slot - 16, g_bytes.data_ptr(), None)),
        (E_INVAL, lambda: L.ghf_compress_planes_delta(ctx.h, d_in.data_ptr(), base, n, e, codes, 2, out, slot, g_bytes.data_ptr(), None)),
        (E_INVAL, lambda: L.ghf_compress_planes_delta(ctx.h, d_in.data_ptr(), base, n, e, codes, 0, out, slot, g_bytes.data_ptr(), bad_idx)),
        (E_EMPTY, lambda: L.ghf_decode_planes_delta(ctx.h, ptrs, sizes, codes, None, base, 0, e, out, cap, g_bytes.data_ptr())),
        (E_CAP, lambda: L.ghf_decode_planes_delta(ctx.h, ptrs, sizes, codes, w.idx, base, n, e, out, cap - 1, g_bytes.data_ptr())),
        (E_INVAL, lambda: L.ghf_decode_planes_delta(ctx.h, ptrs, sizes, codes, bad_idx, base, n, e, out, cap, g_bytes.data_ptr())),
        (E_CAP, lambda: L.ghf_decode_planes_range_delta(ctx.h, ptrs, sizes, codes, w.idx, None, None, None, base, e, first, count, out,
                                                        count * e - 1)),
        (E_INVAL, lambda: L.ghf_decode_planes_range_delta(ctx.h, ptrs, sizes, codes, w.idx, infos, tptrs, tbytes, base, e, first, count,
                                                          out, cap)),  # both sources
        (E_INVAL, lambda: L.ghf_decode_planes_range_delta(ctx.h, ptrs, sizes, codes, None, None, None, None, base, e, first, count, out,
                                                          cap)),       # neither
        (E_INVAL, lambda: L.ghf_decode_planes_range_delta(ctx.h, ptrs, sizes, codes, bad_idx, None, None, None, base, e, first, count,
                                                          out, cap)),
        (E_INVAL, lambda: L.ghf_decode_planes_range_delta(ctx.h, ptrs, sizes, codes, w.idx, None, None, None, base, e, n - 10, 11, out,
                                                          cap)),
    ]
    for k, (want, call) in enumerate(cases):
        assert call() == want, k
        torch.cuda.synchronize()
        assert bool((g_planes == GUARD).all().item()) and bool((g_out == GUARD).all().item()), k
        assert bool((g_bytes == -1).all().item()) and bool((g_hists == GUARD_WORD).all().item()), k
        assert L.ghf_sync(ctx.h) == OK, k  # nothing latched either
    good_call(ghf, ctx, torch)
    for which in ("indexes", "tables"):
        decode_range_checked(ctx, torch, w, first, count, **w.source(which))
