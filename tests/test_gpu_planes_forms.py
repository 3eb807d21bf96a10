"""GPU: byte planes in three forms (ghf_planes_split_to / ghf_planes_merge_from / ghf_planes_merge_range_from /
ghf_compress_planes_forms / ghf_decode_planes_forms / ghf_decode_planes_forms_range).

Expected values come from numpy (plane p of x is x[p::E], a raw slot is that plane) and from the oracle through
tests/forms_model.py (the choice rule restated, the expected slots) alone.  Every output and every input sits between 0xA5
guard bytes.  Sizes, ranges, pairs of tensors and the guard helpers are those of the tests of the calls this family
generalises (tests/test_gpu_planes.py, test_gpu_planes_range.py, test_gpu_planes_delta.py, test_gpu_sparse.py)."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import forms_model as model
import pkgload
import test_gpu_planes as tp
import test_gpu_planes_delta as tpd
import test_gpu_planes_range as tr
import test_gpu_sparse as tgs

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_CORRUPT = 0, 1, 3, 5, 7
GUARD, PAD = tgs.GUARD, tgs.PAD
WIDTHS = (2, 4, 8)
T, G = tp.T, tp.G
COMPRESS_N = (1, 64, 4097, 65536 + 3)
assert COMPRESS_N == tp.COMPRESS_N
AUTO = model.AUTO
guarded, guarded_with, guards_intact, untouched, to_dev = tgs.guarded, tgs.guarded_with, tgs.guards_intact, tgs.untouched, tgs.to_dev
preloaded = tpd.preloaded


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    assert pkg.ghf.PLANES_TILE == T and pkg.ghf.PLANES_GROUPS == G and pkg.ghf.RAW_AUTO == AUTO == pkg.ghf.SPARSE_AUTO
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


@pytest.fixture(scope="module")
def pair():
    """two runs of uniform bytes with different seeds, long enough for every pointer-kernel case"""
    n = max(max(tp.split_sizes(e)[-1] * e for e in WIDTHS), max((tr.BASE + 15 + G * T[e] + 7) * e for e in WIDTHS))
    assert n < 64 << 20
    x, b = dg.uniform_bytes(n, seed=0x464F5258), dg.uniform_bytes(n, seed=0x464F5242)
    x.setflags(write=False)
    b.setflags(write=False)
    return x, b


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------- 1. the pointer kernels: split_to and merge_from
def separate(torch, e, n):
    """every plane in a guarded buffer of its own, at an address unrelated to the others"""
    bufs = [guarded(torch, n + 16 * p) for p in range(e)]  # different sizes: the allocator does not line them up
    return bufs, [b[PAD:] for b in bufs], [n + 16 * p for p in range(e)]


def reversed_slots(torch, e, n):
    """the planes are slots of ONE buffer, plane p in slot e - 1 - p"""
    stride = ((n + 15) & ~15) + 48
    buf = guarded(torch, e * stride)
    return [buf], [buf[PAD + (e - 1 - p) * stride :] for p in range(e)], None


@pytest.mark.parametrize("delta", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("e", WIDTHS)
def test_split_to_and_merge_from_are_exact_between_guard_bytes(env, pair, e, delta):
    ghf, ctx, torch = env
    for n in tp.split_sizes(e):
        x, b = pair[0][: n * e], pair[1][: n * e]
        src = x ^ b if delta else x
        (_, d_x), (_, d_b) = guarded_with(torch, x), guarded_with(torch, b)
        base = d_b if delta else None
        # the parents on the same data
        stride = (n + 15) & ~15
        d_par = torch.full((e * stride,), GUARD, dtype=torch.uint8, device="cuda")
        if delta:
            ctx.planes_split_delta(d_x, d_b, e, n_elems=n, d_planes=d_par, plane_stride=stride)
        else:
            ctx.planes_split(d_x, e, n_elems=n, d_planes=d_par, plane_stride=stride)
        layouts = [separate] + ([reversed_slots] if n == 3 * T[e] + 5 else [])
        for layout in layouts:
            bufs, planes, sizes = layout(torch, e, n)
            ctx.planes_split_to(d_x, planes, e, n_elems=n, d_base=base)
            back = guarded(torch, n * e)
            ctx.planes_merge_from(planes, n, e, d_out=back[PAD:], d_base=base)
            ctx.sync()
            h_par = host(d_par).reshape(e, stride)
            for p in range(e):
                got = host(planes[p][:n])
                assert np.array_equal(got, src[p::e]), (n, p, layout.__name__)
                assert np.array_equal(got, h_par[p, :n]), (n, p)
            if sizes:
                assert all(guards_intact(bf, sz) and bool((bf[PAD + n : PAD + sz] == GUARD).all().item()) for bf, sz in zip(bufs, sizes)), n
            else:  # one buffer: everything that is not a plane's n bytes is still guard
                h = host(bufs[0]).copy()
                st = ((n + 15) & ~15) + 48
                for p in range(e):
                    h[PAD + p * st : PAD + p * st + n] = GUARD
                assert (h == GUARD).all(), n
            assert np.array_equal(host(back[PAD : PAD + n * e]), x) and guards_intact(back, n * e), (n, layout.__name__)
            if delta:  # in place: the base is overwritten with base ^ delta
                buf = preloaded(torch, d_b)
                ctx.planes_merge_from(planes, n, e, d_out=buf[PAD:], d_base=buf[PAD : PAD + n * e])
                ctx.sync()
                assert np.array_equal(host(buf[PAD : PAD + n * e]), x) and guards_intact(buf, n * e), n
        # ... and merge_from on the parent's own planes, at planes + p * stride, gives what the parent's merge gives
        back = guarded(torch, n * e)
        ctx.planes_merge_from([d_par[p * stride :] for p in range(e)], n, e, d_out=back[PAD:], d_base=base)
        want = ctx.planes_merge_delta(d_par, stride, d_b, n, e) if delta else ctx.planes_merge(d_par, stride, n, e)
        ctx.sync()
        assert torch.equal(back[PAD : PAD + n * e], want[: n * e]) and guards_intact(back, n * e), n


# ---------------------------------------------------------------- 2. merge_range_from
def run_planes(torch, src, e, lead, count):
    """elements [0, lead + count) of src as planes in separate guarded buffers whose payload ends exactly at the run's last
    byte -> (buffers, the address views of every plane's byte of element `lead`)"""
    bufs, views = [], []
    for p in range(e):
        buf, _ = guarded_with(torch, np.ascontiguousarray(src[p : (lead + count) * e : e]))
        bufs.append(buf)
        views.append(buf[PAD + lead :])
    return bufs, views


def check_merge_range_from(ctx, torch, pair, e, skew, count, delta):
    lead = tr.BASE + skew
    x, b = pair[0][: (lead + count) * e], pair[1][: (lead + count) * e]
    src = x ^ b if delta else x
    bufs, views = run_planes(torch, src, e, lead, count)
    want = x[lead * e :]
    base = to_dev(torch, b[lead * e :]) if delta else None  # the base elements of the run, unskewed
    for inplace in (False, True) if delta else (False,):
        buf = preloaded(torch, base) if inplace else guarded(torch, count * e)
        ctx.planes_merge_range_from(views, count, e, d_out=buf[PAD:], d_base=buf[PAD : PAD + count * e] if inplace else base)
        ctx.sync()
        assert np.array_equal(host(buf[PAD : PAD + count * e]), want), (e, skew, count, delta, inplace)
        assert guards_intact(buf, count * e), (e, skew, count)
    for p, bf in enumerate(bufs):  # the sources are only read
        assert guards_intact(bf, lead + count), (e, skew, count, p)


@pytest.mark.parametrize("delta", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_from_every_skew_and_the_small_counts(env, pair, e, delta):
    ghf, ctx, torch = env
    for skew in range(16):
        check_merge_range_from(ctx, torch, pair, e, skew, 2 * 2048 + 77, delta)
    for count in (1, 15, 16, 17, T[e] - 1, T[e] + 1):
        for skew in (0, 1, 9, 15):
            check_merge_range_from(ctx, torch, pair, e, skew, count, delta)


@pytest.mark.parametrize("e", WIDTHS)
def test_merge_range_from_full_grid(env, pair, e):
    ghf, ctx, torch = env
    check_merge_range_from(ctx, torch, pair, e, 3, G * T[e] + 7, False)
    check_merge_range_from(ctx, torch, pair, e, 13, G * T[e] + 7, True)


def test_merge_range_from_refuses_pointers_that_disagree_modulo_16(env, pair):
    ghf, ctx, torch = env
    for e in WIDTHS:
        count, lead = 100, tr.BASE + 5
        _, views = run_planes(torch, pair[0][: (lead + count) * e], e, lead, count)
        buf = guarded(torch, count * e)
        for p in range(e):
            bad = list(views)
            bad[p] = views[p][1:]
            with pytest.raises(ghf.GhfError) as err:
                ctx.planes_merge_range_from(bad, count, e, d_out=buf[PAD:])
            assert err.value.status == E_INVAL
        # the two calls that take whole planes want them aligned
        for call in (lambda: ctx.planes_merge_from(views, count, e, d_out=buf[PAD:]),
                     lambda: ctx.planes_split_to(to_dev(torch, pair[0][: count * e]), views, e, n_elems=count)):
            with pytest.raises(ghf.GhfError) as err:
                call()
            assert err.value.status == E_INVAL
        assert untouched(torch, buf)


# ---------------------------------------------------------------- 3. and 4. compress, byte exact; round trips
def explicit_masks(e):
    return list(range(1 << e)) if e < 8 else [0, 0xFF, 0x3F, 0xAA]


def compress_forms(ghf, ctx, torch, d_new, d_base, e, n, raw, sparse, ranks=False):
    slot = ghf.planes_slot_bytes(n)
    d_out = torch.full((2 * e * slot,), GUARD, dtype=torch.uint8, device="cuda")
    d_codes = torch.full((2 * e, C.sizeof(ghf.Code)), GUARD, dtype=torch.uint8, device="cuda")
    return ctx.compress_planes_forms(d_new, e, raw_planes=raw, sparse_planes=sparse, d_base=d_base, n_elems=n, d_out=d_out,
                                     d_codes=d_codes, indexes=True, ranks=ranks)


def check_stored(ghf, r, want, waited):
    """every slot, size, code, side-car and reported mask of a compress call against the model"""
    e, n, slot = want.e, want.n, r["slot_bytes"]
    assert slot == ghf.planes_slot_bytes(n)
    assert (r["raw_planes"], r["sparse_planes"]) == (want.raw, want.sparse), (bin(r["raw_planes"]), bin(r["sparse_planes"]))
    assert r["n_vals"] == (want.n_vals if waited else [0] * e)
    h_out, sizes, h_codes, idx = host(r["out"]), [int(v) for v in host(r["out_bytes"])], host(r["codes"]), r["indexes"]
    print("stored", sizes, "total", sum(sizes), "of", n * e)
    assert sizes == want.sizes
    for j in range(2 * e):
        body = h_out[j * slot : (j + 1) * slot]
        if want.kind[j] is None:  # an empty slot reports 0, is unwritten, has no code and no side-car
            assert (body == GUARD).all() and (h_codes[j] == GUARD).all(), j
        elif want.kind[j] == "raw":  # the plane and nothing behind it; no code, no side-car
            assert np.array_equal(body[:n], want.data[j]) and (body[n:] == GUARD).all(), j
            assert (h_codes[j] == GUARD).all(), j
        else:
            assert np.array_equal(body[: sizes[j]], want.data[j]), j
            assert ghf.Code.from_buffer_copy(h_codes[j].tobytes()).as_dict() == want.tables[j], j
            assert idx[j].n_symbols == want.symbols[j], j
        if want.kind[j] != "image":
            assert not idx[j].d_chunk_bit and not idx[j].d_seg_bit and idx[j].n_symbols == 0, j
    return sizes


def slots_of(r):
    return [r["out"][j * r["slot_bytes"] : (j + 1) * r["slot_bytes"]] for j in range(2 * r["elem_bytes"])]


def round_trips(ctx, torch, r, sizes, new, d_base, what):
    """from side-cars and without them; plain, or with a base into a fresh output and in place"""
    e, n = r["elem_bytes"], r["n_elems"]
    for indexes in (r["indexes"], None):
        for inplace in (False, True) if d_base is not None else (False,):
            buf = preloaded(torch, d_base) if inplace else guarded(torch, n * e)
            base = buf[PAD : PAD + n * e] if inplace else d_base
            _, nbytes = ctx.decode_planes_forms(slots_of(r), sizes, r["codes"], r["raw_planes"], r["sparse_planes"], r["n_vals"], n, e,
                                                indexes=indexes, d_base=base, d_out=buf[PAD:], cap=n * e)
            ctx.sync()
            assert int(nbytes.item()) == n * e, (what, inplace)
            assert np.array_equal(host(buf[PAD : PAD + n * e]), new), (what, indexes is None, inplace)
            assert guards_intact(buf, n * e), (what, inplace)


@pytest.mark.parametrize("n", COMPRESS_N)
@pytest.mark.parametrize("e", WIDTHS)
def test_explicit_raw_masks_are_byte_exact_and_round_trip(env, e, n):
    """sparse_planes = 0 and every raw mask: a raw slot is the numpy plane, a dense slot oracle.compress of it.  Both masks
    are explicit and nothing is sparse, so the call does not wait for the device: what shows of that from outside is that
    h_n_vals comes back zeroed"""
    ghf, ctx, torch = env
    x = model.normal_elems(n, e)
    d_x = to_dev(torch, x)
    for raw in explicit_masks(e):
        want = model.Stored(x, e, raw=raw, sparse=0)
        r = compress_forms(ghf, ctx, torch, d_x, None, e, n, raw, 0)
        ctx.sync()
        sizes = check_stored(ghf, r, want, waited=False)
        assert torch.equal(d_x, to_dev(torch, x))  # the input is only read
        round_trips(ctx, torch, r, sizes, x, None, (e, n, raw))
        ctx.planes_index_free(r["indexes"])


PINNED = {65536: {2: (0b01, 88620), 4: (0b0111, 219692), 8: (0b00111111, 461747)},
          4097: {2: (0b01, 6608), 4: (0b0111, 14802), 8: (0b01111111, 30561)},
          64: {2: (0b11, 128), 4: (0b1111, 256), 8: (0xFF, 512)}, 1: {2: (0b11, 2), 4: (0b1111, 4), 8: (0xFF, 8)}}


@pytest.mark.parametrize("n", sorted(set(PINNED) | set(COMPRESS_N)))
@pytest.mark.parametrize("e", WIDTHS)
def test_raw_auto_chooses_the_model_s_masks_and_the_pinned_sizes(env, e, n):
    """default_rng(7).standard_normal(n): GHF_RAW_AUTO alone and both masks automatic store the same (no plane is 3/4 zeros)"""
    ghf, ctx, torch = env
    x = model.normal_elems(n, e)
    d_x = to_dev(torch, x)
    for sparse in (0, AUTO):
        want = model.Stored(x, e, raw=AUTO, sparse=sparse)
        r = compress_forms(ghf, ctx, torch, d_x, None, e, n, AUTO, sparse)
        ctx.sync()
        sizes = check_stored(ghf, r, want, waited=True)
        if n in PINNED:
            assert (r["raw_planes"], sum(sizes)) == PINNED[n][e]
        assert all(s <= n for s in sizes) and sum(sizes) <= n * e
        round_trips(ctx, torch, r, sizes, x, None, (e, n, sparse))
        ctx.planes_index_free(r["indexes"])


@pytest.mark.parametrize("e", WIDTHS)
def test_uniform_bytes_never_store_more_than_the_tensor(env, e):
    """dg.uniform_bytes(seed = 0x554E4946): every plane's image is larger than the plane, so everything is raw"""
    ghf, ctx, torch = env
    n = 65536 + 3
    x = dg.uniform_bytes(n * e, seed=0x554E4946)
    want = model.Stored(x, e, raw=AUTO, sparse=AUTO)
    r = compress_forms(ghf, ctx, torch, to_dev(torch, x), None, e, n, AUTO, AUTO)
    ctx.sync()
    sizes = check_stored(ghf, r, want, waited=True)
    assert sum(sizes) <= n * e and r["raw_planes"] == (1 << e) - 1
    round_trips(ctx, torch, r, sizes, x, None, e)
    ctx.planes_index_free(r["indexes"])


@pytest.mark.parametrize("step", [1e-3, 1e-1])
@pytest.mark.parametrize("n", (4097, 65536 + 3))
@pytest.mark.parametrize("e", WIDTHS)
def test_with_a_base_both_automatic_masks_equal_the_model(env, e, n, step):
    """the stepped pairs of tests/test_gpu_planes_delta.py: the high planes of new ^ base go sparse, the low ones raw"""
    ghf, ctx, torch = env
    new, base = tgs.stepped(n, e, step)
    want = model.Stored(new ^ base, e, raw=AUTO, sparse=AUTO)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    r = compress_forms(ghf, ctx, torch, d_new, d_base, e, n, AUTO, AUTO, ranks=True)
    ctx.sync()
    sizes = check_stored(ghf, r, want, waited=True)
    assert torch.equal(d_new, to_dev(torch, new)) and torch.equal(d_base, to_dev(torch, base))
    round_trips(ctx, torch, r, sizes, new, d_base, (e, n, step))
    ctx.planes_index_free(r["indexes"])


def three_forms(n, seed=0x33464F52):
    """fp32-wide elements made by hand: planes 0 and 1 uniform bytes (raw), plane 2 skewed (dense), plane 3 mostly zero
    (sparse)"""
    rng = np.random.default_rng(seed)
    x = np.empty((n, 4), dtype=np.uint8)
    x[:, 0], x[:, 1] = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    x[:, 2] = np.minimum(rng.geometric(0.3, n), 255).astype(np.uint8)
    x[:, 3] = rng.integers(1, 256, n, dtype=np.uint8) * (rng.integers(0, 64, n) == 0)
    return x.reshape(-1)


def test_one_tensor_in_all_three_forms(env):
    ghf, ctx, torch = env
    n = 65536 + 3
    x = three_forms(n)
    want = model.Stored(x, 4, raw=AUTO, sparse=AUTO)
    assert (want.raw, want.sparse) == (0b0011, 0b1000)
    assert want.kind == ["raw", "raw", "image", "image", None, None, None, "image"]
    r = compress_forms(ghf, ctx, torch, to_dev(torch, x), None, 4, n, AUTO, AUTO, ranks=True)
    ctx.sync()
    sizes = check_stored(ghf, r, want, waited=True)
    assert sizes[2] == model.image(want.planes[2]).size < n  # the oracle's sizes, taken here
    round_trips(ctx, torch, r, sizes, x, None, "three forms")
    # the same masks given explicitly: the one wait remains (a sparse plane's value count), the bytes are the same
    r2 = compress_forms(ghf, ctx, torch, to_dev(torch, x), None, 4, n, 0b0011, 0b1000)
    ctx.sync()
    check_stored(ghf, r2, want, waited=True)
    for rr in (r, r2):
        ctx.planes_index_free(rr["indexes"])


def test_an_all_zero_tensor_is_raw_when_small_and_sparse_when_large(env):
    """the two-header rule: a sparse plane stores 2 * ghf_header_bytes(1) = 2096 bytes of headers"""
    ghf, ctx, torch = env
    for n, masks in ((64, (0b11, 0)), (65536, (0, 0b11))):
        x = np.zeros(n * 2, dtype=np.uint8)
        want = model.Stored(x, 2, raw=AUTO, sparse=AUTO)
        assert (want.raw, want.sparse) == masks
        r = compress_forms(ghf, ctx, torch, to_dev(torch, x), None, 2, n, AUTO, AUTO)
        ctx.sync()
        sizes = check_stored(ghf, r, want, waited=True)
        round_trips(ctx, torch, r, sizes, x, None, n)
        ctx.planes_index_free(r["indexes"])


@pytest.mark.parametrize("e", WIDTHS)
def test_a_lying_side_car_leaves_the_output_alone_and_in_place_the_base(env, e):
    """plane 0 raw, the others dense, against a base; the last plane's side-car puts the end of segment 63 of block 4 one bit
    late, as in tests/test_gpu_planes_delta.py: GHF_E_CORRUPT latches and the merge behind it stores nothing"""
    ghf, ctx, torch = env
    n = 65536 + 3
    new, base = tpd.stepped(n, e)
    d_base = to_dev(torch, base)
    r = compress_forms(ghf, ctx, torch, to_dev(torch, new), d_base, e, n, 0b1, 0)
    ctx.sync()
    sizes = [int(v) for v in host(r["out_bytes"])]
    idx = r["indexes"]
    chunk, seg = ctx.index_to_host(idx[e - 1])
    seg = seg.copy()
    seg[4 * 64 + 63] += 1
    d_chunk, d_seg = to_dev(torch, chunk.view(np.uint8)), to_dev(torch, seg.view(np.uint8))
    bad = (ghf.Index * (2 * e))()
    for j in range(2 * e):
        C.memmove(C.byref(bad[j]), C.byref(idx[j]), C.sizeof(ghf.Index))
    bad[e - 1].d_chunk_bit, bad[e - 1].d_seg_bit = d_chunk.data_ptr(), d_seg.data_ptr()

    def decode(base_arg, out):
        ctx.decode_planes_forms(slots_of(r), sizes, r["codes"], 0b1, 0, r["n_vals"], n, e, indexes=bad, d_base=base_arg, d_out=out, cap=n * e)

    buf = guarded(torch, n * e)
    decode(d_base, buf[PAD:])
    assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
    assert untouched(torch, buf)
    assert ctx.L.ghf_clear_status(ctx.h) == OK
    buf = preloaded(torch, d_base)
    decode(buf[PAD : PAD + n * e], buf[PAD:])
    assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
    assert np.array_equal(host(buf[PAD : PAD + n * e]), base) and guards_intact(buf, n * e)
    assert ctx.L.ghf_clear_status(ctx.h) == OK
    round_trips(ctx, torch, r, sizes, new, d_base, "the true side-cars")
    ctx.planes_index_free(idx)


@pytest.mark.parametrize("e", WIDTHS)
def test_an_all_raw_tensor_decodes_on_a_context_that_never_compressed(env, e):
    """nothing but the merge: no code, no side-car, no workspace of an earlier call.  And behind a latched status that merge
    stores nothing"""
    ghf, ctx, torch = env
    n, all_raw = 4097, (1 << e) - 1
    x = model.normal_elems(n, e)
    planes = [guarded_with(torch, pl) for pl in model.planes_of(x, e)]
    streams = [v for _, v in planes] + [None] * e
    sizes = [n] * e + [0] * e
    fresh = ghf.Context(0)
    try:
        buf = guarded(torch, n * e)
        _, nbytes = fresh.decode_planes_forms(streams, sizes, None, all_raw, 0, [0] * e, n, e, indexes=None, d_out=buf[PAD:], cap=n * e)
        fresh.sync()
        assert int(nbytes.item()) == n * e and np.array_equal(host(buf[PAD : PAD + n * e]), x) and guards_intact(buf, n * e)
        # latch GHF_E_CORRUPT with a sparse merge that is told of one value too many (tests/test_gpu_sparse.py)
        mask, vals = tgs.sparse_form(np.arange(1, 65, dtype=np.uint8))
        junk = guarded(torch, 64)
        fresh.sparse_merge(to_dev(torch, mask), to_dev(torch, np.append(vals, 0)), vals.size + 1, 64, d_out=junk[PAD:])
        buf = guarded(torch, n * e)
        fresh.decode_planes_forms(streams, sizes, None, all_raw, 0, [0] * e, n, e, indexes=None, d_out=buf[PAD:], cap=n * e)
        assert fresh.L.ghf_sync(fresh.h) == E_CORRUPT
        assert untouched(torch, buf) and untouched(torch, junk)
        assert fresh.L.ghf_clear_status(fresh.h) == OK
    finally:
        fresh.close()
    assert all(guards_intact(b, n) for b, _ in planes)


# ---------------------------------------------------------------- 5. range
N_ELEMS = tr.N_ELEMS
RANGES = tr.RANGES


class World:
    """one tensor compressed once by ghf_compress_planes_forms with side-cars and rank tables; the seek table of every stream
    that has a code through host bytes and back"""

    def __init__(self, ghf, ctx, torch, x, b, e, raw, sparse):
        self.e, self.n, self.x, self.b = e, x.size // e, x, b
        self.d_b = None if b is None else to_dev(torch, b)
        r = compress_forms(ghf, ctx, torch, to_dev(torch, x), self.d_b, e, self.n, raw, sparse, ranks=True)
        ctx.sync()
        self.r, self.raw, self.sparse = r, r["raw_planes"], r["sparse_planes"]
        self.sizes = [int(v) for v in host(r["out_bytes"])]
        self.slots = slots_of(r)
        self.infos, self.d_tables = [None] * (2 * e), [None] * (2 * e)
        for j in range(2 * e):
            if r["indexes"][j].n_symbols:
                d_table = ctx.seek_pack(r["indexes"][j])
                ctx.sync()
                t = host(d_table).copy()
                self.infos[j], self.d_tables[j] = ghf.seek_parse(t), to_dev(torch, t)
        self.ranks = [None] * e
        for p in range(e):
            if (self.sparse >> p) & 1:
                t = host(r["ranks"][p * r["rank_slot_bytes"] :][: ghf.sparse_rank_bytes(self.n)]).copy()
                self.ranks[p] = (ghf.sparse_rank_parse(t), t)

    def source(self, which):
        return {"indexes": self.r["indexes"]} if which == "indexes" else {"infos": self.infos, "d_tables": self.d_tables}

    def check(self, ctx, torch, first, count, which):
        e = self.e
        want = self.x[first * e : (first + count) * e]
        base = None if self.d_b is None else self.d_b[first * e : (first + count) * e].clone()
        for inplace in (False, True) if base is not None else (False,):
            buf = preloaded(torch, base) if inplace else guarded(torch, count * e)
            ctx.decode_planes_forms_range(self.slots, self.sizes, self.r["codes"], self.raw, self.sparse, self.ranks, self.n, e, first, count,
                                          d_base=buf[PAD : PAD + count * e] if inplace else base, d_out=buf[PAD:], cap=count * e,
                                          **self.source(which))
            ctx.sync()
            assert np.array_equal(host(buf[PAD : PAD + count * e]), want), (first, count, which, inplace)
            assert guards_intact(buf, count * e), (first, count, which, inplace)


def range_masks(e):
    return {"dense": 0, "raw": (1 << e) - 1, "auto": AUTO}


@pytest.mark.parametrize("which", ["indexes", "tables"])
@pytest.mark.parametrize("based", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("mask", ["dense", "raw", "auto"])
@pytest.mark.parametrize("e", (2, 4))
def test_decode_forms_range(env, e, mask, based, which):
    """bf16 / fp32 of N_ELEMS elements over the ranges of tests/test_gpu_planes_range.py; the index, info and table entries of a
    raw plane are null"""
    ghf, ctx, torch = env
    if based:
        x, b = tpd.stepped(N_ELEMS, e)
    else:
        x, b = model.normal_elems(N_ELEMS, e), None
    w = World(ghf, ctx, torch, x, b, e, range_masks(e)[mask], 0)
    if mask == "auto" and not based:
        assert 0 < w.raw < (1 << e) - 1, bin(w.raw)  # a tensor with raw and dense planes (a small step leaves no plane of the XOR to be raw)
    for p in range(e):
        if (w.raw >> p) & 1:
            assert w.infos[p] is None and w.d_tables[p] is None and not w.r["indexes"][p].d_seg_bit
    for first, count in RANGES:
        w.check(ctx, torch, first, count, which)
    buf = guarded(torch, 64)  # count == 0: GHF_OK, nothing queued, nothing written
    ctx.decode_planes_forms_range(w.slots, w.sizes, w.r["codes"], w.raw, w.sparse, w.ranks, w.n, e, 1005, 0, d_out=buf[PAD:], cap=64,
                                  d_base=None if w.d_b is None else w.d_b, **w.source(which))
    assert ctx.L.ghf_sync(ctx.h) == OK and untouched(torch, buf)
    ctx.planes_index_free(w.r["indexes"])


R = 32768
MIXED_N = 2 * R + 1061
MIXED_RANGES = ((0, MIXED_N), (R - 100, 300), (100, 40000), (R + 15, 4097), (2 * R - 1, 2), (MIXED_N - 1, 1), (7, 9))
assert any(f // R != (f + c - 1) // R and f % 16 for f, c in MIXED_RANGES)


@pytest.mark.parametrize("which", ["indexes", "tables"])
@pytest.mark.parametrize("based", [False, True], ids=["plain", "base"])
def test_decode_forms_range_of_a_sparse_a_dense_and_two_raw_planes(env, based, which):
    """the hand-made tensor of three forms with its rank tables, over ranges that cross a rank block; with a base the tensor is
    the XOR, so that new ^ base has those planes"""
    ghf, ctx, torch = env
    d = three_forms(MIXED_N)
    b = dg.uniform_bytes(MIXED_N * 4, seed=0x4D495842) if based else None
    x = d ^ b if based else d
    w = World(ghf, ctx, torch, x, b, 4, AUTO, AUTO)
    assert (w.raw, w.sparse) == (0b0011, 0b1000)
    for first, count in MIXED_RANGES:
        w.check(ctx, torch, first, count, which)
    ctx.planes_index_free(w.r["indexes"])


# ---------------------------------------------------------------- 6. refusals on a live context, nothing queued
def test_refusals_leave_every_output_untouched(env):
    ghf, ctx, torch = env
    L = ctx.L
    e, n = 4, 4097
    x = model.normal_elems(n, e)
    d_x = to_dev(torch, x)
    slot = ghf.planes_slot_bytes(n)
    out = guarded(torch, 2 * e * slot)
    sizes_out = torch.full((2 * e,), tgs.GUARD_WORD, dtype=torch.int64, device="cuda")
    raw, chosen, n_vals = C.c_uint(0), C.c_uint(0), (C.c_size_t * e)()

    def compress(rm, sm, d_in=d_x.data_ptr(), d_base=None, n_elems=n, width=e, d_out=out[PAD:].data_ptr(), slot_bytes=slot,
                 d_bytes=sizes_out.data_ptr(), h_raw=C.byref(raw)):
        return L.ghf_compress_planes_forms(ctx.h, d_in, d_base, n_elems, width, rm, sm, d_out, slot_bytes, d_bytes, None, None, None, 0,
                                           h_raw, C.byref(chosen), n_vals)

    # the mask errors
    for rm, sm in ((1 << e, 0), (AUTO | 1, 0), (0, AUTO | 1), (0, 1 << e), (0b0101, 0b0100), (0xF, 0x1)):
        assert compress(rm, sm) == E_INVAL, (rm, sm)
    for width in (0, 1, 3, 16):
        assert compress(AUTO, 0, width=width) == E_INVAL, width
    assert compress(AUTO, 0, d_in=None) == E_INVAL and compress(AUTO, 0, d_out=None) == E_INVAL
    assert compress(AUTO, 0, d_bytes=None) == E_INVAL and compress(AUTO, 0, h_raw=None) == E_INVAL
    assert compress(AUTO, 0, d_in=d_x.data_ptr() + 1) == E_INVAL and compress(AUTO, 0, d_base=d_x.data_ptr() + 8) == E_INVAL
    assert compress(AUTO, 0, slot_bytes=slot + 8) == E_INVAL
    assert compress(AUTO, 0, n_elems=0) == E_EMPTY
    assert compress(AUTO, 0, slot_bytes=slot - 16) == E_CAP
    assert untouched(torch, out) and bool((sizes_out == tgs.GUARD_WORD).all().item())

    # a good call, then the decodes' refusals
    r = compress_forms(ghf, ctx, torch, d_x, None, e, n, 0b0011, 0)
    ctx.sync()
    sizes = [int(v) for v in host(r["out_bytes"])]
    slots = slots_of(r)
    buf = guarded(torch, n * e)

    def decode(rm, sm, streams=slots, stream_bytes=sizes, cap=n * e, n_elems=n, d_out=buf[PAD:]):
        try:
            ctx.decode_planes_forms(streams, stream_bytes, r["codes"], rm, sm, r["n_vals"], n_elems, e, indexes=r["indexes"], d_out=d_out, cap=cap)
        except ghf.GhfError as err:
            return err.status
        return OK

    def decode_range(rm, sm, streams=slots, stream_bytes=sizes, cap=100 * e, first=5, count=100, d_out=buf[PAD:]):
        try:
            ctx.decode_planes_forms_range(streams, stream_bytes, r["codes"], rm, sm, None, n, e, first, count, indexes=r["indexes"], d_out=d_out,
                                          cap=cap)
        except ghf.GhfError as err:
            return err.status
        return OK

    for call in (decode, decode_range):
        for rm, sm in ((AUTO, 0), (1 << e, 0), (0b0011 | AUTO, 0), (0b0011, 0b0001)):
            assert call(rm, sm) == E_INVAL, (call.__name__, rm, sm)
        short = list(sizes)
        short[1] = n - 1  # a raw stream is n_elems bytes and nothing else
        assert call(0b0011, 0, stream_bytes=short) == E_INVAL
        off = list(slots)
        off[0] = slots[0][1:]  # a misaligned raw pointer
        assert call(0b0011, 0, streams=off) == E_INVAL
        gone = list(slots)
        gone[1] = None  # a null required pointer
        assert call(0b0011, 0, streams=gone) == E_INVAL
        assert call(0b0011, 0, cap=16) == E_CAP
    assert decode(0b1111, 0, n_elems=0, stream_bytes=[0] * (2 * e)) == E_EMPTY  # all raw: no index stands in front of the size check
    assert decode_range(0b0011, 0, first=n - 50, count=100) == E_INVAL  # a range past n_elems
    assert untouched(torch, buf)
    assert L.ghf_sync(ctx.h) == OK
    # the pointer calls
    planes = [guarded(torch, n) for _ in range(e)]
    views = [p[PAD:] for p in planes]
    ptrs = ctx._plane_ptrs(views, e)
    for width in (0, 1, 3, 16):
        assert L.ghf_planes_split_to(ctx.h, d_x.data_ptr(), None, n, width, ptrs) == E_INVAL
        assert L.ghf_planes_merge_from(ctx.h, ptrs, None, n, width, buf[PAD:].data_ptr()) == E_INVAL
        assert L.ghf_planes_merge_range_from(ctx.h, ptrs, None, n, width, buf[PAD:].data_ptr()) == E_INVAL
    assert L.ghf_planes_split_to(ctx.h, d_x.data_ptr(), None, 0, e, ptrs) == E_EMPTY
    assert L.ghf_planes_merge_from(ctx.h, ptrs, None, 0, e, buf[PAD:].data_ptr()) == E_EMPTY
    assert L.ghf_planes_split_to(ctx.h, d_x.data_ptr(), d_x.data_ptr() + 4, n, e, ptrs) == E_INVAL  # a misaligned base
    assert L.ghf_planes_split_to(ctx.h, None, None, n, e, ptrs) == E_INVAL and L.ghf_planes_split_to(ctx.h, d_x.data_ptr(), None, n, e, None) == E_INVAL
    hole = ctx._plane_ptrs([views[0], 0, views[2], views[3]], e)
    assert L.ghf_planes_split_to(ctx.h, d_x.data_ptr(), None, n, e, hole) == E_INVAL
    assert L.ghf_planes_merge_from(ctx.h, hole, None, n, e, buf[PAD:].data_ptr()) == E_INVAL
    assert all(untouched(torch, p) for p in planes) and untouched(torch, buf)
    assert L.ghf_sync(ctx.h) == OK
    ctx.planes_index_free(r["indexes"])


# ---------------------------------------------------------------- 7. the existing calls are unchanged
@pytest.mark.parametrize("form", ["plain", "delta"])
def test_the_sparse_calls_store_and_read_what_they_did(env, form):
    """in a process that has run the forms calls: ghf_compress_planes_sparse_ranked[_delta] still writes the model's bytes of
    tests/test_gpu_sparse.py, and ghf_decode_planes_sparse_range[_delta] still reads them back"""
    ghf, ctx, torch = env
    e, n, mask = 4, 65536 + 3, 0b1010
    x = model.normal_elems(n, e)
    r0 = compress_forms(ghf, ctx, torch, to_dev(torch, x), None, e, n, AUTO, AUTO)  # the new path first, on the same context
    ctx.sync()
    ctx.planes_index_free(r0["indexes"])
    new, base, src, images, tables, n_vals = tgs.want_for(form, e, n, mask)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    slot = ghf.planes_slot_bytes(n)
    d_out = torch.full((2 * e * slot,), GUARD, dtype=torch.uint8, device="cuda")
    if form == "delta":
        r = ctx.compress_planes_sparse_ranked_delta(d_new, d_base, e, sparse_planes=mask, n_elems=n, d_out=d_out, indexes=True)
    else:
        r = ctx.compress_planes_sparse_ranked(d_new, e, sparse_planes=mask, n_elems=n, d_out=d_out, indexes=True)
    ctx.sync()
    assert r["sparse_planes"] == mask and r["n_vals"] == n_vals
    h_out, sizes, h_codes = host(r["out"]), [int(v) for v in host(r["out_bytes"])], host(r["codes"])
    for j in range(2 * e):
        if images[j] is None:
            assert sizes[j] == 0 and (h_out[j * slot : (j + 1) * slot] == GUARD).all(), j
            continue
        assert sizes[j] == images[j].size and np.array_equal(h_out[j * slot :][: sizes[j]], images[j]), j
        assert ghf.Code.from_buffer_copy(h_codes[j].tobytes()).as_dict() == tables[j], j
    ranks = [None] * e
    for p in range(e):
        if (mask >> p) & 1:
            t = host(r["ranks"][p * r["rank_slot_bytes"] :][: ghf.sparse_rank_bytes(n)]).copy()
            ranks[p] = (ghf.sparse_rank_parse(t), t)
    slots = [r["out"][j * slot : (j + 1) * slot] for j in range(2 * e)]
    for first, count in ((R - 100, 300), (1000 + 7, 2 * 2048 + 77), (0, n)):
        buf = guarded(torch, count * e)
        if form == "delta":
            ctx.decode_planes_sparse_range_delta(slots, sizes, r["codes"], d_base[first * e : (first + count) * e].clone(), mask, ranks, n, e,
                                                 first, count, indexes=r["indexes"], d_out=buf[PAD:], cap=count * e)
        else:
            ctx.decode_planes_sparse_range(slots, sizes, r["codes"], mask, ranks, n, e, first, count, indexes=r["indexes"], d_out=buf[PAD:],
                                           cap=count * e)
        ctx.sync()
        assert np.array_equal(host(buf[PAD : PAD + count * e]), new[first * e : (first + count) * e]), (first, count)
        assert guards_intact(buf, count * e)
    ctx.planes_index_free(r["indexes"])
