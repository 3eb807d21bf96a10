"""GPU: zero-suppressed byte planes (ghf_sparse_split / ghf_sparse_merge / ghf_compress_planes_sparse[_delta] /
ghf_decode_planes_sparse[_delta]).

Expected values come from numpy (the mask is np.packbits(x != 0, bitorder="little"), the values are x[x != 0]) and from the
oracle (oracle.compress / histogram / build_code) alone.  Every output sits between guard bytes, every input too: the byte
behind a string's last one is 0xA5, so a kernel that takes a byte behind the end for a value shows.  The pairs of tensors
are those of tests/test_gpu_planes_delta.py."""
import ctypes as C

import numpy as np
import pytest

import pkgload
import test_gpu_planes_delta as tpd
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_CORRUPT = 0, 1, 3, 5, 7
GUARD = 0xA5
GUARD_WORD = -0x5A5A5A5A5A5A5A5B
PAD = 64  # guard bytes in front of and behind a buffer; keeps it 16-byte aligned
WIDTHS = (2, 4, 8)
COMPRESS_N = (1, 64, 4097, 65536 + 3)
assert COMPRESS_N == tpd.COMPRESS_N
T, G = 4096, 256 * 16


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    assert pkg.ghf.SPARSE_TILE == T and pkg.ghf.SPARSE_GROUPS == G and pkg.ghf.SPARSE_SCAN == G
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def guarded(torch, nbytes):
    return torch.full((PAD + nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda")


def guarded_with(torch, a):
    """a host array in the middle of a guarded device buffer -> (buffer, the payload's view)"""
    buf = guarded(torch, a.size)
    if a.size:
        buf[PAD : PAD + a.size] = torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()
    return buf, buf[PAD : PAD + a.size]


def guards_intact(buf, nbytes):
    return bool((buf[:PAD] == GUARD).all().item()) and bool((buf[PAD + nbytes :] == GUARD).all().item())


def untouched(torch, buf):
    torch.cuda.synchronize()
    return bool((buf == GUARD).all().item())


def sparse_form(x):
    """(mask, vals) of a byte string, from numpy alone"""
    nz = x != 0
    return np.packbits(nz, bitorder="little"), np.ascontiguousarray(x[nz])


# ---------------------------------------------------------------- 1. split and merge
# T - 1 .. T + 1: one tile and its neighbours; 3 T + 5: a slab of whole tiles and a ragged one; the last size: G + 2 tiles, so
# that every workgroup with a slab takes two tiles and the upper half of the grid takes none (the scan takes one count per
# workgroup and so never more than one step: there is no larger edge of its own)
SIZES = (1, 7, 8, 9, 15, 16, 17, 127, 128, 129, T - 1, T, T + 1, 3 * T + 5, (G + 1) * T + 5)
assert SIZES[-1] < 64 << 20 and -(-SIZES[-1] // T) > G


def nonzero_bytes(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8)


def single(at):
    def make(n, rng):
        if at(n) < 0 or at(n) >= n:
            return None
        x = np.zeros(n, dtype=np.uint8)
        x[at(n)] = 0x5A
        return x

    return make


def density(num, den):
    return lambda n, rng: nonzero_bytes(rng, n) * (rng.integers(0, den, n) < num).astype(np.uint8)


def comb(n, rng):
    """tiles alternately all zero and all non-zero, the first one zero: offsets carry across empty tiles"""
    return nonzero_bytes(rng, n) * ((np.arange(n) // T) % 2).astype(np.uint8)


def comb_from_the_first_tile(n, rng):
    return nonzero_bytes(rng, n) * ((np.arange(n) // T + 1) % 2).astype(np.uint8)


def two_values(n, rng):
    return np.array([0x01, 0x80], dtype=np.uint8)[rng.integers(0, 2, n)] * rng.integers(0, 2, n, dtype=np.uint8)


PATTERNS = {
    "all_zero": lambda n, rng: np.zeros(n, dtype=np.uint8),
    "all_ff": lambda n, rng: np.full(n, 0xFF, dtype=np.uint8),
    "single_at_0": single(lambda n: 0),
    "single_at_n-1": single(lambda n: n - 1),
    "single_at_T-1": single(lambda n: T - 1),
    "single_at_T": single(lambda n: T),
    "density_1_64": density(1, 64),
    "density_1_2": density(1, 2),
    "density_255_256": density(255, 256),
    "comb": comb,
    "comb_from_the_first_tile": comb_from_the_first_tile,
    "values_01_80": two_values,
}


def check_split_and_merge(ghf, ctx, torch, x, what):
    n = x.size
    mask, vals = sparse_form(x)
    nv, mb = vals.size, mask.size
    assert mb == ghf.sparse_mask_bytes(n) and (n % 8 == 0 or mask[-1] >> (n % 8) == 0)
    L = ctx.L
    _, d_x = guarded_with(torch, x)
    mbuf, vbuf = guarded(torch, mb), guarded(torch, nv)
    count = torch.full((3,), GUARD_WORD, dtype=torch.int64, device="cuda")
    ctx.sparse_split(d_x, n, d_mask=mbuf[PAD:], d_vals=vbuf[PAD:], vals_cap=nv, n_vals=count[1:2])
    obuf = guarded(torch, n)
    ctx.sparse_merge(mbuf[PAD:], vbuf[PAD:], nv, n, d_out=obuf[PAD:])
    # ... and from buffers the split did not write: the true strings with guard bytes behind them
    (_, d_mask), (tbuf, _) = guarded_with(torch, mask), guarded_with(torch, vals)
    d_vals = tbuf[PAD:]  # never an empty view: a merge that is told of one value too many still has a pointer to take
    obuf2 = guarded(torch, n)
    ctx.sparse_merge(d_mask, d_vals if nv else None, nv, n, d_out=obuf2[PAD:])
    assert L.ghf_sync(ctx.h) == OK, what
    assert np.array_equal(mbuf[PAD : PAD + mb].cpu().numpy(), mask), what
    assert np.array_equal(vbuf[PAD : PAD + nv].cpu().numpy(), vals), what
    assert count.cpu().tolist() == [GUARD_WORD, nv, GUARD_WORD], what
    assert guards_intact(mbuf, mb) and guards_intact(vbuf, nv), what
    for b in (obuf, obuf2):
        assert np.array_equal(b[PAD : PAD + n].cpu().numpy(), x), what
        assert guards_intact(b, n), what
    if nv:  # one byte of capacity too few: the values stay away, the mask and the count that would have sufficed arrive
        mbuf, vbuf = guarded(torch, mb), guarded(torch, nv)
        count = torch.full((3,), GUARD_WORD, dtype=torch.int64, device="cuda")
        ctx.sparse_split(d_x, n, d_mask=mbuf[PAD:], d_vals=vbuf[PAD:], vals_cap=nv - 1, n_vals=count[1:2])
        assert L.ghf_sync(ctx.h) == E_CAP, what
        assert untouched(torch, vbuf), what
        assert np.array_equal(mbuf[PAD : PAD + mb].cpu().numpy(), mask) and guards_intact(mbuf, mb), what
        assert count.cpu().tolist() == [GUARD_WORD, nv, GUARD_WORD], what
        assert L.ghf_clear_status(ctx.h) == OK
    damaged = [("n_vals + 1", d_mask, nv + 1)]
    if nv:
        damaged.append(("n_vals - 1", d_mask, nv - 1))
    if n % 8:
        bad = mask.copy()
        bad[-1] |= 1 << (n % 8)
        damaged.append(("pad bit", guarded_with(torch, bad)[1], nv))
    for why, m, k in damaged:
        obuf = guarded(torch, n)
        ctx.sparse_merge(m, d_vals, k, n, d_out=obuf[PAD:])
        assert L.ghf_sync(ctx.h) == E_CORRUPT, (what, why)
        assert untouched(torch, obuf), (what, why)
        # while the status stands, a good merge stores nothing either
        ctx.sparse_merge(d_mask, d_vals, nv, n, d_out=obuf[PAD:])
        assert L.ghf_sync(ctx.h) == E_CORRUPT and untouched(torch, obuf), (what, why)
        assert L.ghf_clear_status(ctx.h) == OK
    obuf = guarded(torch, n)  # the context works again
    ctx.sparse_merge(d_mask, d_vals, nv, n, d_out=obuf[PAD:])
    assert L.ghf_sync(ctx.h) == OK, what
    assert np.array_equal(obuf[PAD : PAD + n].cpu().numpy(), x) and guards_intact(obuf, n), what


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_split_and_merge_are_exact_between_guard_bytes(env, pattern):
    ghf, ctx, torch = env
    for n in SIZES:
        x = PATTERNS[pattern](n, np.random.default_rng(n))
        if x is not None:
            check_split_and_merge(ghf, ctx, torch, x, (pattern, n))


# ---------------------------------------------------------------- 2. the plane calls
def stepped(n, e, step, seed=7):
    """the recipe of tests/test_gpu_planes_delta.py with the step as an argument -> (new, base) as bytes"""
    dt = np.float64 if e == 8 else np.float32
    w = np.random.default_rng(seed).standard_normal(n).astype(dt)
    g = np.random.default_rng(seed + 1).standard_normal(n).astype(dt)
    return tpd.as_bytes((w + dt(step) * g).astype(dt), e), tpd.as_bytes(w, e)


def masks_for(e):
    return {"none": 0, "all": (1 << e) - 1, "alternating": 0x55 & ((1 << e) - 1)}


_want = {}


def want_for(form, e, n, mask):
    """what the call must store for the planes of `new` (form "plain") or of new ^ base ("delta"), planes in `mask` sparse:
    (new, base, source bytes, [expected image of slot j or None], [expected tables or None], n_vals)"""
    key = (form, e, n, mask)
    if key not in _want:
        new, base = tpd.stepped(n, e)
        src = new ^ base if form == "delta" else new
        planes = tpd.planes_of(src, e)
        streams = [None] * (2 * e)
        for p, pl in enumerate(planes):
            if (mask >> p) & 1:
                m, v = sparse_form(pl)
                streams[p] = m
                streams[e + p] = v if v.size else None
            else:
                streams[p] = pl
        images = [None if s is None else orc.compress(s) for s in streams]
        tables = [None if s is None else orc.build_code(orc.histogram(s)).as_dict() for s in streams]
        _want[key] = (new, base, src, images, tables, [int(np.count_nonzero(pl)) for pl in planes])
    return _want[key]


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def compress_sparse(ghf, ctx, torch, form, d_new, d_base, e, n, mask, indexes=True):
    slot = ghf.planes_slot_bytes(n)
    d_out = torch.full((2 * e * slot,), GUARD, dtype=torch.uint8, device="cuda")
    if form == "delta":
        return ctx.compress_planes_sparse_delta(d_new, d_base, e, sparse_planes=mask, n_elems=n, d_out=d_out, indexes=indexes)
    return ctx.compress_planes_sparse(d_new, e, sparse_planes=mask, n_elems=n, d_out=d_out, indexes=indexes)


def decode_sparse(ctx, form, streams, sizes, codes, d_base, chosen, n_vals, n, e, indexes, d_out):
    if form == "delta":
        return ctx.decode_planes_sparse_delta(streams, sizes, codes, d_base, chosen, n_vals, n, e, indexes=indexes, d_out=d_out, cap=n * e)
    return ctx.decode_planes_sparse(streams, sizes, codes, chosen, n_vals, n, e, indexes=indexes, d_out=d_out, cap=n * e)


def round_trip_checked(ctx, torch, form, new, d_base, streams, sizes, codes, chosen, n_vals, n, e, indexes, what):
    for inplace in (False, True) if form == "delta" else (False,):
        buf = tpd.preloaded(torch, d_base) if inplace else guarded(torch, n * e)
        base = buf[PAD : PAD + n * e] if inplace else d_base
        _, nbytes = decode_sparse(ctx, form, streams, sizes, codes, base, chosen, n_vals, n, e, indexes, buf[PAD:])
        ctx.sync()
        assert int(nbytes.item()) == n * e, (what, inplace)
        assert np.array_equal(buf[PAD : PAD + n * e].cpu().numpy(), new), (what, inplace)
        assert guards_intact(buf, n * e), (what, inplace)


@pytest.mark.parametrize("which", ["none", "all", "alternating"])
@pytest.mark.parametrize("n", COMPRESS_N)
@pytest.mark.parametrize("e", WIDTHS)
@pytest.mark.parametrize("form", ["plain", "delta"])
def test_every_slot_is_the_oracle_s_image_and_round_trips_three_ways(env, form, e, n, which):
    ghf, ctx, torch = env
    mask = masks_for(e)[which]
    new, base, src, images, tables, n_vals = want_for(form, e, n, mask)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    r = compress_sparse(ghf, ctx, torch, form, d_new, d_base, e, n, mask)
    ctx.sync()
    assert r["sparse_planes"] == mask and r["n_vals"] == n_vals
    slot = r["slot_bytes"]
    assert slot == ghf.planes_slot_bytes(n)
    h_out, sizes, h_codes = r["out"].cpu().numpy(), [int(v) for v in r["out_bytes"].cpu().numpy()], r["codes"].cpu().numpy()
    idx = r["indexes"]
    for j in range(2 * e):
        if images[j] is None:  # an empty slot reports 0, is unwritten and has no side-car
            assert sizes[j] == 0 and (h_out[j * slot : (j + 1) * slot] == GUARD).all(), j
            assert not idx[j].d_chunk_bit and not idx[j].d_seg_bit and idx[j].n_symbols == 0, j
            continue
        assert sizes[j] == images[j].size, (j, sizes[j], images[j].size)
        assert np.array_equal(h_out[j * slot :][: sizes[j]], images[j]), j
        assert ghf.Code.from_buffer_copy(h_codes[j].tobytes()).as_dict() == tables[j], j
        stream_symbols = n if not (mask >> (j % e)) & 1 else ghf.sparse_mask_bytes(n) if j < e else n_vals[j - e]
        assert idx[j].n_symbols == stream_symbols, j
    assert torch.equal(d_new, to_dev(torch, new)) and torch.equal(d_base, to_dev(torch, base))  # the inputs are only read
    if mask == 0:  # nothing sparse: the dense call's slots, sizes and codes
        dense = ctx.compress_planes_delta(d_new, d_base, e, n_elems=n, flags=ghf.PLANES_BUILD_CODES) if form == "delta" \
            else ctx.compress_planes_coded(d_new, e, n_elems=n, flags=ghf.PLANES_BUILD_CODES)
        ctx.sync()
        d_sizes = [int(v) for v in dense["out_bytes"].cpu().numpy()]
        assert d_sizes == sizes[:e] and np.array_equal(dense["codes"].cpu().numpy(), h_codes[:e])
        h_dense = dense["out"].cpu().numpy()
        for p in range(e):
            assert np.array_equal(h_dense[p * slot :][: sizes[p]], h_out[p * slot :][: sizes[p]]), p
    slots = [r["out"][j * slot : (j + 1) * slot] for j in range(2 * e)]
    round_trip_checked(ctx, torch, form, new, d_base, slots, sizes, r["codes"], mask, n_vals, n, e, idx, "side-cars")
    round_trip_checked(ctx, torch, form, new, d_base, slots, sizes, r["codes"], mask, n_vals, n, e, None, "without side-cars")
    # from files: images the oracle alone made, codes from their own headers; empty slots carry nothing at all
    f_slots = [None if im is None else to_dev(torch, im) for im in images]
    f_sizes = [0 if im is None else im.size for im in images]
    f_codes = torch.stack([ctx.new_code() if im is None else ctx.code_to_device(ghf.parse_header(im)[0]) for im in images]).contiguous()
    round_trip_checked(ctx, torch, form, new, d_base, f_slots, f_sizes, f_codes, mask, n_vals, n, e, None, "files")
    ctx.planes_index_free(idx)


# ---------------------------------------------------------------- 3. a damaged sparse plane
@pytest.mark.parametrize("e", WIDTHS)
def test_a_mask_with_one_bit_too_many_leaves_the_output_alone_and_in_place_the_base(env, e):
    """the top plane of the delta, stored sparse: its mask image is rebuilt by the oracle with one more bit set, its values image
    is the true one.  Every stream decodes to the size it should, the merge of the plane counts one bit more than there are
    values: GHF_E_CORRUPT from ghf_sync, and the merge into d_out stores nothing."""
    ghf, ctx, torch = env
    n, mask = 65536 + 3, masks_for(e)["all"]
    new, base, src, images, tables, n_vals = want_for("delta", e, n, mask)
    p = e - 1
    plane = tpd.planes_of(src, e)[p]
    assert 0 < n_vals[p] < n
    m, _ = sparse_form(plane)
    k = int(np.flatnonzero(plane == 0)[n // 3])
    m = m.copy()
    m[k >> 3] |= 1 << (k & 7)
    bad_images = list(images)
    bad_images[p] = orc.compress(m)
    d_base = to_dev(torch, base)
    streams = [None if im is None else to_dev(torch, im) for im in bad_images]
    sizes = [0 if im is None else im.size for im in bad_images]
    codes = torch.stack([ctx.new_code() if im is None else ctx.code_to_device(ghf.parse_header(im)[0]) for im in bad_images]).contiguous()
    buf = guarded(torch, n * e)
    decode_sparse(ctx, "delta", streams, sizes, codes, d_base, mask, n_vals, n, e, None, buf[PAD:])
    assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
    assert untouched(torch, buf)
    assert ctx.L.ghf_clear_status(ctx.h) == OK
    buf = tpd.preloaded(torch, d_base)
    decode_sparse(ctx, "delta", streams, sizes, codes, buf[PAD : PAD + n * e], mask, n_vals, n, e, None, buf[PAD:])
    assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
    assert np.array_equal(buf[PAD : PAD + n * e].cpu().numpy(), base) and guards_intact(buf, n * e)
    assert ctx.L.ghf_clear_status(ctx.h) == OK
    streams[p] = to_dev(torch, images[p])  # the true mask: the context works again
    sizes[p] = images[p].size
    codes[p] = ctx.code_to_device(ghf.parse_header(images[p])[0])
    round_trip_checked(ctx, torch, "delta", new, d_base, streams, sizes, codes, mask, n_vals, n, e, None, "the true mask")


# ---------------------------------------------------------------- 4. sizes
def oracle_sizes(delta, e, n):
    """(the 3/4 rule in numpy, stored bytes under it, stored bytes with every plane dense), from the oracle alone"""
    rule, sparse, dense = 0, 0, 0
    for p, pl in enumerate(tpd.planes_of(delta, e)):
        d = orc.compress(pl).size
        dense += d
        if n - np.count_nonzero(pl) >= n - n // 4:
            rule |= 1 << p
            m, v = sparse_form(pl)
            s = orc.compress(m).size + (orc.compress(v).size if v.size else 0)
            assert s <= d, (p, s, d)  # no plane the rule chooses comes out larger than its dense image
            sparse += s
        else:
            sparse += d
    return rule, sparse, dense


# (dense, sparse where >= 3/4 zero) bytes at n = 65536, seed 7: recomputed from the oracle below, pinned here beside it
PINNED = {(2, 1e-3): (27886, 21903), (2, 1e-5): (18742, 6775), (4, 1e-3): (160497, 154514), (4, 1e-5): (112187, 100220),
          (8, 1e-3): (407197, 397141), (8, 1e-5): (359308, 343897)}


@pytest.mark.parametrize("step", [1e-3, 1e-5])
@pytest.mark.parametrize("e", WIDTHS)
def test_auto_follows_the_rule_and_stores_less_than_the_dense_planes(env, e, step):
    ghf, ctx, torch = env
    n = 65536
    new, base = stepped(n, e, step)
    if step == 1e-3:
        assert np.array_equal(new, tpd.stepped(n, e)[0]) and np.array_equal(base, tpd.stepped(n, e)[1])  # the recipe of that file
    rule, sparse, dense = oracle_sizes(new ^ base, e, n)
    print("E = %d, step %g: dense %d bytes, sparse where >= 3/4 zero (planes 0x%x) %d bytes, ratio %.3f" % (e, step, dense, rule, sparse, sparse / dense))
    assert (dense, sparse) == PINNED[(e, step)]
    assert sparse < dense
    r = compress_sparse(ghf, ctx, torch, "delta", to_dev(torch, new), to_dev(torch, base), e, n, ghf.SPARSE_AUTO, indexes=False)
    ctx.sync()
    assert r["sparse_planes"] == rule
    assert int(r["out_bytes"].sum().item()) == sparse


def test_a_frozen_layer_stores_a_mask_per_plane_and_no_values(env):
    """new == base at 65536 elements: every plane is all zeros, so every plane is sparse and every values slot is empty; 2073
    bytes per plane (a header and one bit per mask byte) against 9241 dense.  Both are recomputed from the oracle."""
    ghf, ctx, torch = env
    n = 65536
    per_sparse = orc.compress(np.zeros(ghf.sparse_mask_bytes(n), dtype=np.uint8)).size
    per_dense = orc.compress(np.zeros(n, dtype=np.uint8)).size
    assert (per_sparse, per_dense) == (2073, 9241)
    for e in WIDTHS:
        new = tpd.stepped(n, e)[0]
        d_new = to_dev(torch, new)
        r = compress_sparse(ghf, ctx, torch, "delta", d_new, d_new.clone(), e, n, ghf.SPARSE_AUTO)
        ctx.sync()
        assert r["sparse_planes"] == (1 << e) - 1 and r["n_vals"] == [0] * e
        assert [int(v) for v in r["out_bytes"].cpu().numpy()] == [per_sparse] * e + [0] * e
        slot = r["slot_bytes"]
        assert bool((r["out"][e * slot :] == GUARD).all().item())
        slots = [r["out"][j * slot : (j + 1) * slot] for j in range(e)] + [None] * e
        round_trip_checked(ctx, torch, "delta", new, d_new, slots, [per_sparse] * e + [0] * e, r["codes"], r["sparse_planes"],
                           r["n_vals"], n, e, r["indexes"], "frozen")
        ctx.planes_index_free(r["indexes"])


# ---------------------------------------------------------------- 5. refusals on a live context; it stays usable after each
def test_call_level_refusals_come_back_at_once_and_leave_the_context_usable(env):
    ghf, ctx, torch = env
    L = ctx.L
    e, n = 4, 4097
    mask = 0b1100
    new, base, src, images, tables, n_vals = want_for("delta", e, n, mask)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    good = compress_sparse(ghf, ctx, torch, "delta", d_new, d_base, e, n, mask)
    ctx.sync()
    slot = good["slot_bytes"]
    sizes = [int(v) for v in good["out_bytes"].cpu().numpy()]
    vp, sz = C.c_void_p, C.c_size_t
    ptrs = (vp * (2 * e))(*[good["out"][j * slot :].data_ptr() for j in range(2 * e)])
    h_sizes = (sz * (2 * e))(*sizes)
    h_n_vals = (sz * e)(*n_vals)
    idx = good["indexes"]
    bad_idx = (ghf.Index * (2 * e))()
    C.memmove(bad_idx, idx, C.sizeof(bad_idx))
    assert n_vals[2] > 0
    bad_idx[e + 2].n_symbols += 1  # the values of plane 2
    dense_idx = (ghf.Index * (2 * e))()  # every mask's side-car as if the plane were dense
    C.memmove(dense_idx, idx, C.sizeof(dense_idx))
    dense_idx[2].n_symbols = n
    g_out = torch.full((2 * e * slot + 64,), GUARD, dtype=torch.uint8, device="cuda")
    g_bytes = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    g_small = torch.full((PAD + n + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    codes = good["codes"].data_ptr()
    chosen, out_vals = C.c_uint(0), (sz * e)()
    inp, bas, out = d_new.data_ptr(), d_base.data_ptr(), g_out.data_ptr()
    small = g_small[PAD:].data_ptr()
    AUTO = ghf.SPARSE_AUTO

    def compress(d_in=inp, d_b=bas, n_=n, e_=e, m=mask, d_o=out, slot_=slot, d_nb=g_bytes.data_ptr(), d_c=codes, ch=C.byref(chosen), nv=out_vals):
        return L.ghf_compress_planes_sparse_delta(ctx.h, d_in, d_b, n_, e_, m, d_o, slot_, d_nb, d_c, None, ch, nv)

    def decode(p=ptrs, s=h_sizes, d_c=codes, ix=idx, d_b=bas, m=mask, nv=h_n_vals, n_=n, e_=e, d_o=out, cap=n * e):
        return L.ghf_decode_planes_sparse_delta(ctx.h, p, s, d_c, ix, d_b, m, nv, n_, e_, d_o, cap, g_bytes.data_ptr())

    null_ptrs = (vp * (2 * e))(*[None if j == 1 else ptrs[j] for j in range(2 * e)])
    odd_ptrs = (vp * (2 * e))(*[ptrs[j] + 8 if j == e + 2 else ptrs[j] for j in range(2 * e)])
    cases = [
        (E_INVAL, lambda: compress(m=1 << e)),  # a bit at elem_bytes
        (E_INVAL, lambda: compress(m=1 << 8)),
        (E_INVAL, lambda: compress(m=AUTO | 1)),  # AUTO together with an explicit bit
        (E_INVAL, lambda: decode(m=AUTO)),  # the decode is told what was chosen
        (E_INVAL, lambda: decode(m=1 << e)),
        (E_INVAL, lambda: decode(ix=bad_idx)),  # an index of another size
        (E_INVAL, lambda: decode(ix=dense_idx)),
        (E_INVAL, lambda: compress(e_=3)),
        (E_INVAL, lambda: decode(e_=16)),
        (E_EMPTY, lambda: compress(n_=0)),
        (E_EMPTY, lambda: decode(n_=0, ix=None, nv=(sz * e)())),
        (E_CAP, lambda: compress(slot_=slot - 16)),
        (E_CAP, lambda: decode(cap=n * e - 1)),
        (E_INVAL, lambda: compress(d_in=None)),
        (E_INVAL, lambda: compress(d_b=None)),
        (E_INVAL, lambda: compress(d_o=None)),
        (E_INVAL, lambda: compress(d_nb=None)),
        (E_INVAL, lambda: compress(ch=None)),
        (E_INVAL, lambda: compress(nv=None)),
        (E_INVAL, lambda: compress(d_in=inp + 8)),
        (E_INVAL, lambda: compress(d_b=bas + 8)),
        (E_INVAL, lambda: compress(d_o=out + 8)),
        (E_INVAL, lambda: compress(d_c=codes + 8)),
        (E_INVAL, lambda: compress(slot_=slot + 8)),
        (E_INVAL, lambda: decode(p=None)),
        (E_INVAL, lambda: decode(s=None)),
        (E_INVAL, lambda: decode(d_c=None)),
        (E_INVAL, lambda: decode(d_b=None)),
        (E_INVAL, lambda: decode(nv=None)),
        (E_INVAL, lambda: decode(d_o=None)),
        (E_INVAL, lambda: decode(p=null_ptrs)),
        (E_INVAL, lambda: decode(p=odd_ptrs)),
        (E_INVAL, lambda: decode(d_b=bas + 8)),
        (E_INVAL, lambda: decode(d_o=out + 8)),
        (E_INVAL, lambda: L.ghf_sparse_split(ctx.h, None, n, small, out, n, g_bytes.data_ptr())),
        (E_INVAL, lambda: L.ghf_sparse_split(ctx.h, inp, n, None, out, n, g_bytes.data_ptr())),
        (E_INVAL, lambda: L.ghf_sparse_split(ctx.h, inp, n, small, None, n, g_bytes.data_ptr())),
        (E_INVAL, lambda: L.ghf_sparse_split(ctx.h, inp, n, small, out, n, None)),
        (E_INVAL, lambda: L.ghf_sparse_split(ctx.h, inp + 8, n, small, out, n, g_bytes.data_ptr())),
        (E_INVAL, lambda: L.ghf_sparse_split(ctx.h, inp, n, small + 8, out, n, g_bytes.data_ptr())),
        (E_INVAL, lambda: L.ghf_sparse_split(ctx.h, inp, n, small, out + 8, n, g_bytes.data_ptr())),
        (E_EMPTY, lambda: L.ghf_sparse_split(ctx.h, inp, 0, small, out, n, g_bytes.data_ptr())),
        (E_INVAL, lambda: L.ghf_sparse_merge(ctx.h, None, bas, 5, n, out)),
        (E_INVAL, lambda: L.ghf_sparse_merge(ctx.h, inp, None, 5, n, out)),
        (E_INVAL, lambda: L.ghf_sparse_merge(ctx.h, inp, bas, 5, n, None)),
        (E_INVAL, lambda: L.ghf_sparse_merge(ctx.h, inp + 8, bas, 5, n, out)),
        (E_INVAL, lambda: L.ghf_sparse_merge(ctx.h, inp, bas + 8, 5, n, out)),
        (E_INVAL, lambda: L.ghf_sparse_merge(ctx.h, inp, bas, 5, n, out + 8)),
        (E_EMPTY, lambda: L.ghf_sparse_merge(ctx.h, inp, bas, 0, 0, out)),
    ]
    for k, (want, call) in enumerate(cases):
        assert call() == want, k
        torch.cuda.synchronize()
        assert bool((g_out == GUARD).all().item()) and bool((g_small == GUARD).all().item()), k
        assert bool((g_bytes == -1).all().item()), k
        assert L.ghf_sync(ctx.h) == OK, k  # nothing latched either
    slots = [good["out"][j * slot : (j + 1) * slot] for j in range(2 * e)]
    round_trip_checked(ctx, torch, "delta", new, d_base, slots, sizes, good["codes"], mask, n_vals, n, e, idx, "after the refusals")
    ctx.planes_index_free(idx)
