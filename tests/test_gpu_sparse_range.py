"""GPU: an element range of zero-suppressed byte planes (ghf_sparse_rank_pack / ghf_sparse_merge_at /
ghf_compress_planes_sparse_ranked[_delta] / ghf_decode_planes_sparse_range[_delta]).

Expected values come from numpy alone: the rank table and the plan from tests/sparse_range_model.py, the output from the
slice of the tensor.  Every output sits between guard bytes.  The pairs of tensors are those of tests/test_gpu_sparse.py
(the recipe of section 19 at steps of 1e-3 and 1e-5) and an identical pair."""
import ctypes as C

import numpy as np
import pytest

import pkgload
import sparse_range_model as model
import test_gpu_planes_delta as tpd
import test_gpu_sparse as tgs

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT = 0, 1, 3, 5, 6, 7
GUARD, PAD = tgs.GUARD, tgs.PAD
WIDTHS = (2, 4, 8)
R = model.RANK_ELEMS
N = 3 * R + 4099
guarded, guarded_with, guards_intact, untouched, to_dev = tgs.guarded, tgs.guarded_with, tgs.guards_intact, tgs.untouched, tgs.to_dev


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    assert pkg.ghf.SPARSE_RANK_ELEMS == R
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def byte_string(n, density=0.25, seed=3):
    rng = np.random.default_rng(seed + n % 1000)
    x = rng.integers(1, 256, n, dtype=np.uint8)
    x[rng.random(n) >= density] = 0
    return x


# ---------------------------------------------------------------- 1. the rank table
# 1 .. 8: a mask of one byte; R - 1 .. R + 1: one rank block and its neighbours; N: four blocks, the last ragged; the last size:
# 4099 tiles and a ragged one, so that a workgroup's slab has two tiles and rank blocks straddle slabs
PACK_N = (1, 7, 8, R - 1, R, R + 1, N, (16 << 20) + 3 * R + 5)


@pytest.mark.parametrize("n", PACK_N)
def test_rank_pack_writes_the_model_s_table_between_guard_bytes(env, n):
    ghf, ctx, torch = env
    for density in (0.25, 1.0) if n <= N else (0.25,):
        x = byte_string(n, density)
        if n > R:
            x[R : R + R // 2] = 0  # a stretch without values inside a block
        mask, _ = model.sparse_form(x)
        want = ghf.sparse_rank_table(x)
        if n <= N:
            assert np.array_equal(want, model.table_of(x))
        m_buf, d_mask = guarded_with(torch, mask)
        size = ghf.sparse_rank_bytes(n)
        assert size == want.size
        buf = guarded(torch, size)
        ctx.sparse_rank_pack(d_mask, n, d_table=buf[PAD:], cap=size)
        ctx.sync()
        got = buf[PAD : PAD + size].cpu().numpy()
        assert np.array_equal(got, want), (n, density, model.cum_in(got)[:6], model.cum_in(want)[:6])
        assert guards_intact(buf, size) and guards_intact(m_buf, mask.size)
        info = ghf.sparse_rank_parse(got)
        assert (info.n, info.n_vals, info.n_blocks) == (n, np.count_nonzero(x), model.rank_blocks(n))


def test_rank_pack_refusals_and_a_set_pad_bit(env):
    ghf, ctx, torch = env
    n = R + 5
    mask, _ = model.sparse_form(byte_string(n))
    d_mask = to_dev(torch, mask)
    size = ghf.sparse_rank_bytes(n)
    buf = guarded(torch, size)
    L, h = ctx.L, ctx.h
    assert L.ghf_sparse_rank_pack(h, d_mask.data_ptr(), n, buf[PAD:].data_ptr(), size - 1) == E_CAP
    assert L.ghf_sparse_rank_pack(h, d_mask.data_ptr(), n, buf[PAD:].data_ptr(), 64) == E_CAP
    assert L.ghf_sparse_rank_pack(h, d_mask.data_ptr(), 0, buf[PAD:].data_ptr(), size) == E_EMPTY
    assert L.ghf_sparse_rank_pack(h, None, n, buf[PAD:].data_ptr(), size) == E_INVAL
    assert L.ghf_sparse_rank_pack(h, d_mask.data_ptr(), n, None, size) == E_INVAL
    assert L.ghf_sparse_rank_pack(h, d_mask.data_ptr(), n, buf[PAD + 8 :].data_ptr(), size) == E_INVAL
    assert L.ghf_sync(h) == OK and untouched(torch, buf)
    bad = mask.copy()
    bad[-1] |= 0x80  # a pad bit: the mask is not one of a string of n bytes
    ctx.sparse_rank_pack(to_dev(torch, bad), n, d_table=buf[PAD:], cap=size)
    assert L.ghf_sync(h) == E_CORRUPT and untouched(torch, buf)
    assert L.ghf_clear_status(h) == OK


# ---------------------------------------------------------------- 2. values that start anywhere
SKIPS = (0, 1, 15, 16, 4095)
# one tile and its neighbours, a slab of whole tiles and a ragged one, and more tiles than workgroups
AT_N = (1, 17, 4095, 4096, 4097, 3 * 4096 + 5, (tgs.G + 1) * 4096 + 5)


@pytest.mark.parametrize("skip", SKIPS)
def test_merge_at_is_exact_between_guard_bytes(env, skip):
    ghf, ctx, torch = env
    rng = np.random.default_rng(skip)
    for n in AT_N:
        for density in (0.02, 1.0) if n < 100000 else (0.3,):
            x = byte_string(n, density, seed=skip)
            mask, vals = model.sparse_form(x)
            # the values stand behind `skip` bytes that are not theirs and in front of a guard that is not theirs either
            held = np.concatenate([rng.integers(1, 256, skip, dtype=np.uint8), vals])
            v_buf, d_vals = guarded_with(torch, held)
            m_buf, d_mask = guarded_with(torch, mask)
            buf = guarded(torch, n)
            ctx.sparse_merge_at(d_mask, d_vals, skip, vals.size, n, d_out=buf[PAD:])
            ctx.sync()
            assert np.array_equal(buf[PAD : PAD + n].cpu().numpy(), x), (n, density, skip)
            assert guards_intact(buf, n) and guards_intact(v_buf, held.size) and guards_intact(m_buf, mask.size)
    if skip == 0:  # skip = 0 is ghf_sparse_merge: the same bytes from both calls, on a string of its own
        n0 = 3 * 4096 + 5
        x0 = byte_string(n0, 0.3, seed=1)
        mask0, vals0 = model.sparse_form(x0)
        d_mask0, d_vals0 = to_dev(torch, mask0), to_dev(torch, vals0)
        a = ctx.sparse_merge(d_mask0, d_vals0, vals0.size, n0)
        b = ctx.sparse_merge_at(d_mask0, d_vals0, 0, vals0.size, n0)
        ctx.sync()
        assert np.array_equal(a.cpu().numpy(), x0) and torch.equal(a, b)


def test_merge_at_with_a_wrong_n_vals_stores_nothing(env):
    ghf, ctx, torch = env
    n = 3 * 4096 + 5
    x = byte_string(n)
    mask, vals = model.sparse_form(x)
    held = np.concatenate([np.full(15, 7, np.uint8), vals, np.full(16, 9, np.uint8)])
    d_vals, d_mask = to_dev(torch, held), to_dev(torch, mask)
    for wrong in (vals.size - 1, vals.size + 1, 0):
        buf = guarded(torch, n)
        ctx.sparse_merge_at(d_mask, d_vals, 15, wrong, n, d_out=buf[PAD:])
        assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT and untouched(torch, buf), wrong
        assert ctx.L.ghf_clear_status(ctx.h) == OK
    L, h = ctx.L, ctx.h
    buf = guarded(torch, n)
    out = buf[PAD:].data_ptr()
    assert L.ghf_sparse_merge_at(h, d_mask.data_ptr(), d_vals.data_ptr(), 15, vals.size, 0, out) == E_EMPTY
    assert L.ghf_sparse_merge_at(h, d_mask.data_ptr(), None, 15, vals.size, n, out) == E_INVAL
    assert L.ghf_sparse_merge_at(h, d_mask.data_ptr(), d_vals[1:].data_ptr(), 15, vals.size, n, out) == E_INVAL
    assert L.ghf_sparse_merge_at(h, d_mask.data_ptr(), d_vals.data_ptr(), 2**64 - 1, vals.size, n, out) == E_INVAL
    assert L.ghf_sync(h) == OK and untouched(torch, buf)
    ctx.sparse_merge_at(d_mask, d_vals, 15, vals.size, n, d_out=buf[PAD:])  # the context works again
    ctx.sync()
    assert np.array_equal(buf[PAD : PAD + n].cpu().numpy(), x)


# ---------------------------------------------------------------- 3. the pairs, compressed once per case
def pair(e, step):
    """(new, base) as bytes: the pairs of section 19 at a step, or an identical pair (step None: every n_vals is 0)"""
    if step is None:
        base = tgs.stepped(N, e, 1e-3)[1]
        return base.copy(), base
    return tgs.stepped(N, e, step)


_stored = {}


def stored(env, e, step, form, mask):
    """the tensor compressed by the ranked call, with everything a range decode needs, from side-cars and from seek tables"""
    ghf, ctx, torch = env
    key = (e, step, form, mask)
    if key in _stored:
        return _stored[key]
    new, base = pair(e, step)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    rslot = (ghf.sparse_rank_bytes(N) + 15) & ~15
    d_ranks = torch.full((e * rslot,), GUARD, dtype=torch.uint8, device="cuda")
    kw = dict(sparse_planes=mask, n_elems=N, indexes=True, d_ranks=d_ranks, rank_slot_bytes=rslot)
    r = ctx.compress_planes_sparse_ranked_delta(d_new, d_base, e, **kw) if form == "delta" else ctx.compress_planes_sparse_ranked(d_new, e, **kw)
    ctx.sync()
    slot, sizes, chosen = r["slot_bytes"], [int(v) for v in r["out_bytes"].cpu().numpy()], r["sparse_planes"]
    slots = [r["out"][j * slot : (j + 1) * slot] if sizes[j] else None for j in range(2 * e)]
    h_ranks = d_ranks.cpu().numpy()
    ranks = []
    for p in range(e):
        t = h_ranks[p * rslot : p * rslot + ghf.sparse_rank_bytes(N)].copy()
        ranks.append((ghf.sparse_rank_parse(t), t) if (chosen >> p) & 1 else None)
    d_tables = [None if s is None else ctx.seek_pack(r["indexes"][j]) for j, s in enumerate(slots)]
    ctx.sync()
    infos = [None if t is None else ghf.seek_parse(t.cpu().numpy()) for t in d_tables]
    _stored[key] = dict(new=new, base=base, d_base=d_base, r=r, slots=slots, sizes=sizes, chosen=chosen, ranks=ranks, h_ranks=h_ranks,
                        rslot=rslot, d_tables=d_tables, infos=infos)
    return _stored[key]


def masks_for(e):
    return {"auto": None, "none": 0, "top": 1 << (e - 1), "all": (1 << e) - 1}


@pytest.mark.parametrize("step", [1e-3, 1e-5, None])
@pytest.mark.parametrize("e", WIDTHS)
@pytest.mark.parametrize("form", ["plain", "delta"])
def test_the_ranked_compress_is_the_sparse_compress_plus_the_model_s_tables(env, form, e, step):
    ghf, ctx, torch = env
    new, base = pair(e, step)
    src = new ^ base if form == "delta" else new
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    for mask in (ghf.SPARSE_AUTO, masks_for(e)["all"]):
        s = stored(env, e, step, form, mask)
        r = s["r"]
        plain = tgs.compress_sparse(ghf, ctx, torch, form, d_new, d_base, e, N, mask)
        ctx.sync()
        assert plain["sparse_planes"] == r["sparse_planes"] and plain["n_vals"] == r["n_vals"]
        assert torch.equal(plain["out_bytes"], r["out_bytes"]) and torch.equal(plain["codes"], r["codes"])
        slot = r["slot_bytes"]
        a, b = plain["out"].cpu().numpy(), r["out"].cpu().numpy()
        for j, size in enumerate(s["sizes"]):
            assert np.array_equal(a[j * slot :][:size], b[j * slot :][:size]), j
            assert plain["indexes"][j].n_symbols == r["indexes"][j].n_symbols, j
        for p, plane in enumerate(tpd.planes_of(src, e)):
            got = s["h_ranks"][p * s["rslot"] : (p + 1) * s["rslot"]]
            if (s["chosen"] >> p) & 1:
                want = model.table_of(plane)
                assert np.array_equal(got[: want.size], want) and (got[want.size :] == GUARD).all(), p
                assert s["ranks"][p][0].n_vals == r["n_vals"][p]
            else:
                assert (got == GUARD).all(), p  # the slot of a dense plane stays unwritten
        ctx.planes_index_free(plain["indexes"])
        if step is None:
            assert s["chosen"] == (1 << e) - 1 or form == "plain"
    if form == "delta" and step is None:
        assert r["n_vals"] == [0] * e


def test_the_ranked_compress_refuses_a_bad_rank_output(env):
    ghf, ctx, torch = env
    e = 2
    new, base = pair(e, 1e-5)
    d_new, d_base = to_dev(torch, new), to_dev(torch, base)
    slot, rslot = ghf.planes_slot_bytes(N), (ghf.sparse_rank_bytes(N) + 15) & ~15
    d_out, d_bytes = ctx.empty_u8(2 * e * slot), torch.zeros(2 * e, dtype=torch.int64, device="cuda")
    d_ranks = guarded(torch, e * rslot)
    chosen, n_vals = C.c_uint(0), (C.c_size_t * e)()

    def call(ranks, rs, delta):
        front = (ctx.h, d_new.data_ptr()) + ((d_base.data_ptr(),) if delta else ())
        f = ctx.L.ghf_compress_planes_sparse_ranked_delta if delta else ctx.L.ghf_compress_planes_sparse_ranked
        return f(*front, N, e, 3, d_out.data_ptr(), slot, d_bytes.data_ptr(), None, None, C.byref(chosen), n_vals, ranks, rs)

    ok = d_ranks[PAD:].data_ptr()
    for delta in (False, True):
        assert call(None, rslot, delta) == E_INVAL
        assert call(ok + 8, rslot, delta) == E_INVAL
        assert call(ok, rslot + 8, delta) == E_INVAL
        assert call(ok, rslot - 16, delta) == E_CAP
        assert call(ok, 0, delta) == E_CAP
    assert ctx.L.ghf_sync(ctx.h) == OK and untouched(torch, d_ranks)
    assert call(ok, rslot, True) == OK
    ctx.sync()
    assert guards_intact(d_ranks, e * rslot)


# ---------------------------------------------------------------- 4. the range calls
# the whole range; the range that ends at n; count = 1 (at the start, behind a block boundary, at the end); ranges inside one
# block (the first, a middle one); across a block boundary with first % 16 != 0; across two boundaries; a range that begins on
# a boundary and one that ends on one
RANGES = ((0, N), (R + 4097, N - R - 4097), (0, 1), (R, 1), (N - 1, 1), (7, 9), (R + 15, 4097), (R - 9, 4097), (4095, 2 * R), (2 * R, 4099),
          (32769, R - 1))
assert all(f + c <= N for f, c in RANGES) and any(f % 16 and f // R != (f + c - 1) // R for f, c in RANGES)


def decode_range(ctx, s, form, e, first, count, source, d_base, d_out, mask=None, ranks=None):
    kw = dict(indexes=s["r"]["indexes"]) if source == "side-cars" else dict(infos=s["infos"], d_tables=s["d_tables"])
    mask = s["chosen"] if mask is None else mask
    ranks = s["ranks"] if ranks is None else ranks
    if form == "delta":
        return ctx.decode_planes_sparse_range_delta(s["slots"], s["sizes"], s["r"]["codes"], d_base, mask, ranks, N, e, first, count,
                                                    d_out=d_out, cap=count * e, **kw)
    return ctx.decode_planes_sparse_range(s["slots"], s["sizes"], s["r"]["codes"], mask, ranks, N, e, first, count, d_out=d_out,
                                          cap=count * e, **kw)


@pytest.mark.parametrize("which", ["auto", "none", "top", "all"])
@pytest.mark.parametrize("step", [1e-3, 1e-5, None])
@pytest.mark.parametrize("e", WIDTHS)
def test_every_range_is_the_slice_from_both_sources_plain_delta_and_in_place(env, e, step, which):
    ghf, ctx, torch = env
    mask = masks_for(e)[which]
    mask = ghf.SPARSE_AUTO if mask is None else mask
    if which == "auto" and step == 1e-3:
        ranges = RANGES
    else:  # thinned: the whole range, the one that ends at n, count = 1, inside a block, across a boundary at an odd first
        ranges = ((0, N), (R + 4097, N - R - 4097), (N - 1, 1), (7, 9), (R - 9, 4097))
    for form in ("plain", "delta"):
        s = stored(env, e, step, form, mask)
        if which == "all":
            assert s["chosen"] == (1 << e) - 1
        if which == "none":
            assert s["chosen"] == 0 and s["ranks"] == [None] * e
        for first, count in ranges:
            want = s["new"][first * e : (first + count) * e]
            d_shard = s["d_base"][first * e : (first + count) * e].clone()  # the caller's shard of the base (16-byte aligned: a fresh tensor)
            for source in ("side-cars", "tables"):
                for inplace in (False, True) if form == "delta" else (False,):
                    buf = tpd.preloaded(torch, d_shard) if inplace else guarded(torch, count * e)
                    base = buf[PAD : PAD + count * e] if inplace else d_shard
                    decode_range(ctx, s, form, e, first, count, source, base, buf[PAD:])
                    ctx.sync()
                    what = (form, first, count, source, inplace, hex(s["chosen"]))
                    assert np.array_equal(buf[PAD : PAD + count * e].cpu().numpy(), want), what
                    assert guards_intact(buf, count * e), what
            if s["chosen"] == 0:  # nothing sparse: the call of section 17 on the same images
                slots, sizes = s["slots"][:e], s["sizes"][:e]
                for kw in (dict(indexes=s["r"]["indexes"]), dict(infos=s["infos"][:e], d_tables=s["d_tables"][:e])):
                    if form == "delta":
                        ref = ctx.decode_planes_range_delta(slots, sizes, s["r"]["codes"], d_shard, e, first, count, **kw)
                    else:
                        ref = ctx.decode_planes_range(slots, sizes, s["r"]["codes"], e, first, count, **kw)
                    ctx.sync()
                    assert np.array_equal(ref[: count * e].cpu().numpy(), want), (form, first, count)


def test_count_zero_queues_nothing(env):
    ghf, ctx, torch = env
    s = stored(env, 2, 1e-5, "delta", ghf.SPARSE_AUTO)
    buf = guarded(torch, 64)
    for source in ("side-cars", "tables"):
        for first in (0, 5, N):
            decode_range(ctx, s, "delta", 2, first, 0, source, s["d_base"], buf[PAD:])
    ctx.sync()
    assert untouched(torch, buf)


# ---------------------------------------------------------------- 5. a damaged rank table
@pytest.mark.parametrize("source", ["side-cars", "tables"])
@pytest.mark.parametrize("e", WIDTHS)
def test_a_rank_table_with_one_entry_raised_passes_the_parse_and_fails_the_merge(env, e, source):
    """cum[1] of a sparse plane, raised by one: still monotone, still within a block's elements, so the parse accepts
    it.  A range that reads it as v_lo or v_hi gives the sparse merge a count its mask does not have: GHF_E_CORRUPT from
    ghf_sync, nothing in d_out; in place, d_out keeps the base.  A range that reads neither entry is served."""
    ghf, ctx, torch = env
    s = stored(env, e, 1e-5, "delta", ghf.SPARSE_AUTO)
    p = max((q for q in range(e) if (s["chosen"] >> q) & 1), key=lambda q: s["ranks"][q][0].n_vals)  # the sparse plane with most values
    t = s["ranks"][p][1].copy()
    cum = model.cum_in(t).copy()
    assert cum[1] + 1 <= cum[2] and cum[1] + 1 <= R
    cum[1] += 1
    t[model.HEADER_BYTES :] = cum.astype("<u8").view(np.uint8)
    bad = list(s["ranks"])
    bad[p] = (ghf.sparse_rank_parse(t), t)  # the parse accepts it
    for first, count in ((5, 100), (R + 5, 100), (R - 9, 4097)):  # cum[1] as v_hi, as v_lo, and as neither (b0 = 0, b1 = 2)
        want = s["new"][first * e : (first + count) * e]
        d_shard = s["d_base"][first * e : (first + count) * e].clone()
        for inplace in (False, True):
            buf = tpd.preloaded(torch, d_shard) if inplace else guarded(torch, count * e)
            base = buf[PAD : PAD + count * e] if inplace else d_shard
            decode_range(ctx, s, "delta", e, first, count, source, base, buf[PAD:], ranks=bad)
            if first == R - 9:
                ctx.sync()
                assert np.array_equal(buf[PAD : PAD + count * e].cpu().numpy(), want)
                continue
            assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT, (first, inplace)
            assert ctx.L.ghf_clear_status(ctx.h) == OK
            if inplace:
                assert torch.equal(buf[PAD : PAD + count * e], d_shard) and guards_intact(buf, count * e)
            else:
                assert untouched(torch, buf)
    buf = guarded(torch, 100 * e)  # the true table: the context works again
    decode_range(ctx, s, "delta", e, 5, 100, source, s["d_base"][5 * e : 105 * e].clone(), buf[PAD:])
    ctx.sync()
    assert np.array_equal(buf[PAD : PAD + 100 * e].cpu().numpy(), s["new"][5 * e : 105 * e])


# ---------------------------------------------------------------- 6. call-level refusals
def test_call_level_refusals_come_back_at_once_and_leave_the_context_usable(env):
    ghf, ctx, torch = env
    e = 2
    s = stored(env, e, 1e-3, "delta", 3)  # both planes sparse, both with values
    assert s["chosen"] == 3 and all(r[0].n_vals for r in s["ranks"])
    first, count = R - 9, 4097
    d_shard = s["d_base"][first * e : (first + count) * e].clone()
    buf = guarded(torch, count * e)
    L, h = ctx.L, ctx.h
    slots = 2 * e

    def args(source):
        ptrs = (C.c_void_p * slots)(*[x.data_ptr() for x in s["slots"]])
        sizes = (C.c_size_t * slots)(*s["sizes"])
        idx = s["r"]["indexes"] if source == "side-cars" else None
        infos = t_ptrs = t_bytes = None
        if source == "tables":
            infos = (ghf.SeekInfo * slots)(*s["infos"])
            t_ptrs = (C.c_void_p * slots)(*[x.data_ptr() for x in s["d_tables"]])
            t_bytes = (C.c_size_t * slots)(*[ghf.seek_bytes(i.n_symbols) for i in s["infos"]])
        r_infos = (ghf.SparseRankInfo * e)(*[r[0] for r in s["ranks"]])
        r_ptrs = (C.c_void_p * e)(*[r[1].ctypes.data for r in s["ranks"]])
        return dict(ptrs=ptrs, sizes=sizes, codes=s["r"]["codes"].data_ptr(), idx=idx, infos=infos, t_ptrs=t_ptrs, t_bytes=t_bytes,
                    r_infos=r_infos, r_ptrs=r_ptrs, base=d_shard.data_ptr(), mask=s["chosen"], n=N, e=e, first=first, count=count,
                    out=buf[PAD:].data_ptr(), cap=count * e)

    def call(a, delta=True):
        front = (h, a["ptrs"], a["sizes"], a["codes"], a["idx"], a["infos"], a["t_ptrs"], a["t_bytes"], a["r_infos"], a["r_ptrs"])
        tail = (a["mask"], a["n"], a["e"], a["first"], a["count"], a["out"], a["cap"])
        if delta:
            return L.ghf_decode_planes_sparse_range_delta(*front, a["base"], *tail)
        return L.ghf_decode_planes_sparse_range(*front, *tail)

    def refused(source, want, **change):
        a = args(source)
        for k, v in change.items():
            if callable(v):
                v(a)
            else:
                a[k] = v
        for delta in (True, False):
            assert call(a, delta) == want, (source, change, delta)

    def setter(key, j, value, field=None):
        def f(a):
            if field is None:
                a[key][j] = value
            else:
                setattr(a[key][j], field, value)
        return f

    for source in ("side-cars", "tables"):
        # the refusals of ghf_decode_planes_range
        refused(source, E_INVAL, ptrs=None)
        refused(source, E_INVAL, sizes=None)
        refused(source, E_INVAL, codes=None)
        refused(source, E_INVAL, out=None)
        for bad_e in (0, 1, 3, 16):
            refused(source, E_INVAL, e=bad_e)
        refused(source, E_INVAL, idx=None, infos=None, t_ptrs=None, t_bytes=None)  # neither source
        refused(source, E_INVAL, x=setter("ptrs", 0, None))
        refused(source, E_INVAL, x=setter("ptrs", 1, s["slots"][1].data_ptr() + 8))
        refused(source, E_INVAL, out=buf[PAD + 8 :].data_ptr())
        refused(source, E_INVAL, first=N, count=1)
        refused(source, E_INVAL, first=1, count=N)
        refused(source, E_INVAL, first=2**64 - 1, count=2)
        refused(source, E_CAP, cap=count * e - 1)
        # ... and what the sparse form adds
        refused(source, E_INVAL, mask=ghf.SPARSE_AUTO)
        refused(source, E_INVAL, mask=ghf.SPARSE_AUTO | 1)
        refused(source, E_INVAL, mask=1 << e)
        refused(source, E_INVAL, r_infos=None)
        refused(source, E_INVAL, r_ptrs=None)
        refused(source, E_INVAL, x=setter("r_ptrs", 1, None))
        refused(source, E_INVAL, x=setter("r_infos", 0, N + 1, "n"))
        refused(source, E_INVAL, n=N - 1, first=5, count=9)          # no stream has the symbols of another n_elems
        refused(source, E_INVAL, mask=1)                             # plane 1 given as dense: its stream is a mask
        refused(source, E_INVAL, x=setter("r_infos", 1, s["ranks"][1][0].n_vals + 1, "n_vals"))  # the values stream has another count
        refused(source, E_INVAL, x=setter("ptrs", e + 1, None))      # a values slot that is needed
    a = args("side-cars")
    a["infos"], a["t_ptrs"], a["t_bytes"] = args("tables")["infos"], args("tables")["t_ptrs"], args("tables")["t_bytes"]
    assert call(a) == E_INVAL  # both sources
    a = args("side-cars")
    a["base"] = None
    assert call(a, True) == E_INVAL
    a["base"] = d_shard.data_ptr() + 8
    assert call(a, True) == E_INVAL
    # a dense stream whose symbol count is not n_elems / a mask stream whose count is not the mask's: the side-car of another slot
    a = args("side-cars")
    swapped = (ghf.Index * slots)(*[s["r"]["indexes"][j] for j in (e, 1, 0, 1)])
    a["idx"] = swapped
    assert call(a) == E_INVAL
    a = args("tables")
    a["t_bytes"][1] += 24
    assert call(a) == E_FORMAT  # a seek table whose size is not what its header implies
    a = args("tables")
    a["t_bytes"][e] += 24
    assert call(a) == E_FORMAT  # ... of a values stream
    # the two cum entries the call reads: not ordered, above n_vals, further apart than the sub-string has elements
    t = s["ranks"][0][1]
    cum = [int(v) for v in model.cum_in(t)]
    for what, j, value in (("not ordered", 0, cum[2] + 1), ("above n_vals", 2, cum[4] + 1)):  # the range reads cum[0] and cum[2]
        bad = t.copy()
        bad[64 + 8 * j : 72 + 8 * j] = np.frombuffer(int(value).to_bytes(8, "little"), np.uint8)
        for source in ("side-cars", "tables"):
            a = args(source)
            a["r_ptrs"][0] = bad.ctypes.data
            assert call(a) == E_FORMAT, (what, source)
    # further apart than the sub-string has elements: cum[1] = R + 1, read for a range inside block 0.  An info that allows so
    # many values has to claim them, and the values stream has to agree with the info to get this far
    bad = t.copy()
    bad[64 + 8 : 64 + 16] = np.frombuffer(int(R + 1).to_bytes(8, "little"), np.uint8)
    a = args("tables")
    a["r_ptrs"][0] = bad.ctypes.data
    a["first"], a["count"] = 5, 9
    a["r_infos"][0].n_vals = N
    a["infos"][e].n_symbols, a["infos"][e].n_blocks = N, -(-N // 4096)
    a["t_bytes"][e] = ghf.seek_bytes(N)
    assert call(a) == E_FORMAT
    a["r_ptrs"][0] = t.ctypes.data  # the same call with the true entries passes every check (count = 0: nothing is queued)
    a["count"] = 0
    assert call(a) == OK
    # a values slot is ignored when n_vals == 0
    z = stored(env, e, None, "delta", ghf.SPARSE_AUTO)
    assert z["r"]["n_vals"] == [0, 0] and z["slots"][e] is None and z["slots"][e + 1] is None
    assert L.ghf_sync(h) == OK and untouched(torch, buf)
    decode_range(ctx, s, "delta", e, first, count, "tables", d_shard, buf[PAD:])  # the context works
    ctx.sync()
    assert np.array_equal(buf[PAD : PAD + count * e].cpu().numpy(), s["new"][first * e : (first + count) * e])
