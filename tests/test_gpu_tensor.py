"""GPU: the container calls (include/ghf_tensor.h) against tests/tensor_model.py, byte for byte.

ghf_compress_tensor and ghf_tensor_pack must write exactly the model's container -- head, tables, rank tables, streams, zero
pads -- and nothing behind it; a container copied to another address opens from its 768 head bytes and decodes, whole, in
place, by range and by rows, to the tensor; a capacity that does not suffice is a verdict reached before the first store; a
damaged container is refused by the open (the head) or by the device (a .crs2 header, a table header) and no decoder serves it.
The inputs, the masks the choice rule answers for them and the container sizes are pinned here from the model."""
import importlib

import numpy as np
import pytest

import pkgload
import tensor_model as tm

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_CAP, E_FORMAT, E_CORRUPT = 0, 1, 5, 6, 7
FILL = 0xA5
# the container sizes of the pinned inputs, as the model gives them (asserted before they are used)
SIZES = {"d4": 94224, "d2": 23680, "d8": 26576, "p4": 15728, "p2_1": 800, "p2_9": 800}
RANGES = ((0, None), (4095, 3), (32767, 2), (40000, 20000), (None, 1))  # None: n, and n - 1


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    gt = importlib.import_module("golden_huffman_amd.ghf_tensor")
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, gt, ctx, torch
    ctx.close()


def to_dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def filled(torch, n, value=FILL):
    return torch.full((n,), value, dtype=torch.uint8, device="cuda")


def status_of(ghf, call):
    """the status a call (or the sync behind it) raises, 0 when it does not"""
    try:
        call()
    except ghf.GhfError as err:
        return err.status
    return OK


def compress(env, key, cap=None, room=64):
    """ghf_compress_tensor of a pinned input into a buffer of 0xA5 -> (the whole buffer on the host, the reported size, cap)"""
    ghf, gt, ctx, torch = env
    e, n, rel, raw, sparse, _, _ = tm.CASES[key]
    base, new, c = tm.case(key)
    cap = gt.bound(n, e) if cap is None else cap
    buf = filled(torch, cap + room)
    d_base = None if base is None else to_dev(torch, base)
    _, nbytes = gt.compress_tensor(ctx, to_dev(torch, new), e, raw_planes=raw, sparse_planes=sparse, d_base=d_base, d_container=buf, cap=cap)
    return buf, nbytes, cap


@pytest.fixture(scope="module")
def packed(env):
    """key -> the container the library wrote for a pinned input, on the host, checked against the model once"""
    ghf, gt, ctx, torch = env
    cache = {}

    def get(key):
        if key not in cache:
            c = tm.case(key)[2]
            buf, nbytes, cap = compress(env, key)
            ctx.sync()
            host = buf.cpu().numpy()
            assert int(nbytes.item()) == c.total == SIZES[key], key
            assert np.array_equal(host[: c.total], c.bytes), (key, int(np.flatnonzero(host[: c.total] != c.bytes)[0]))
            assert (host[c.total :] == FILL).all(), key
            cache[key] = host[: c.total].copy()
        return cache[key]

    return get


def test_the_model_answers_the_pinned_masks_and_sizes():
    for key, (e, n, rel, raw, sparse, want_raw, want_sparse) in tm.CASES.items():
        c = tm.case(key)[2]
        assert (c.raw, c.sparse) == (want_raw, want_sparse) and c.total == SIZES[key], key
    for key, want in tm.N_VALS.items():
        assert tm.case(key)[2].stored.n_vals == want, key


@pytest.mark.parametrize("key", list(tm.CASES))
def test_compress_tensor_writes_the_model_container_and_nothing_behind_it(packed, key):
    packed(key)  # size, bytes [0, size) and the fill behind them are held there


def test_pack_from_the_forms_outputs_gives_the_same_container(env, packed):
    """ghf_tensor_pack on what ghf_compress_planes_forms left, explicit masks, slots full of 0xEE: the pads come out zero"""
    ghf, gt, ctx, torch = env
    for key in ("d4", "p4"):
        e, n = tm.CASES[key][:2]
        base, new, c = tm.case(key)
        slot = ghf.planes_slot_bytes(n)
        d_slots = filled(torch, 2 * e * slot, 0xEE)
        fr = ctx.compress_planes_forms(to_dev(torch, new), e, raw_planes=c.raw, sparse_planes=c.sparse,
                                       d_base=None if base is None else to_dev(torch, base), d_out=d_slots, slot_bytes=slot, indexes=True,
                                       ranks=True)
        assert (fr["raw_planes"], fr["sparse_planes"]) == (c.raw, c.sparse)
        streams = [d_slots[j * slot : (j + 1) * slot] for j in range(2 * e)]
        rsb = fr["rank_slot_bytes"]
        ranks = [fr["ranks"][p * rsb : (p + 1) * rsb] for p in range(e)]
        buf = filled(torch, c.total + 64)
        _, nbytes = gt.pack(ctx, streams, fr["out_bytes"], fr["indexes"], ranks, c.raw, c.sparse, fr["n_vals"], n, e, flags=c.flags,
                            d_container=buf, cap=c.total)
        ctx.sync()
        host = buf.cpu().numpy()
        assert int(nbytes.item()) == c.total
        assert np.array_equal(host[: c.total], packed(key)) and (host[c.total :] == FILL).all(), key
        ctx.planes_index_free(fr["indexes"])


def test_every_stream_size_residue_modulo_16(env):
    """all-raw bf16-wide tensors of 1 .. 48 elements: both streams have n bytes, the pads are zero, the bytes the model's"""
    ghf, gt, ctx, torch = env
    runs = []
    for n in range(1, 49):
        src, c = tm.all_raw(n)
        slot = ghf.planes_slot_bytes(n)
        d_slots = filled(torch, 4 * slot, 0xEE)
        fr = ctx.compress_planes_forms(to_dev(torch, src), 2, raw_planes=0b11, sparse_planes=0, d_out=d_slots, slot_bytes=slot, indexes=True)
        buf = filled(torch, c.total + 32)
        _, nbytes = gt.pack(ctx, [d_slots[j * slot : (j + 1) * slot] for j in range(4)], fr["out_bytes"], fr["indexes"], None, 0b11, 0,
                            fr["n_vals"], n, 2, d_container=buf, cap=c.total)
        runs.append((n, c, buf, nbytes, d_slots))
    ctx.sync()
    for n, c, buf, nbytes, _ in runs:
        host = buf.cpu().numpy()
        assert int(nbytes.item()) == c.total == 768 + 2 * tm.pad16(n), n
        assert np.array_equal(host[: c.total], c.bytes), n
        assert not host[768 + n : 768 + tm.pad16(n)].any() and (host[c.total :] == FILL).all(), n


@pytest.mark.parametrize("n", [(3 << 20) + 7, (65 << 20) + 5])
def test_large_raw_streams_through_the_loop_with_four_loads_in_flight(env, n):
    """all-raw bf16-wide tensors: 3 Mi elements give slabs of 1022 vectors (one trip of the unrolled loop for 254 lanes, fewer workgroups
    than the cap), 65 Mi elements 4096 slabs of 2081 vectors (two trips and a tail, sections that begin inside a slab)"""
    ghf, gt, ctx, torch = env
    src, c = tm.all_raw(n)
    region = (c.total - c.streams_off) // 16
    groups = min(4096, max(1, (2 * tm.pad16(n) // 16 + 1023) // 1024))
    # a lane takes the unrolled loop while 768 vectors lie in front of it: 254 of 256 lanes once, and every lane twice
    assert -(-region // groups) == (2081 if n > (64 << 20) else 1022)
    buf = filled(torch, c.total + 64)
    _, nbytes = gt.compress_tensor(ctx, to_dev(torch, src), 2, raw_planes=0b11, sparse_planes=0, d_container=buf, cap=c.total)
    ctx.sync()
    assert int(nbytes.item()) == c.total == 768 + 2 * tm.pad16(n)
    want = to_dev(torch, c.bytes)
    assert torch.equal(buf[: c.total], want) and bool((buf[c.total :] == FILL).all())
    del buf, want
    gt.release_workspace(ctx)  # 4 slots of 1.125 n bytes go back; the next call grows its own


def test_a_stored_stream_of_no_bytes_is_refused_by_the_device(env):
    """a size of 0 for a stored slot is not one any stage writes: GHF_E_CORRUPT, nothing stored"""
    ghf, gt, ctx, torch = env
    n = 100
    src, c = tm.all_raw(n)
    d_planes = to_dev(torch, np.concatenate([np.resize(p, 112) for p in c.stored.planes]))
    sizes = torch.tensor([n, 0, 0, 0], dtype=torch.int64, device="cuda")
    buf = filled(torch, c.total + 32)
    nbytes = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    gt.pack(ctx, [d_planes[:112], d_planes[112:], None, None], sizes, (ghf.Index * 4)(), None, 0b11, 0, [0, 0], n, 2, d_container=buf,
            cap=c.total, nbytes=nbytes)
    assert status_of(ghf, ctx.sync) == E_CORRUPT
    assert (buf.cpu().numpy() == FILL).all() and int(nbytes.item()) == -77


def test_the_workspace_comes_back_after_a_release(env, packed):
    ghf, gt, ctx, torch = env
    want = packed("d2")
    gt.release_workspace(ctx)
    buf, nbytes, cap = compress(env, "d2")
    ctx.sync()
    assert int(nbytes.item()) == want.size and np.array_equal(buf.cpu().numpy()[: want.size], want)


def relocated(env, host, shift=48):
    """the container in a fresh buffer at another 16-byte offset, opened from its 768 head bytes alone"""
    ghf, gt, ctx, torch = env
    buf = filled(torch, host.size + shift + 64, 0xC3)
    view = buf[shift : shift + host.size]
    view.copy_(to_dev(torch, host))
    assert view.data_ptr() % 16 == 0
    return gt.open(ctx, view, host.size, head=host[: tm.HEAD_BYTES]), view


@pytest.mark.parametrize("key", list(tm.CASES))
def test_a_relocated_container_decodes_whole_in_place_by_range_and_by_rows(env, packed, key):
    ghf, gt, ctx, torch = env
    e, n = tm.CASES[key][:2]
    base, new, c = tm.case(key)
    t, keep = relocated(env, packed(key))
    info = t.info
    assert (info.elem_bytes, info.n_elems, info.raw_planes, info.sparse_planes, info.flags, info.total_bytes) == (e, n, c.raw, c.sparse, c.flags, c.total)
    d_base = None if base is None else to_dev(torch, base)
    whole, nbytes = t.decode(d_base=d_base, d_out=filled(torch, n * e + 32, 0x5A), cap=n * e)
    outs = [("whole", whole, new, n * e)]
    if base is not None:  # in place: d_out holds the base
        inplace = to_dev(torch, base)
        t.decode(d_base=inplace, d_out=inplace)
        outs.append(("in place", inplace, new, n * e))
    for first, count in RANGES:
        first = n - 1 if first is None else first
        count = n - first if count is None else count
        if first + count > n:
            continue
        r_base = None if base is None else to_dev(torch, base[first * e : (first + count) * e])
        part = t.decode_range(first, count, d_base=r_base, d_out=filled(torch, count * e + 32, 0x5A), cap=count * e)
        outs.append(("range %d+%d" % (first, count), part, new[first * e : (first + count) * e], count * e))
    rows = None
    if n >= 128:
        rng = np.random.default_rng(3)
        idx = np.concatenate([rng.integers(0, n - 127, size=62), [0, n - 128]]).astype(np.int64)  # the tensor's last row included
        d_rows, d_status = t.gather(to_dev(torch, idx), 128, index_stride=1, d_base=d_base)
        rows = (idx, d_rows, d_status)
    ctx.sync()
    assert int(nbytes.item()) == n * e
    for what, d_out, want, size in outs:
        got = d_out.cpu().numpy()
        assert np.array_equal(got[:size], want), (key, what)
        assert got.size == size or (got[size:] == 0x5A).all(), (key, what)
    if rows:
        idx, d_rows, d_status = rows
        assert not d_status.cpu().numpy().any(), key
        got = d_rows.cpu().numpy().reshape(64, 128 * e)
        for r, first in enumerate(idx):
            assert np.array_equal(got[r], new[first * e : (first + 128) * e]), (key, r)
    t.close()


def test_a_head_fetched_by_the_open_itself(env, packed):
    ghf, gt, ctx, torch = env
    host = packed("p4")
    _, new, c = tm.case("p4")
    view = to_dev(torch, host)
    t = gt.open(ctx, view, host.size, head=None)
    out, _ = t.decode()
    ctx.sync()
    assert np.array_equal(out.cpu().numpy()[: new.size], new)
    t.close()


def test_a_capacity_that_does_not_suffice(env, packed):
    ghf, gt, ctx, torch = env
    c = tm.case("d4")[2]
    size = c.total
    packed("d4")
    # one vector short: the verdict comes from the device, before any workgroup's first store to the stream region
    buf, nbytes, cap = compress(env, "d4", cap=size - 16, room=64)
    assert status_of(ghf, ctx.sync) == E_CAP
    host = buf.cpu().numpy()
    assert int(nbytes.item()) == size
    assert (host[cap:] == FILL).all()
    assert (host[c.streams_off : cap] == FILL).all() and (host[:768] == FILL).all()  # neither a stream nor the head was stored
    # below the host-known part: refused at call level, nothing written
    low = c.streams_off - 16
    buf = filled(torch, size)
    assert status_of(ghf, lambda: compress_into(env, "d4", buf, low)) == E_CAP
    ctx.sync()
    assert (buf.cpu().numpy() == FILL).all()
    # ... and by the pack call with nothing at all queued
    e, n = c.e, c.n
    idx = (ghf.Index * (2 * e))()
    for j in range(2 * e):
        if c.stored.kind[j] == "image":
            idx[j] = ctx.index_alloc(c.stored.symbols[j])
    dummy = filled(torch, 4096)
    call = lambda: gt.pack(ctx, [dummy] * (2 * e), torch.zeros(2 * e, dtype=torch.int64, device="cuda"), idx, [dummy] * e, c.raw, c.sparse,  # noqa: E731
                           c.stored.n_vals, n, e, flags=c.flags, d_container=buf, cap=low)
    assert status_of(ghf, call) == E_CAP
    ctx.sync()
    assert (buf.cpu().numpy() == FILL).all()
    ctx.planes_index_free(idx)


def compress_into(env, key, buf, cap):
    ghf, gt, ctx, torch = env
    e, n, rel, raw, sparse, _, _ = tm.CASES[key]
    base, new, _ = tm.case(key)
    return gt.compress_tensor(ctx, to_dev(torch, new), e, raw_planes=raw, sparse_planes=sparse, d_base=to_dev(torch, base), d_container=buf,
                              cap=cap)


def test_a_damaged_container(env, packed):
    ghf, gt, ctx, torch = env
    good = packed("d4")
    base, new, c = tm.case("d4")
    e, n = c.e, c.n
    d_base = to_dev(torch, base)
    idx = to_dev(torch, np.arange(0, 64 * 128, 128, dtype=np.int64))
    # a .crs2 header word of the dense plane: the min_len word no longer fits the code
    bad = good.copy()
    bad[c.dir[tm.STREAMS + 1][0] + 4 * 258 + 3] ^= 0x20
    t, keep = relocated(env, bad)
    assert status_of(ghf, ctx.sync) == E_FORMAT  # latched by k_tensor_open
    out = filled(torch, n * e, 0x5A)
    nbytes = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    t.decode(d_base=d_base, d_out=out, nbytes=nbytes)
    assert status_of(ghf, ctx.sync) == E_FORMAT  # the code stayed zero: no decoder builds tables from it
    assert (out.cpu().numpy() == 0x5A).all() and int(nbytes.item()) == -77  # neither the tensor nor its size was stored
    _, d_status = t.gather(idx, 128, index_stride=1, d_base=d_base)
    ctx.sync()  # a gather never latches
    assert (d_status.cpu().numpy() == E_FORMAT).all()
    t.close()
    # a seek table that is not one
    bad = good.copy()
    bad[c.dir[tm.TABLES + 1][0]] ^= 0xFF
    t, keep = relocated(env, bad)
    assert status_of(ghf, ctx.sync) == E_FORMAT
    t.close()
    # a rank table whose header counts other values than the head
    bad = good.copy()
    bad[c.dir[tm.RANKS + 2][0] + 24] ^= 1
    assert status_of(ghf, lambda: relocated(env, bad)) == E_FORMAT
    assert status_of(ghf, ctx.sync) == E_FORMAT  # the device saw it too; the sync clears it
    # a damaged directory: refused at once, nothing queued
    bad = good.copy()
    bad[128 + 16 * (tm.STREAMS + 1)] ^= 8
    assert status_of(ghf, lambda: relocated(env, bad)) == E_FORMAT
    ctx.sync()
    # ... and a container in a buffer that is shorter than its head says
    view = to_dev(torch, good)
    assert status_of(ghf, lambda: gt.open(ctx, view, good.size - 16, head=good[:768])) == E_FORMAT
    ctx.sync()


def test_the_delta_flag_is_held_against_the_base_both_ways(env, packed):
    ghf, gt, ctx, torch = env
    idx = to_dev(torch, np.arange(4, dtype=np.int64))
    for key, give_base in (("d4", False), ("p4", True)):
        base, new, c = tm.case(key)
        t, keep = relocated(env, packed(key))
        ctx.sync()
        d_base = to_dev(torch, new) if give_base else None
        out = filled(torch, new.size, 0x5A)
        assert status_of(ghf, lambda: t.decode(d_base=d_base, d_out=out)) == E_INVAL, key
        assert status_of(ghf, lambda: t.decode_range(5, 7, d_base=d_base, d_out=out)) == E_INVAL, key
        assert status_of(ghf, lambda: t.gather(idx, 128, d_base=d_base, d_out=out)) == E_INVAL, key
        ctx.sync()  # nothing was queued, nothing latched
        assert (out.cpu().numpy() == 0x5A).all(), key
        t.close()
