"""GPU: the seek table (ghf_seek_pack / ghf_seek_expand) and ghf_decode_range, all bit-exact.

The expected table is computed here from the reference's code lengths (tests/golden/golden.json) and the input alone:
symbol k begins at bit 8 * header_bytes + sum(length[in[:k]]).  Nothing the library computes enters it."""
import base64
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import datagen as dg
import pkgload
from cases import CASES, INLINE_CRS2
from oracle import oracle as orc
from range_worlds import expected_table

pytestmark = pytest.mark.gpu

E_INVAL, E_CAP, E_FORMAT, E_CORRUPT = 1, 5, 6, 7
GUARD = 0xA5
REC = np.dtype([("start", "<u8"), ("run", "<u2", (8,))])
assert REC.itemsize == 24


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def compress_with_index(ctx, torch, data):
    d_in = to_dev(torch, data)
    idx = ctx.index_alloc(data.size)
    d_out, nbytes, d_code = ctx.compress(d_in, index=idx)
    ctx.sync()
    return d_in, d_out, int(nbytes.item()), d_code, idx


def pack_to_host(ctx, idx, d_stream=None, stream_bytes=0, n=None):
    d_table = ctx.seek_pack(idx, d_stream, stream_bytes, n=n)
    ctx.sync()
    return d_table.cpu().numpy()


# ---------------------------------------------------------------- 1. the packed table against an independent expectation
@pytest.mark.parametrize("name", list(CASES))
def test_packed_table_equals_the_one_computed_from_reference_lengths(env, golden, name):
    ghf, ctx, torch = env
    g = golden[name]
    data = CASES[name]()
    _, d_out, nb, d_code, idx = compress_with_index(ctx, torch, data)
    got = pack_to_host(ctx, idx)
    want = expected_table(data, g["length"], 8 * g["header_bytes"])
    assert got.size == ghf.seek_bytes(data.size) == want.size
    assert np.array_equal(got, want), "first difference at byte %d" % int(np.nonzero(got != want)[0][0])
    ctx.index_free(idx)


# ---------------------------------------------------------------- 2. round trip through host bytes
def round_trip(ghf, ctx, torch, data):
    d_in, d_out, nb, d_code, idx = compress_with_index(ctx, torch, data)
    chunk0, seg0 = ctx.index_to_host(idx)
    table = pack_to_host(ctx, idx)
    ctx.index_free(idx)
    info = ghf.seek_parse(table)
    assert info.n_symbols == data.size and info.flags == 0
    d_table = to_dev(torch, table)
    idx2 = ctx.seek_expand(info, d_table, d_out, nb, d_code)
    ctx.sync()
    chunk1, seg1 = ctx.index_to_host(idx2)
    assert np.array_equal(chunk1, chunk0)
    assert np.array_equal(seg1, seg0), "first difference at segment %d" % int(np.nonzero(seg1 != seg0)[0][0])
    back, nout = ctx.decode(d_out, nb, d_code, idx2)
    ctx.sync()
    assert int(nout.item()) == data.size
    assert torch.equal(back[: data.size], d_in)
    ctx.index_free(idx2)


@pytest.mark.parametrize("name", list(CASES))
def test_round_trip_through_host_bytes(env, name):
    ghf, ctx, torch = env
    round_trip(ghf, ctx, torch, CASES[name]())


@pytest.mark.parametrize("n", [(8 << 20) - 1, 8 << 20, (8 << 20) + 4097])
@pytest.mark.parametrize("kind", ["uniform", "zipf", "sym16"])
def test_round_trip_8MiB(env, kind, n):
    ghf, ctx, torch = env
    round_trip(ghf, ctx, torch, dg.make(kind, n, seed=900 + n % 97))


# ---------------------------------------------------------------- 3. a stream the reference wrote
@pytest.mark.parametrize("name", sorted(INLINE_CRS2))
def test_reference_written_stream_indexed_once(env, golden, name):
    """golden.json carries these .crs2 files whole, as the compiled reference wrote them: K6 rebuilds the side-car once
    (decoded_size), seek_pack(index=None) keeps it, and from then on the file decodes through the table"""
    ghf, ctx, torch = env
    g = golden[name]
    crs = np.frombuffer(base64.b64decode(g["crs2_b64"]), dtype=np.uint8)
    assert crs.size == g["crs2_bytes"]
    code, hs = ghf.parse_header(crs)
    d_stream = to_dev(torch, np.concatenate([crs, np.zeros(64, np.uint8)]))
    d_code = ctx.code_to_device(code)
    n = ctx.decoded_size(d_stream, crs.size, d_code)
    assert n == g["n"]
    table = pack_to_host(ctx, None, d_stream, crs.size, n=n)
    assert np.array_equal(table, expected_table(CASES[name](), g["length"], 8 * g["header_bytes"]))
    info = ghf.seek_parse(table)
    idx = ctx.seek_expand(info, to_dev(torch, table), d_stream, crs.size, d_code)
    back, nout = ctx.decode(d_stream, crs.size, d_code, idx)
    ctx.sync()
    assert int(nout.item()) == n
    assert hashlib.sha256(back[:n].cpu().numpy().tobytes()).hexdigest() == g["decoded_sha256"]
    ctx.index_free(idx)


def test_seek_pack_without_index_needs_a_rebuilt_side_car(env):
    ghf, ctx, torch = env
    crs = orc.compress(dg.zipf_bytes(5000, seed=3))
    d_stream = to_dev(torch, np.concatenate([crs, np.zeros(64, np.uint8)]))
    other = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(ghf.GhfError) as e:
        ctx.seek_pack(None, other, 4096, n=5000)
    assert e.value.status == E_INVAL


# ---------------------------------------------------------------- 4. decode_range
def range_pairs(n):
    fixed = [
        (4096 * 5, 10000), (4096 * 5 + 100, 10000),            # block-aligned / unaligned start
        (0, 10), (4096 * 7, 33), (4096 * 7 + 3, 40),          # end inside the first segment of a block
        (1000, 5017), (4096 * 2, 4096 + 77),                   # end inside a segment
        (100, 64 * 50 - 100), (4096 * 9, 64 * 3),              # end on a segment end
        (100, 4096 * 3 - 100), (4096, 8192), (4096 * 4 + 64, 4096 - 64),  # end on a block end
        (4096 * 3 + 70, 20), (64 * 11 + 1, 62),                # inside one segment
        (0, 1), (4095, 1), (4096, 1), (n - 1, 1),              # count 1
        (0, n),                                                # the whole stream
        (n - 5000, 5000), (n - 2 * 4096 - 1, 2 * 4096 + 1), (n - 64, 64), (n - 4096, 4096),  # ending at n
    ]
    rng = np.random.default_rng(20240607)
    rand = []
    for i in range(200):
        first = int(rng.integers(0, n))
        limit = n - first
        count = int(rng.integers(1, min(limit, (1 << 21) if i % 4 == 0 else 20000) + 1))
        rand.append((first, count))
    return fixed + rand


@pytest.mark.parametrize("kind", ["zipf", "uniform"])
def test_decode_range(env, kind):
    ghf, ctx, torch = env
    n = 3 << 20
    data = dg.make(kind, n, seed=77)
    d_in, d_out, nb, d_code, idx = compress_with_index(ctx, torch, data)
    table = pack_to_host(ctx, idx)
    info = ghf.seek_parse(table)
    d_table = to_dev(torch, table)
    pad = 256
    buf = torch.empty(n + 2 * pad, dtype=torch.uint8, device="cuda")
    pairs = range_pairs(n)
    assert len(pairs) >= 220
    for first, count in pairs:
        for source in ("index", "table"):
            for off in (pad, pad + 67):  # buf is 256-byte aligned: a 16-aligned and an odd output pointer
                buf.fill_(GUARD)
                out = buf[off : off + count]
                assert out.data_ptr() % 16 == (0 if off == pad else 3)
                if source == "index":
                    ctx.decode_range(d_out, nb, d_code, first, count, index=idx, d_out=out)
                else:
                    ctx.decode_range(d_out, nb, d_code, first, count, info=info, d_table=d_table, d_out=out)
                ctx.sync()
                where = (kind, source, first, count, off)
                assert torch.equal(out, d_in[first : first + count]), where
                assert bool((buf[:off] == GUARD).all()) and bool((buf[off + count :] == GUARD).all()), where
    # argument errors
    out = buf[pad : pad + 100]
    for kw in ({"index": idx}, {"info": info, "d_table": d_table}):
        with pytest.raises(ghf.GhfError) as e:
            ctx.decode_range(d_out, nb, d_code, n - 50, 100, d_out=out, **kw)
        assert e.value.status == E_INVAL
        with pytest.raises(ghf.GhfError) as e:
            ctx.decode_range(d_out, nb, d_code, n + 1, 0, d_out=out, **kw)
        assert e.value.status == E_INVAL
        with pytest.raises(ghf.GhfError) as e:
            ctx.decode_range(d_out, nb, d_code, 10, 100, d_out=out, cap=99, **kw)
        assert e.value.status == E_CAP
    for kw in ({}, {"index": idx, "info": info, "d_table": d_table}, {"info": info}, {"d_table": d_table}):
        with pytest.raises(ghf.GhfError) as e:
            ctx.decode_range(d_out, nb, d_code, 10, 100, d_out=out, table_bytes=table.size, **kw)
        assert e.value.status == E_INVAL
    with pytest.raises(ghf.GhfError) as e:  # a misaligned stream pointer
        ctx.decode_range(d_out[1:], nb - 1, d_code, 10, 100, index=idx, d_out=out)
    assert e.value.status == E_INVAL
    with pytest.raises(ghf.GhfError) as e:  # a misaligned table pointer
        ctx.decode_range(d_out, nb, d_code, 10, 100, info=info, d_table=to_dev(torch, np.concatenate([[0], table]).astype(np.uint8))[1:], d_out=out)
    assert e.value.status == E_INVAL
    # count == 0: nothing happens
    buf.fill_(GUARD)
    ctx.decode_range(d_out, nb, d_code, 1234, 0, index=idx, d_out=buf[pad:pad + 1], cap=0)
    ctx.sync()
    assert bool((buf == GUARD).all())
    ctx.index_free(idx)


# ---------------------------------------------------------------- 5. a GHF_EMIT_REBASE shard
def test_rebased_shard_keeps_its_flag(env):
    ghf, ctx, torch = env
    data = dg.zipf_bytes(300001, seed=5)
    d_in = to_dev(torch, data)
    d_code = ctx.build_code(ctx.histogram(d_in))
    ctx.encode_plan(d_in, d_code)
    S = 128 * 77777 + 37
    assert S % 128 != 0
    start = torch.tensor([S], dtype=torch.int64, device="cuda")
    idx = ctx.index_alloc(data.size)
    d_out = torch.zeros(ghf.shard_bound(data.size), dtype=torch.uint8, device="cuda")
    end = ctx.encode_emit(d_in, d_code, d_out, start_bit=start, flags=ghf.EMIT_REBASE, index=idx)  # no GHF_EMIT_LAST
    ctx.sync()
    idx.flags = ghf.INDEX_NO_END_MARK
    nbytes = int(end[1].item())
    chunk0, seg0 = ctx.index_to_host(idx)
    table = pack_to_host(ctx, idx)
    code = ctx.code_to_host(d_code)
    assert np.array_equal(table, expected_table(data, list(code.length), S % 128, flags=ghf.INDEX_NO_END_MARK))
    ctx.index_free(idx)
    info = ghf.seek_parse(table)
    assert info.flags == ghf.INDEX_NO_END_MARK
    idx2 = ctx.seek_expand(info, to_dev(torch, table), d_out, nbytes, d_code)
    assert idx2.flags == ghf.INDEX_NO_END_MARK
    ctx.sync()
    chunk1, seg1 = ctx.index_to_host(idx2)
    assert np.array_equal(chunk1, chunk0) and np.array_equal(seg1, seg0)
    back, nout = ctx.decode(d_out, nbytes, d_code, idx2)
    ctx.sync()
    assert int(nout.item()) == data.size and torch.equal(back[: data.size], d_in)
    # ... and a range of the shard that reaches its end: no end mark is asked for
    out = ctx.decode_range(d_out, nbytes, d_code, data.size - 7000, 7000, info=info, d_table=to_dev(torch, table))
    ctx.sync()
    assert torch.equal(out[:7000], d_in[data.size - 7000 :])
    ctx.index_free(idx2)


# ---------------------------------------------------------------- 6. corrupted tables
def _records(table):
    return table[64:].view(REC)


def _corrupt(table, what):
    t = table.copy()
    r = _records(t)
    if what == "run_plus_1":
        r["run"][5, 3] += 1
    elif what == "run_minus_1":
        r["run"][6, 0] -= 1
    elif what == "start_plus_8":
        r["start"][7] += 8
    elif what == "start_beyond_stream":
        r["start"][5] = np.uint64(1) << np.uint64(40)
    elif what == "start_huge":
        r["start"][8] = np.uint64(0xFFFFFFFFFFFFFFF0)
    elif what == "records_swapped":
        r[[6, 7]] = r[[7, 6]]
    elif what == "records_truncated":
        t = t[:-24]
    else:
        raise AssertionError(what)
    return t


def _status_of(ghf, ctx, call):
    """the status the call itself returns, else the one ghf_sync() reports behind it (which also clears it)"""
    try:
        call()
    except ghf.GhfError as e:
        ctx.sync()
        return e.status
    try:
        ctx.sync()
    except ghf.GhfError as e:
        return e.status
    return 0


@pytest.mark.parametrize("what", ["run_plus_1", "run_minus_1", "start_plus_8", "start_beyond_stream", "start_huge",
                                  "records_swapped", "records_truncated"])
def test_corrupted_table_is_reported_and_harms_nothing(env, what):
    """every start bit of a table is checked against the stream before anything is read there, so these are ordinary
    runs; each is done once"""
    ghf, ctx, torch = env
    n = 1 << 20
    data = dg.zipf_bytes(n, seed=66)
    d_in, d_out, nb, d_code, idx = compress_with_index(ctx, torch, data)
    table = pack_to_host(ctx, idx)
    info = ghf.seek_parse(table)
    bad = _corrupt(table, what)
    d_bad = to_dev(torch, bad)
    # the index arrays of seek_expand sit between guard bytes
    pad = 256
    cb = torch.full((pad + 8 * idx.n_chunks + pad,), GUARD, dtype=torch.uint8, device="cuda")
    sb = torch.full((pad + 4 * idx.n_segs + pad,), GUARD, dtype=torch.uint8, device="cuda")
    fake = ghf.Index()
    C.memmove(C.byref(fake), C.byref(idx), C.sizeof(ghf.Index))
    fake.d_chunk_bit = cb.data_ptr() + pad
    fake.d_seg_bit = sb.data_ptr() + pad
    st = _status_of(ghf, ctx, lambda: ctx.seek_expand(info, d_bad, d_out, nb, d_code, index=fake, table_bytes=bad.size))
    assert st in (E_CORRUPT, E_FORMAT), st
    for g in (cb, sb):
        assert bool((g[:pad] == GUARD).all()) and bool((g[-pad:] == GUARD).all())
    # table-driven range decode over the damaged blocks (3 .. 12), unaligned start
    first, count = 4096 * 3 + 5, 4096 * 10
    buf = torch.full((count + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
    st = _status_of(ghf, ctx, lambda: ctx.decode_range(d_out, nb, d_code, first, count, info=info, d_table=d_bad,
                                                       d_out=buf[pad : pad + count], table_bytes=bad.size))
    assert st in (E_CORRUPT, E_FORMAT), st
    assert bool((buf[:pad] == GUARD).all()) and bool((buf[-pad:] == GUARD).all())
    # the context is usable again (Context.sync() cleared the status): a clean decode, by the table and by the index
    d_table = to_dev(torch, table)
    out = ctx.decode_range(d_out, nb, d_code, first, count, info=info, d_table=d_table)
    back, nout = ctx.decode(d_out, nb, d_code, idx)
    ctx.sync()
    assert torch.equal(out[:count], d_in[first : first + count])
    assert int(nout.item()) == n and torch.equal(back[:n], d_in)
    ctx.index_free(idx)
