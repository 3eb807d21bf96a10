"""GPU: ghf_decode_planes_gather, bit-exact against numpy slices of the tensor.

Streams, codes and seek tables are the oracle's and range_worlds.expected_table's (tests/gather_planes.py), so
k_decode_planes_gather is the only device code here; one test goes through ghf_compress_planes_forms + ghf_seek_pack to hold
the two together.  Every stream, table and raw plane lies in a guarded arena (tests/guarded.py) at exactly its size, and so
does the output: the bytes around it and the padding between its rows must keep the fill pattern.  Expected verdicts come from
tests/gather_model.py, which restates the call's rules in numpy, and are spelled out beside it where the case is small."""
import ctypes as C

import numpy as np
import pytest

import gather_model as gm
import gather_planes as gp
import pkgload
from guarded import GUARD, Arena, first_diff

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_FORMAT, E_CORRUPT = gm.OK, gm.E_INVAL, gm.E_FORMAT, gm.E_CORRUPT
WIDTHS = (2, 4, 8)


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def to_dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the oracle's arrays are read-only)


class Stored:
    """a tensor of gather_planes on the device: per plane its stream, its table and the plane itself (the raw form), each at
    exactly its size in one guarded arena; the codes as the oracle built them"""

    def __init__(self, ghf, torch, t):
        self.t, self.e, self.n = t, t.e, t.n
        self.arena = Arena()
        self.k_stream = [self.arena.add(p.stream_bytes) for p in t.planes]
        self.k_table = [self.arena.add(p.table.size) for p in t.planes]
        self.k_raw = [self.arena.add(t.n) for p in t.planes]
        self.arena.alloc(torch)
        for i, p in enumerate(t.planes):
            self.arena.view(self.k_stream[i]).copy_(to_dev(torch, p.stream))
            self.arena.view(self.k_table[i]).copy_(to_dev(torch, p.table))
            self.arena.view(self.k_raw[i]).copy_(to_dev(torch, p.data))
        self.infos = [ghf.seek_parse(p.table) for p in t.planes]
        self.d_codes = to_dev(torch, np.frombuffer(b"".join(bytes(p.code) for p in t.planes), dtype=np.uint8))
        assert self.d_codes.numel() == t.e * C.sizeof(ghf.Code)

    def args(self, raw, tables=None, stream_bytes=None, d_codes=None):
        """what Context.decode_planes_gather takes for this tensor with the planes of `raw` stored raw; tables / stream_bytes:
        {plane: a damaged table on the device / a cut size}"""
        e = self.e
        streams = [self.arena.view(self.k_raw[i] if raw >> i & 1 else self.k_stream[i]) for i in range(e)]
        sizes = [self.n if raw >> i & 1 else self.t.planes[i].stream_bytes for i in range(e)]
        d_tables = [None if raw >> i & 1 else self.arena.view(self.k_table[i]) for i in range(e)]
        for i, tb in (tables or {}).items():
            d_tables[i] = tb
        for i, sb in (stream_bytes or {}).items():
            sizes[i] = sb
        infos = [None if raw >> i & 1 else self.infos[i] for i in range(e)]
        return dict(streams=streams, stream_bytes=sizes, d_codes=self.d_codes if d_codes is None else d_codes, raw_planes=raw,
                    n_elems=self.n, elem_bytes=e, infos=infos, d_tables=d_tables)


@pytest.fixture(scope="module")
def stored(env):
    ghf, ctx, torch = env
    cache = {}

    def get(e, n=gp.N_SMALL):
        if (e, n) not in cache:
            cache[e, n] = Stored(ghf, torch, gp.tensor(e, n))
        return cache[e, n]

    return get


def gather(env, s, raw, indices, index_stride, row_elems, out_stride=None, **damage):
    """one call into a guarded output -> (the output rows as they came back, one uint8 array of out_stride bytes per row; the
    statuses; whether every byte around the output kept the fill pattern).  The context's status must still be GHF_OK."""
    ghf, ctx, torch = env
    e = s.e
    out_stride = row_elems * e if out_stride is None else out_stride
    n_rows = len(indices)
    arena = Arena()
    k = arena.add(n_rows * out_stride)
    arena.alloc(torch)
    d_index = to_dev(torch, np.asarray(indices, dtype=np.uint64).view(np.int64))
    d_status = torch.full((n_rows,), -1, dtype=torch.int32, device="cuda")
    ctx.decode_planes_gather(d_index=d_index, row_elems=row_elems, index_stride=index_stride, d_out=arena.view(k), out_stride=out_stride,
                             d_row_status=d_status, **s.args(raw, **damage))
    ctx.sync()  # raises if anything latched
    assert ghf.lib().ghf_status(ctx.h) == OK
    intact = arena.fetch() and s.arena.fetch()
    return arena.got(k).reshape(n_rows, out_stride), [int(v) for v in d_status.cpu().numpy()], intact


def check(env, s, raw, indices, index_stride, row_elems, out_stride=None, want_status=None, **damage):
    """the call against numpy: rows whose status is GHF_OK hold the tensor's bytes, every other byte of the output the fill"""
    e = s.e
    got, status, intact = gather(env, s, raw, indices, index_stride, row_elems, out_stride, **damage)
    if want_status is None:
        want_status = [OK] * len(indices)
    assert status == want_status, (e, raw, row_elems, index_stride, status, want_status)
    want = np.full(got.shape, GUARD, dtype=np.uint8)
    for r, (i, st) in enumerate(zip(indices, want_status)):
        if st == OK:
            want[r, : row_elems * e] = s.t.rows([i], index_stride, row_elems)[0]
    assert np.array_equal(got, want), (e, raw, row_elems, index_stride, first_diff(got.reshape(-1), want.reshape(-1)))
    assert intact, "a byte outside the output rows, or of a stream or table, was written"


def raw_modes(t):
    """no raw plane, what GHF_RAW_AUTO chooses, every plane raw"""
    return list(dict.fromkeys([0, t.raw_auto, (1 << t.e) - 1]))


# ---------------------------------------------------------------- 1. row shapes
@pytest.mark.parametrize("e", WIDTHS)
def test_row_shapes_in_every_form(env, stored, e):
    s = stored(e)
    for raw in raw_modes(s.t):
        for row_elems, stride, ids in gp.row_cases(s.n):
            # by element offset the rows lie tight (misaligned wherever the row bytes are no multiple of 16), by row id padded
            out_stride = row_elems * e + (0 if stride == 1 else 5)
            check(env, s, raw, ids, stride, row_elems, out_stride)


# ---------------------------------------------------------------- 2. the row cap
@pytest.mark.parametrize("e", WIDTHS)
def test_one_row_at_the_cap(env, stored, e):
    """65 runs: every lane of the run round, and (the stage holds one plane of such a row) the path that judges first and
    decodes each plane again in front of its stores"""
    s = stored(e, gp.N_CAP)
    assert len(gm.covered(700, gm.MAX_ROW_ELEMS, s.n)) == 65
    check(env, s, 0, [700], 1, gm.MAX_ROW_ELEMS)
    check(env, s, s.t.raw_auto | 1, [700, 0], 1, gm.MAX_ROW_ELEMS)


# ---------------------------------------------------------------- 3. out stride and guards
def test_misaligned_rows_and_padding(env, stored):
    s = stored(2)
    ids = [4090, 0, 505, 4090, s.n - 7]
    check(env, s, 0, ids, 1, 7, 14)  # seven bf16 elements: rows 14 bytes apart, all but the first misaligned
    check(env, s, 0, ids, 1, 7, 14 + 3)
    check(env, s, 0b10, ids, 1, 7, 14 + 19)


# ---------------------------------------------------------------- 4. per-row verdicts
def model_status(s, raw, indices, stride, row_elems, planes=None):
    planes = s.t.model_planes(raw) if planes is None else planes
    return [gm.row_verdict(i, stride, row_elems, s.n, planes) for i in indices]


@pytest.mark.parametrize("e", WIDTHS)
def test_rows_outside_the_tensor(env, stored, e):
    s = stored(e)
    n = s.n
    ids = [0, n // 4 + 10, (n - 4) // 4, 1 << 63, 5, n // 4 - 2]  # stride 4: ok, past the end, passes n, overflows, ok, ok
    want = [OK, E_INVAL, E_INVAL, E_INVAL, OK, OK]
    for raw in raw_modes(s.t):
        assert model_status(s, raw, ids, 4, 7) == want
        check(env, s, raw, ids, 4, 7, want_status=want)


@pytest.mark.parametrize("e", WIDTHS)
def test_a_code_with_a_broken_length_count(env, stored, e):
    ghf, ctx, torch = env
    s = stored(e)
    bad = s.d_codes.clone().cpu().numpy()
    code = ghf.Code.from_buffer_copy(bad[: C.sizeof(ghf.Code)].tobytes())
    sym = next(v for v in range(256) if code.length[v] == code.max_len)
    code.length[sym] -= 1  # the lengths no longer satisfy Kraft with equality
    bad[: C.sizeof(ghf.Code)] = np.frombuffer(bytes(code), dtype=np.uint8)
    ids = [0, 100, s.n, 4096]
    check(env, s, 0, ids, 1, 7, want_status=[E_FORMAT] * 4, d_codes=to_dev(torch, bad))
    check(env, s, 0b01, ids, 1, 7, want_status=[OK, OK, E_INVAL, OK], d_codes=to_dev(torch, bad))  # plane 0 raw: its code is never read


# rows of 512 elements by element offset, inside block 1 unless said otherwise
BLOCK1 = 4096
DAMAGE_ROWS = [BLOCK1 + 3 * 512, BLOCK1 + 4 * 512, BLOCK1 + 2 * 512, BLOCK1 + 5 * 512, BLOCK1 + 2 * 512 + 1, BLOCK1 + 7 * 512, 0,
               2 * 4096, 3 * 4096, BLOCK1 - 512, BLOCK1 - 511]
# run 3; run 4; run 2; run 5; runs 2 and 3; run 7; block 0; block 2; block 3 (the last 5 symbols short: 512 still fit);
# the last run of block 0; that run and run 0 of block 1


def damaged(torch, plane, edits):
    t = plane.table.copy()
    rec = np.frombuffer(t[gm.HEADER :].tobytes(), dtype=gm.REC).copy()
    for (g, k), d in edits.items():
        rec["run"][g][k] = int(rec["run"][g][k]) + d
    t[gm.HEADER :] = np.frombuffer(rec.tobytes(), dtype=np.uint8)
    d = torch.full((t.size + 128,), GUARD, dtype=torch.uint8, device="cuda")  # the table at exactly its size, guards around it
    d[64 : 64 + t.size].copy_(to_dev(torch, t))
    assert d.data_ptr() % 16 == 0
    return t, d[64 : 64 + t.size]


@pytest.mark.parametrize("e", WIDTHS)
def test_two_run_lengths_that_keep_the_chain(env, stored, e):
    ghf, ctx, torch = env
    s = stored(e)
    t, d_t = damaged(torch, s.t.planes[0], {(1, 3): +1, (1, 4): -1})
    planes = s.t.model_planes(0)
    planes[0] = s.t.planes[0].model(table=t)
    want = model_status(s, 0, DAMAGE_ROWS, 1, 512, planes)
    assert want == [E_CORRUPT, E_CORRUPT, OK, OK, E_CORRUPT, OK, OK, OK, OK, OK, OK]
    check(env, s, 0, DAMAGE_ROWS, 1, 512, want_status=want, tables={0: d_t})


@pytest.mark.parametrize("e", WIDTHS)
def test_one_run_length_that_breaks_the_chain(env, stored, e):
    ghf, ctx, torch = env
    s = stored(e)
    t, d_t = damaged(torch, s.t.planes[0], {(1, 3): +1})
    planes = s.t.model_planes(0)
    planes[0] = s.t.planes[0].model(table=t)
    want = model_status(s, 0, DAMAGE_ROWS, 1, 512, planes)
    assert want == [E_CORRUPT] * 6 + [OK, OK, OK, OK, E_CORRUPT]
    check(env, s, 0, DAMAGE_ROWS, 1, 512, want_status=want, tables={0: d_t})


@pytest.mark.parametrize("e", WIDTHS)
def test_a_stream_cut_inside_the_last_block(env, stored, e):
    s = stored(e)
    pl = s.t.planes[0]
    rec = gm.records(pl.table)
    last = rec.size - 1
    cut = (int(rec[last]["start"]) + int(rec[last]["run"][0]) // 2) // 8  # ends inside run 0 of the last block
    assert 8 * cut >= int(rec[last]["start"]) and cut < pl.stream_bytes
    planes = s.t.model_planes(0)
    planes[0] = pl.model(stream_bytes=cut)
    ids = [0, BLOCK1, 2 * 4096 + 3584, 3 * 4096 - 3, 3 * 4096, s.n - 7, 3 * 4096 - 7]
    want = model_status(s, 0, ids, 1, 7, planes)
    assert want == [OK, OK, OK, E_CORRUPT, E_CORRUPT, E_CORRUPT, OK]
    check(env, s, 0, ids, 1, 7, want_status=want, stream_bytes={0: cut})


# ---------------------------------------------------------------- 5. call-level refusals
def test_call_level_refusals_queue_nothing_and_leave_the_status_alone(env, stored):
    ghf, ctx, torch = env
    s = stored(4)
    L, n, e = ghf.lib(), s.n, 4
    raw = 0b0100
    a = s.args(raw)
    ptrs = [x.data_ptr() for x in a["streams"]]
    tptrs = [0 if x is None else x.data_ptr() for x in a["d_tables"]]
    infos = [ghf.SeekInfo() if i is None else i for i in a["infos"]]
    tbytes = [0 if i is None else ghf.seek_bytes(i.n_symbols) for i in a["infos"]]
    d_index = to_dev(torch, np.array([0, 5], dtype=np.int64))
    d_out = torch.full((2 * 64 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_status = torch.full((2,), -1, dtype=torch.int32, device="cuda")

    def call(ctx_h=ctx.h, ptrs=ptrs, sizes=a["stream_bytes"], codes=s.d_codes.data_ptr(), infos=infos, tptrs=tptrs, tbytes=tbytes, raw=raw,
             n_elems=n, e=e, index=d_index.data_ptr(), stride=1, row_elems=7, n_rows=2, out=d_out.data_ptr(), out_stride=28,
             status=d_status.data_ptr(), null=()):
        arr = lambda t, v: None if v is None else (t * len(v))(*v)
        return L.ghf_decode_planes_gather(ctx_h, None if "ptrs" in null else arr(C.c_void_p, ptrs),
                                          None if "sizes" in null else arr(C.c_size_t, sizes), codes,
                                          None if "infos" in null else (ghf.SeekInfo * len(infos))(*infos),
                                          None if "tptrs" in null else arr(C.c_void_p, tptrs),
                                          None if "tbytes" in null else arr(C.c_size_t, tbytes), raw, n_elems, e, index, stride, row_elems,
                                          n_rows, out, out_stride, status)

    def off(v, i, by):
        return [x + by if j == i else x for j, x in enumerate(v)]

    wrong_n = [ghf.SeekInfo(i.n_symbols + 1, i.n_blocks, i.flags, i.version) for i in infos]
    refusals = [
        ("null context", dict(ctx_h=None), E_INVAL),
        ("elem_bytes 3", dict(e=3), E_INVAL), ("elem_bytes 16", dict(e=16), E_INVAL), ("elem_bytes 0", dict(e=0), E_INVAL),
        ("a raw bit at elem_bytes", dict(raw=raw | 1 << e), E_INVAL),
        ("row_elems 0", dict(row_elems=0), E_INVAL),
        ("row_elems above the cap", dict(row_elems=gm.MAX_ROW_ELEMS + 1, out_stride=(gm.MAX_ROW_ELEMS + 1) * e), E_INVAL),
        ("out_stride below the row", dict(out_stride=27), E_INVAL),
        ("null stream array", dict(null=("ptrs",)), E_INVAL), ("null size array", dict(null=("sizes",)), E_INVAL),
        ("null codes", dict(codes=None), E_INVAL), ("null infos", dict(null=("infos",)), E_INVAL),
        ("null table array", dict(null=("tptrs",)), E_INVAL), ("null table sizes", dict(null=("tbytes",)), E_INVAL),
        ("null index", dict(index=None), E_INVAL), ("null out", dict(out=None), E_INVAL), ("null status", dict(status=None), E_INVAL),
        ("null stream", dict(ptrs=[None] + ptrs[1:]), E_INVAL), ("misaligned stream", dict(ptrs=off(ptrs, 1, 8)), E_INVAL),
        ("null table", dict(tptrs=[None] + tptrs[1:]), E_INVAL), ("misaligned table", dict(tptrs=off(tptrs, 0, 8)), E_INVAL),
        ("misaligned out", dict(out=d_out.data_ptr() + 4), E_INVAL), ("misaligned codes", dict(codes=s.d_codes.data_ptr() + 4), E_INVAL),
        ("misaligned index", dict(index=d_index.data_ptr() + 4), E_INVAL), ("misaligned status", dict(status=d_status.data_ptr() + 2), E_INVAL),
        ("a raw stream that is not n_elems long", dict(sizes=off(a["stream_bytes"], 2, -1)), E_INVAL),
        ("a table of another n_symbols", dict(infos=[wrong_n[0]] + infos[1:]), E_INVAL),
        ("table bytes that do not match the header", dict(tbytes=off(tbytes, 1, 24)), E_FORMAT),
    ]
    for what, kw, rc in refusals:
        assert call(**kw) == rc, what
    # a raw plane's table, info and code entries are not read: plane 2's are null / zero here
    assert tptrs[2] == 0 and tbytes[2] == 0
    assert call(n_rows=0) == OK
    ctx.sync()
    assert L.ghf_status(ctx.h) == OK
    assert bool((d_out == GUARD).all()) and bool((d_status == -1).all()), "a refused call, or one of no rows, queued something"
    assert call() == OK  # the same arguments, accepted
    ctx.sync()
    assert [int(v) for v in d_status.cpu()] == [OK, OK]
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:28], s.t.rows([0], 1, 7)[0]) and np.array_equal(got[28:56], s.t.rows([5], 1, 7)[0])
    assert bool((got[56:] == GUARD).all())


# ---------------------------------------------------------------- 6. with the library's own streams and tables
@pytest.mark.parametrize("e", (2, 4))
def test_through_compress_planes_forms_and_seek_pack(env, e):
    ghf, ctx, torch = env
    t = gp.tensor(e)
    n = t.n
    r = ctx.compress_planes_forms(to_dev(torch, t.bytes), e, raw_planes=ghf.RAW_AUTO, sparse_planes=0, indexes=True)
    ctx.sync()
    assert r["sparse_planes"] == 0 and r["raw_planes"] == t.raw_auto
    sizes = [int(v) for v in r["out_bytes"].cpu().numpy()][:e]
    streams = [r["out"][p * r["slot_bytes"] :][: sizes[p]] for p in range(e)]
    infos, d_tables = [None] * e, [None] * e
    for p in range(e):
        if not r["raw_planes"] >> p & 1:
            d_table = ctx.seek_pack(r["indexes"][p])
            ctx.sync()
            host = d_table.cpu().numpy().copy()
            assert np.array_equal(host, t.planes[p].table), "ghf_seek_pack and expected_table disagree"
            infos[p], d_tables[p] = ghf.seek_parse(host), to_dev(torch, host)
    ids = [3, 0, (n - 513) // 513, 3, 7]
    d_out, d_status = ctx.decode_planes_gather(streams, sizes, r["codes"], r["raw_planes"], n, e, to_dev(torch, np.array(ids, dtype=np.int64)),
                                               513, infos=infos, d_tables=d_tables)
    ctx.sync()
    ctx.planes_index_free(r["indexes"])
    assert [int(v) for v in d_status.cpu()] == [OK] * len(ids)
    assert np.array_equal(d_out.cpu().numpy(), np.concatenate(t.rows(ids, 513, 513)))
