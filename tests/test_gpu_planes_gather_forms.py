"""GPU: ghf_decode_planes_gather_forms, bit-exact against numpy slices of the tensor.

Streams, codes, seek tables and rank tables are the oracle's, range_worlds.expected_table's and sparse_range_model.table_of's
(tests/gather_forms_planes.py), so k_decode_planes_gather_forms is the only device code here; one test goes through
ghf_compress_planes_forms + ghf_seek_pack to hold the product's own output against the call.  Every stream, table, rank table
and raw plane and the base lie in a guarded arena (tests/guarded.py) at exactly their sizes, and so does the output: the bytes
around it and the padding between its rows must keep the fill pattern.  Expected verdicts and rows come from
tests/gather_forms_model.py; for intact inputs the rows are also held against plain slices of the tensor."""
import ctypes as C

import numpy as np
import pytest

import gather_forms_model as fm
import gather_forms_planes as fp
import gather_model as gm
import gather_planes as gp
import pkgload
import sparse_range_model as srm
from guarded import GUARD, Arena, first_diff

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_FORMAT, E_CORRUPT = fm.OK, fm.E_INVAL, fm.E_FORMAT, fm.E_CORRUPT
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


def guarded_copy(torch, host):
    """a host array on the device at exactly its size, guards around it, 16-byte aligned"""
    d = torch.full((host.size + 128,), GUARD, dtype=torch.uint8, device="cuda")
    d[64 : 64 + host.size].copy_(to_dev(torch, host))
    assert d.data_ptr() % 16 == 0
    return d[64 : 64 + host.size]


class Stored:
    """a tensor of gather_forms_planes on the device: per slot its stream (a raw plane: the plane) and seek table, per sparse
    plane its rank table image, and the base, each at exactly its size in one guarded arena; the codes as the oracle built them"""

    def __init__(self, ghf, torch, t):
        self.t, self.e, self.n = t, t.e, t.n
        e = t.e
        self.src = [None] * (2 * e)  # per slot: the fp.Stream, or the raw plane's bytes
        for i, p in enumerate(t.planes):
            self.src[i] = p.data if p.kind == "raw" else p.main
            self.src[e + i] = p.values
        self.arena = Arena()
        host = lambda s: s if isinstance(s, np.ndarray) else s.stream
        self.k_stream = [None if s is None else self.arena.add(host(s).size) for s in self.src]
        self.k_table = [None if s is None or isinstance(s, np.ndarray) else self.arena.add(s.table.size) for s in self.src]
        self.k_rank = [None if p.kind != "sparse" else self.arena.add(p.rank.size) for p in t.planes]
        self.k_base = self.arena.add(t.base.size)
        self.arena.alloc(torch)
        for j, s in enumerate(self.src):
            if s is not None:
                self.arena.view(self.k_stream[j]).copy_(to_dev(torch, host(s)))
            if self.k_table[j] is not None:
                self.arena.view(self.k_table[j]).copy_(to_dev(torch, s.table))
        for i, p in enumerate(t.planes):
            if p.kind == "sparse":
                self.arena.view(self.k_rank[i]).copy_(to_dev(torch, p.rank))
        self.arena.view(self.k_base).copy_(to_dev(torch, t.base))
        self.infos = [None if k is None else ghf.seek_parse(self.src[j].table) for j, k in enumerate(self.k_table)]
        self.rank_infos = [None if p.kind != "sparse" else ghf.sparse_rank_parse(p.rank) for p in t.planes]
        blank = bytes(C.sizeof(ghf.Code))
        self.codes = [blank if k is None else bytes(self.src[j].code) for j, k in enumerate(self.k_table)]
        self.d_codes = to_dev(torch, np.frombuffer(b"".join(self.codes), dtype=np.uint8))

    def args(self, with_base, tables=None, stream_bytes=None, ranks=None, d_codes=None, streams=None):
        """what Context.decode_planes_gather_forms takes for this tensor; tables / stream_bytes / streams: {slot: a damaged table
        on the device / a cut size / another stream}; ranks: {plane: a damaged rank table image on the device}"""
        e = self.e
        v = lambda k: None if k is None else self.arena.view(k)
        d_streams = [v(k) for k in self.k_stream]
        sizes = [0 if k is None else self.arena.regions[k][1] for k in self.k_stream]
        d_tables = [v(k) for k in self.k_table]
        for j, tb in (tables or {}).items():
            d_tables[j] = tb
        for j, sb in (stream_bytes or {}).items():
            sizes[j] = sb
        for j, st in (streams or {}).items():
            d_streams[j], sizes[j] = st, st.numel()
        rk = [None if k is None else (self.rank_infos[i], v(k)) for i, k in enumerate(self.k_rank)]
        for i, r in (ranks or {}).items():
            rk[i] = (self.rank_infos[i], r)
        return dict(streams=d_streams, stream_bytes=sizes, d_codes=self.d_codes if d_codes is None else d_codes, raw_planes=self.t.raw,
                    sparse_planes=self.t.sparse, ranks=rk, n_elems=self.n, elem_bytes=e, infos=list(self.infos), d_tables=d_tables,
                    d_base=v(self.k_base) if with_base else None)


@pytest.fixture(scope="module")
def stored(env):
    ghf, ctx, torch = env
    cache = {}

    def get(e):
        if e not in cache:
            cache[e] = Stored(ghf, torch, fp.tensor(e))
        return cache[e]

    return get


def gather(env, s, with_base, indices, index_stride, row_elems, out_stride=None, **damage):
    """one call into a guarded output -> (the output rows as they came back, the statuses, whether every byte around the
    output and around the stored tensor kept the fill pattern).  The context's status must still be GHF_OK."""
    ghf, ctx, torch = env
    e = s.e
    out_stride = row_elems * e if out_stride is None else out_stride
    n_rows = len(indices)
    arena = Arena()
    k = arena.add(n_rows * out_stride)
    arena.alloc(torch)
    d_index = to_dev(torch, np.asarray(indices, dtype=np.uint64).view(np.int64))
    d_status = torch.full((n_rows,), -1, dtype=torch.int32, device="cuda")
    ctx.decode_planes_gather_forms(d_index=d_index, row_elems=row_elems, index_stride=index_stride, d_out=arena.view(k), out_stride=out_stride,
                                   d_row_status=d_status, **s.args(with_base, **damage))
    ctx.sync()  # raises if anything latched
    assert ghf.lib().ghf_status(ctx.h) == OK
    intact = arena.fetch() and s.arena.fetch()
    return arena.got(k).reshape(n_rows, out_stride), [int(v) for v in d_status.cpu().numpy()], intact


def check(env, s, with_base, indices, index_stride, row_elems, out_stride=None, planes=None, want_status=None, neighbours_intact=True,
          **damage):
    """the call against the model: the statuses are the model's, rows whose status is GHF_OK hold the model's bytes -- for an
    intact tensor also the plain slice of `new` (with a base) or of the delta -- and every other byte of the output the fill"""
    e = s.e
    intact_input = planes is None
    planes = s.t.model_planes() if planes is None else planes
    got, status, intact = gather(env, s, with_base, indices, index_stride, row_elems, out_stride, **damage)
    model_status = [fm.row_verdict(i, index_stride, row_elems, s.n, planes) for i in indices]
    if want_status is not None:
        assert model_status == want_status, (model_status, want_status)  # the case is what its comment says
    assert status == model_status, (e, with_base, row_elems, index_stride, status, model_status)
    want = np.full(got.size, GUARD, dtype=np.uint8)
    fm.expected_rows(planes, s.n, s.t.base if with_base else None, indices, index_stride, row_elems, model_status, want, got.shape[1])
    want = want.reshape(got.shape)
    if intact_input or neighbours_intact:  # the rows that are served are the tensor's: a damaged case has truly intact neighbours
        for r, (i, st) in enumerate(zip(indices, model_status)):
            if st == OK:
                assert np.array_equal(want[r, : row_elems * e], s.t.rows([i], index_stride, row_elems, with_base)[0])
    assert np.array_equal(got, want), (e, with_base, row_elems, index_stride, first_diff(got.reshape(-1), want.reshape(-1)))
    assert intact, "a byte outside the output rows, or of a stream, table or the base, was written"


# ---------------------------------------------------------------- 1. row shapes, with a base and without
@pytest.mark.parametrize("with_base", (False, True))
@pytest.mark.parametrize("e", WIDTHS)
def test_row_shapes_in_every_form(env, stored, e, with_base):
    s = stored(e)
    for row_elems, firsts in fp.row_cases(s.t):
        check(env, s, with_base, firsts, 1, row_elems, want_status=[OK] * len(firsts))
    # by row id, padded rows: rows 0, 1, the last whole one, one repeated
    for row_elems in (7, 513, 4096):
        ids = [s.n // row_elems - 1, 1, 0, 1]
        check(env, s, with_base, ids, row_elems, row_elems, row_elems * e + 5, want_status=[OK] * 4)


def test_misaligned_rows_and_padding(env, stored):
    s = stored(2)
    ids = [32765, 0, fp.RUN_AT + 505, 32765, s.n - 7]
    for with_base in (False, True):
        check(env, s, with_base, ids, 1, 7, 14)  # seven bf16 elements: rows 14 bytes apart, all but the first misaligned
        check(env, s, with_base, ids, 1, 7, 14 + 3)
        check(env, s, with_base, ids, 1, 7, 14 + 19)


# ---------------------------------------------------------------- 2. identity with the parent call
@pytest.mark.parametrize("e", WIDTHS)
def test_without_sparse_planes_and_base_the_parent_call_is_reproduced_byte_for_byte(env, e):
    ghf, ctx, torch = env
    cases = [(gp.N_SMALL, 7, 1, [4090, 0, 505, gp.N_SMALL - 7, gp.N_SMALL, 1 << 63]), (gp.N_SMALL, 513, 513, [3, 0, 24, 3]),
             (gp.N_SMALL, 4097, 1, [4097, 0, gp.N_SMALL - 4097])]
    if e == 2:
        cases.append((gp.N_CAP, gm.MAX_ROW_ELEMS, 1, [700, 0]))
    for n, row_elems, stride, ids in cases:
        t = gp.tensor(e, n)
        for raw in dict.fromkeys([0, t.raw_auto | 1]):
            streams = [to_dev(torch, p.data if raw >> i & 1 else p.stream) for i, p in enumerate(t.planes)]
            sizes = [int(x.numel()) for x in streams]
            d_tables = [None if raw >> i & 1 else to_dev(torch, p.table) for i, p in enumerate(t.planes)]
            infos = [None if raw >> i & 1 else ghf.seek_parse(p.table) for i, p in enumerate(t.planes)]
            d_codes = to_dev(torch, np.frombuffer(b"".join(bytes(p.code) for p in t.planes) * 2, dtype=np.uint8))
            d_index = to_dev(torch, np.asarray(ids, dtype=np.uint64).view(np.int64))
            outs = []
            for forms in (False, True):
                d_out = torch.full((len(ids) * row_elems * e,), GUARD, dtype=torch.uint8, device="cuda")
                d_status = torch.full((len(ids),), -1, dtype=torch.int32, device="cuda")
                if forms:
                    ctx.decode_planes_gather_forms(streams + [None] * e, sizes + [0] * e, d_codes, raw, 0, None, n, e, d_index, row_elems,
                                                   index_stride=stride, infos=infos + [None] * e, d_tables=d_tables + [None] * e,
                                                   d_out=d_out, d_row_status=d_status)
                else:
                    ctx.decode_planes_gather(streams, sizes, d_codes, raw, n, e, d_index, row_elems, index_stride=stride, infos=infos,
                                             d_tables=d_tables, d_out=d_out, d_row_status=d_status)
                ctx.sync()
                outs.append((d_out.cpu().numpy(), d_status.cpu().numpy()))
            assert np.array_equal(outs[0][1], outs[1][1]), (e, n, row_elems, raw)
            assert np.array_equal(outs[0][0], outs[1][0]), (e, n, row_elems, raw, first_diff(outs[0][0], outs[1][0]))
            assert (outs[0][1] == OK).sum() >= 2


# ---------------------------------------------------------------- 3. per-row verdicts
def first_plane(t, form):
    return next(i for i, p in enumerate(t.planes) if p.form == form)


def with_plane(t, i, model):
    planes = t.model_planes()
    planes[i] = model
    return planes


@pytest.mark.parametrize("e", WIDTHS)
def test_rows_outside_the_tensor(env, stored, e):
    s = stored(e)
    n = s.n
    ids = [0, n // 4 + 10, (n - 4) // 4, 1 << 63, 5, n // 4 - 2]  # stride 4: ok, past the end, passes n, overflows, ok, ok
    check(env, s, True, ids, 4, 7, want_status=[OK, E_INVAL, E_INVAL, E_INVAL, OK, OK])


@pytest.mark.parametrize("e", WIDTHS)
def test_a_rank_entry_raised_by_one(env, stored, e):
    """cum[1] + 1: seen by every row whose decoded mask holds block 0 or block 1 to its end; the rows at the start of block 0
    and in block 2 read other entries and are served"""
    ghf, ctx, torch = env
    s = stored(e)
    i = first_plane(s.t, "r" if e != 4 else "s")
    p = s.t.planes[i]
    rank = p.rank.copy()
    cum = srm.cum_in(rank).copy()
    cum[1] += 1
    rank[srm.HEADER_BYTES :] = np.frombuffer(cum.astype("<u8").tobytes(), dtype=np.uint8)
    ids = [100, 32768 - 513, 32768 - 100, 65536 - 513, 65536 + 10, 0]
    check(env, s, True, ids, 1, 513, planes=with_plane(s.t, i, p.model(cum=cum)), ranks={i: guarded_copy(torch, rank)},
          want_status=[OK, E_CORRUPT, E_CORRUPT, E_CORRUPT, OK, OK])


@pytest.mark.parametrize("e", WIDTHS)
def test_two_rank_entries_out_of_order(env, stored, e):
    ghf, ctx, torch = env
    s = stored(e)
    i = first_plane(s.t, "r" if e != 4 else "s")
    p = s.t.planes[i]
    rank = p.rank.copy()
    cum = srm.cum_in(rank).copy()
    cum[1], cum[2] = cum[2], cum[1]
    assert cum[1] > cum[2]
    rank[srm.HEADER_BYTES :] = np.frombuffer(cum.astype("<u8").tobytes(), dtype=np.uint8)
    # in block 1; in block 0, whose decoded mask does not reach the swapped entry; across the edge; repeated; block 0 again
    ids = [40000, 100, 32768 - 3, 40000, 5000]
    check(env, s, False, ids, 1, 7, planes=with_plane(s.t, i, p.model(cum=cum)), ranks={i: guarded_copy(torch, rank)},
          want_status=[E_CORRUPT, OK, E_CORRUPT, E_CORRUPT, OK])


@pytest.mark.parametrize("e", WIDTHS)
def test_a_set_pad_bit(env, stored, e):
    """the mask stream holds a last byte with bit 6 set (n % 8 == 5); only rows that touch that byte see it"""
    ghf, ctx, torch = env
    s = stored(e)
    i = first_plane(s.t, "s" if e != 2 else "r")
    p = s.t.planes[i]
    mask = p.mask.copy()
    mask[-1] |= 1 << 6
    padded = fp.Plane(p.form, p.data, mask=mask)
    assert padded.main.table.size == p.main.table.size
    d_codes = s.d_codes.clone()
    sz = C.sizeof(ghf.Code)
    d_codes[i * sz : (i + 1) * sz] = to_dev(torch, np.frombuffer(bytes(padded.main.code), dtype=np.uint8))
    ids = [s.n - 7, s.n - 8 - 7, 0, s.n - 7 - 3, 65536]
    check(env, s, True, ids, 1, 7, planes=with_plane(s.t, i, padded.model()), streams={i: guarded_copy(torch, padded.main.stream)},
          tables={i: guarded_copy(torch, padded.main.table)}, d_codes=d_codes, want_status=[E_CORRUPT, OK, OK, E_CORRUPT, OK])


def damaged_table(stream, edits):
    t = stream.table.copy()
    rec = np.frombuffer(t[gm.HEADER :].tobytes(), dtype=gm.REC).copy()
    for (g, k), d in edits.items():
        rec["run"][g][k] = int(rec["run"][g][k]) + d
    t[gm.HEADER :] = np.frombuffer(rec.tobytes(), dtype=np.uint8)
    return t


@pytest.mark.parametrize("e", WIDTHS)
def test_a_damaged_mask_run(env, stored, e):
    """run 3 of the mask's seek block 1 (rank block 1, elements 32768 + [12288, 16384)) one bit longer: the chain to the next
    block breaks, so every row that touches rank block 1 fails; rows inside rank blocks 0 and 2 are served"""
    ghf, ctx, torch = env
    s = stored(e)
    i = first_plane(s.t, "r" if e != 4 else "s")
    p = s.t.planes[i]
    t = damaged_table(p.main, {(1, 3): +1})
    ids = [32768 + 12288 + 5, 32768 + 100, 100, 65536 + 10, 32768 - 100, 65536 - 600]
    check(env, s, True, ids, 1, 513, planes=with_plane(s.t, i, p.model(mask_stream=p.main.model(table=t))), tables={i: guarded_copy(torch, t)},
          want_status=[E_CORRUPT, E_CORRUPT, OK, OK, E_CORRUPT, E_CORRUPT])


@pytest.mark.parametrize("e", (2, 8))
def test_a_damaged_values_run(env, stored, e):
    """two run lengths of the values stream of the `r` plane that keep the chain: rows whose values lie in those runs fail"""
    ghf, ctx, torch = env
    s = stored(e)
    i = first_plane(s.t, "r")
    p = s.t.planes[i]
    t = damaged_table(p.values, {(1, 2): +1, (1, 3): -1})  # values [5120, 6144)
    f_bad = fp.RUN_AT + (4096 + 2 * 512 + 100 - fp.rank_in(p, fp.RUN_AT))  # inside the run a rank per element
    assert fp.RUN_AT <= f_bad < fp.RUN_AT + fp.RUN_LEN - 1100 and fp.rank_in(p, f_bad) == 4096 + 2 * 512 + 100
    ids = [f_bad, 100, f_bad + 512, fp.RUN_AT + 8, s.n - 513, f_bad - 300]
    planes = with_plane(s.t, i, p.model(vals_stream=p.values.model(table=t)))
    want = [fm.row_verdict(f, 1, 513, s.n, planes) for f in ids]
    assert want[0] == E_CORRUPT and want[1] == OK and want.count(E_CORRUPT) >= 2 and want.count(OK) >= 2
    check(env, s, False, ids, 1, 513, planes=planes, tables={e + i: guarded_copy(torch, t)})


@pytest.mark.parametrize("e", (2, 8))
def test_a_values_stream_cut_short(env, stored, e):
    ghf, ctx, torch = env
    s = stored(e)
    i = first_plane(s.t, "r")
    p = s.t.planes[i]
    rec = gm.records(p.values.table)
    last = rec.size - 1
    cut = (int(rec[last]["start"]) + int(rec[last]["run"][0]) // 2) // 8  # ends inside run 0 of the values' last block
    assert 8 * cut >= int(rec[last]["start"]) and cut < p.values.stream_bytes
    ids = [100, s.n - 4096, fp.RUN_AT, 65536 + 3000, 0]
    planes = with_plane(s.t, i, p.model(vals_stream=p.values.model(stream_bytes=cut)))
    want = [fm.row_verdict(f, 1, 4096, s.n, planes) for f in ids]
    assert want[0] == OK and want[1] == E_CORRUPT and want[2] == OK
    check(env, s, True, ids, 1, 4096, planes=planes, stream_bytes={e + i: cut})


@pytest.mark.parametrize("e", WIDTHS)
def test_an_incomplete_code(env, stored, e):
    """of a values stream, then of a mask stream: GHF_E_FORMAT on every row, even on one outside the tensor"""
    ghf, ctx, torch = env
    s = stored(e)
    i = first_plane(s.t, "r" if e != 4 else "s")
    sz = C.sizeof(ghf.Code)
    for slot in (e + i, i):
        bad = s.d_codes.clone().cpu().numpy()
        code = ghf.Code.from_buffer_copy(bad[slot * sz : (slot + 1) * sz].tobytes())
        sym = next(v for v in range(256) if code.length[v] == code.max_len)
        code.length[sym] -= 1  # the lengths no longer satisfy Kraft with equality
        bad[slot * sz : (slot + 1) * sz] = np.frombuffer(bytes(code), dtype=np.uint8)
        p = s.t.planes[i]
        broken = p.main.model(code_ok=False) if slot == i else p.values.model(code_ok=False)
        model = p.model(mask_stream=broken) if slot == i else p.model(vals_stream=broken)
        check(env, s, True, [0, 100, s.n, 40000], 1, 7, planes=with_plane(s.t, i, model), d_codes=to_dev(torch, bad),
              want_status=[E_FORMAT] * 4)


# ---------------------------------------------------------------- 4. call-level refusals
def test_call_level_refusals_queue_nothing_and_leave_the_status_alone(env, stored):
    ghf, ctx, torch = env
    s = stored(4)  # forms "swzd": sparse 0b0101, raw 0b0010; slot 6 (the values of the all-zero plane) is empty
    L, n, e = ghf.lib(), s.n, 4
    a = s.args(True)
    raw, sparse = a["raw_planes"], a["sparse_planes"]
    assert (raw, sparse) == (0b0010, 0b0101) and s.t.planes[2].n_vals == 0
    ptrs = [0 if x is None else x.data_ptr() for x in a["streams"]]
    tptrs = [0 if x is None else x.data_ptr() for x in a["d_tables"]]
    infos = [ghf.SeekInfo() if i is None else i for i in a["infos"]]
    tbytes = [0 if i is None else ghf.seek_bytes(i.n_symbols) for i in a["infos"]]
    rinfos = [ghf.SparseRankInfo() if r is None else r[0] for r in a["ranks"]]
    rptrs = [0 if r is None else r[1].data_ptr() for r in a["ranks"]]
    rbytes = [0 if r is None else r[1].numel() for r in a["ranks"]]
    d_index = to_dev(torch, np.array([0, 5], dtype=np.int64))
    d_out = torch.full((2 * 64 + 64,), GUARD, dtype=torch.uint8, device="cuda")
    d_status = torch.full((2,), -1, dtype=torch.int32, device="cuda")

    def call(ctx_h=ctx.h, ptrs=ptrs, sizes=a["stream_bytes"], codes=s.d_codes.data_ptr(), infos=infos, tptrs=tptrs, tbytes=tbytes,
             rinfos=rinfos, rptrs=rptrs, rbytes=rbytes, base=a["d_base"].data_ptr(), raw=raw, sparse=sparse, n_elems=n, e=e,
             index=d_index.data_ptr(), stride=1, row_elems=7, n_rows=2, out=d_out.data_ptr(), out_stride=28, status=d_status.data_ptr(), null=()):
        arr = lambda t, v: (t * len(v))(*v)
        pick = lambda name, v: None if name in null else v
        return L.ghf_decode_planes_gather_forms(ctx_h, pick("ptrs", arr(C.c_void_p, ptrs)), pick("sizes", arr(C.c_size_t, sizes)), codes,
                                                pick("infos", (ghf.SeekInfo * len(infos))(*infos)), pick("tptrs", arr(C.c_void_p, tptrs)),
                                                pick("tbytes", arr(C.c_size_t, tbytes)), pick("rinfos", (ghf.SparseRankInfo * len(rinfos))(*rinfos)),
                                                pick("rptrs", arr(C.c_void_p, rptrs)),
                                                pick("rbytes", arr(C.c_size_t, rbytes)), base, raw, sparse, n_elems, e, index, stride, row_elems,
                                                n_rows, out, out_stride, status)

    def off(v, i, by):
        return [x + by if j == i else x for j, x in enumerate(v)]

    def info_n(v, i, by):
        return [ghf.SeekInfo(x.n_symbols + by, x.n_blocks, x.flags, x.version) if j == i else x for j, x in enumerate(v)]

    wrong_rank_n = [ghf.SparseRankInfo(r.n + 1, r.n_vals, r.n_blocks, r.version, 0) if j == 0 else r for j, r in enumerate(rinfos)]
    refusals = [
        # the parent's, in its order, over the planes' own slots
        ("null context", dict(ctx_h=None), E_INVAL),
        ("elem_bytes 3", dict(e=3), E_INVAL), ("elem_bytes 16", dict(e=16), E_INVAL), ("elem_bytes 0", dict(e=0), E_INVAL),
        ("a raw bit at elem_bytes", dict(raw=raw | 1 << e), E_INVAL), ("GHF_RAW_AUTO", dict(raw=ghf.RAW_AUTO), E_INVAL),
        ("row_elems 0", dict(row_elems=0), E_INVAL),
        ("row_elems above the sparse cap", dict(row_elems=fm.SPARSE_MAX_ROW_ELEMS + 1, out_stride=(fm.SPARSE_MAX_ROW_ELEMS + 1) * e), E_INVAL),
        ("row_elems above the cap", dict(sparse=0, row_elems=gm.MAX_ROW_ELEMS + 1, out_stride=(gm.MAX_ROW_ELEMS + 1) * e), E_INVAL),
        ("out_stride below the row", dict(out_stride=27), E_INVAL),
        ("null stream array", dict(null=("ptrs",)), E_INVAL), ("null size array", dict(null=("sizes",)), E_INVAL),
        ("null codes", dict(codes=None), E_INVAL), ("null infos", dict(null=("infos",)), E_INVAL),
        ("null table array", dict(null=("tptrs",)), E_INVAL), ("null table sizes", dict(null=("tbytes",)), E_INVAL),
        ("null index", dict(index=None), E_INVAL), ("null out", dict(out=None), E_INVAL), ("null status", dict(status=None), E_INVAL),
        ("null stream", dict(ptrs=[None] + ptrs[1:]), E_INVAL), ("misaligned stream", dict(ptrs=off(ptrs, 1, 8)), E_INVAL),
        ("null table", dict(tptrs=[None] + tptrs[1:]), E_INVAL), ("misaligned table", dict(tptrs=off(tptrs, 0, 8)), E_INVAL),
        ("misaligned out", dict(out=d_out.data_ptr() + 4), E_INVAL), ("misaligned codes", dict(codes=s.d_codes.data_ptr() + 4), E_INVAL),
        ("misaligned index", dict(index=d_index.data_ptr() + 4), E_INVAL), ("misaligned status", dict(status=d_status.data_ptr() + 2), E_INVAL),
        ("a raw stream that is not n_elems long", dict(sizes=off(a["stream_bytes"], 1, -1)), E_INVAL),
        ("a dense table of another n_symbols", dict(infos=info_n(infos, 3, 1)), E_INVAL),
        ("table bytes that do not match the header", dict(tbytes=off(tbytes, 3, 24)), E_FORMAT),
        ("a mask's table bytes that do not match the header", dict(tbytes=off(tbytes, 0, 24)), E_FORMAT),
        # the masks
        ("a plane named in both masks", dict(sparse=sparse | raw), E_INVAL), ("GHF_SPARSE_AUTO", dict(sparse=ghf.SPARSE_AUTO), E_INVAL),
        ("an AUTO bit beside plane bits", dict(sparse=sparse | ghf.SPARSE_AUTO), E_INVAL),
        ("a sparse bit at elem_bytes", dict(sparse=sparse | 1 << e), E_INVAL),
        # the rank tables
        ("null rank infos", dict(null=("rinfos",)), E_INVAL), ("null rank pointers", dict(null=("rptrs",)), E_INVAL),
        ("null rank sizes", dict(null=("rbytes",)), E_INVAL),
        ("null rank table", dict(rptrs=[None] + rptrs[1:]), E_INVAL), ("misaligned rank table", dict(rptrs=off(rptrs, 2, 4)), E_INVAL),
        ("rank bytes of another n", dict(rbytes=off(rbytes, 0, 8)), E_INVAL),
        ("a rank info of another n", dict(rinfos=wrong_rank_n), E_INVAL),
        ("a mask table of another n_symbols", dict(infos=info_n(infos, 2, 1), tbytes=off(tbytes, 2, 0)), E_INVAL),
        # the values
        ("null values stream", dict(ptrs=off(ptrs, e, -ptrs[e])), E_INVAL), ("misaligned values table", dict(tptrs=off(tptrs, e, 8)), E_INVAL),
        ("a values table of another n_symbols", dict(infos=info_n(infos, e, -1)), E_INVAL),
        ("values table bytes that do not match the header", dict(tbytes=off(tbytes, e, 24)), E_FORMAT),
    ]
    for what, kw, rc in refusals:
        assert call(**kw) == rc, what
    # the empty slots are not read: the values of the all-zero plane and the upper slots of the raw and the dense plane are null
    assert ptrs[6] == 0 and tptrs[6] == 0 and ptrs[5] == 0 and ptrs[7] == 0 and tptrs[1] == 0
    assert call(n_rows=0) == OK
    ctx.sync()
    assert L.ghf_status(ctx.h) == OK
    assert bool((d_out == GUARD).all()) and bool((d_status == -1).all()), "a refused call, or one of no rows, queued something"
    assert call() == OK  # the same arguments, accepted
    ctx.sync()
    assert [int(v) for v in d_status.cpu()] == [OK, OK]
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:28], s.t.rows([0], 1, 7, True)[0]) and np.array_equal(got[28:56], s.t.rows([5], 1, 7, True)[0])
    assert bool((got[56:] == GUARD).all())
    # the base is read byte by byte: no alignment is asked of it.  One element further on, the rows are XORed with the next element's
    assert call(base=a["d_base"].data_ptr() + e) == OK
    ctx.sync()
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:28], s.t.delta[: 7 * e] ^ s.t.base[e : 8 * e]) and [int(v) for v in d_status.cpu()] == [OK, OK]


# ---------------------------------------------------------------- 5. with the library's own streams and tables
@pytest.mark.parametrize("e", (2, 4))
def test_through_compress_planes_forms_and_seek_pack(env, e):
    ghf, ctx, torch = env
    t = fp.tensor(e)
    n = t.n
    d_base = to_dev(torch, t.base)
    r = ctx.compress_planes_forms(to_dev(torch, t.new), e, raw_planes=ghf.RAW_AUTO, sparse_planes=ghf.SPARSE_AUTO, d_base=d_base, indexes=True,
                                  ranks=True)
    ctx.sync()
    assert r["sparse_planes"] == t.sparse and r["raw_planes"] == t.raw  # the product chooses the forms the tensor was built in
    sizes = [int(v) for v in r["out_bytes"].cpu().numpy()]
    streams = [r["out"][j * r["slot_bytes"] :][: sizes[j]] if sizes[j] else None for j in range(2 * e)]
    infos, d_tables = [None] * (2 * e), [None] * (2 * e)
    for j in range(2 * e):
        p = j % e
        if sizes[j] and not r["raw_planes"] >> p & 1:
            d_table = ctx.seek_pack(r["indexes"][j])
            ctx.sync()
            host = d_table.cpu().numpy().copy()
            src = t.planes[p].main if j < e else t.planes[p].values
            assert np.array_equal(host, src.table), "ghf_seek_pack and expected_table disagree"
            infos[j], d_tables[j] = ghf.seek_parse(host), to_dev(torch, host)
    ranks = [None] * e
    for p in range(e):
        if r["sparse_planes"] >> p & 1:
            img = r["ranks"][p * r["rank_slot_bytes"] :][: ghf.sparse_rank_bytes(n)]
            host = img.cpu().numpy().copy()
            assert np.array_equal(host, t.planes[p].rank)
            ranks[p] = (ghf.sparse_rank_parse(host), img)
    ids = [3, 0, (n - 513) // 513, 3, 63, 64]
    d_out, d_status = ctx.decode_planes_gather_forms(streams, sizes, r["codes"], r["raw_planes"], r["sparse_planes"], ranks, n, e,
                                                     to_dev(torch, np.array(ids, dtype=np.int64)), 513, infos=infos, d_tables=d_tables,
                                                     d_base=d_base)
    ctx.sync()
    ctx.planes_index_free(r["indexes"])
    assert [int(v) for v in d_status.cpu()] == [OK] * len(ids)
    assert np.array_equal(d_out.cpu().numpy(), np.concatenate(t.rows(ids, 513, 513, True)))
