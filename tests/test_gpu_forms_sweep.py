"""GPU: every code shape of the pool through the forms, sparse-range and gather calls -- the families that tests/
test_gpu_code_sweep.py does not reach, with bit walkers of their own: k_seek_expand_streams behind the range calls from seek
tables, and the gather walker on dense planes and on the mask and values streams of sparse ones.

Nothing expected comes from the library.  The tensors are those of tests/forms_sweep.py (and, for ghf_decode_planes_gather,
the typed tensors of tests/code_sweep.py): every stored stream is a pool code's header followed by orc_encode_body, seek
tables are range_worlds.expected_table's, side-cars code_sweep.expected_index's, rank tables sparse_range_model.table_of's,
and every expected byte is a numpy slice of the tensor.  A tensor's stored bytes lie at exactly their sizes in one guarded
arena (tests/guarded.py), every output in another; the guard bytes of both are checked.  Every call here refuses a d_out
that is not 16-byte aligned, so the skew is in the rows: a gather's out_stride is odd, which puts all rows but the first at
odd or unaligned addresses, and its base lies at an odd address.

The images under long codes are larger than ghf_planes_slot_bytes counts (9 bits per symbol): the calls take a pointer and
a size per stream, and nothing refuses them (`warm` holds that such images are among the cases).

The ids say where to look: `E<width>-c<decoder class of plane 0's first stream>`, six tensors each.  A failure names the
case and its planes' code labels, e.g. `E4/case07/ddsz/n.. :: d/<label> | ... | z/<label>`: forms_sweep.cases(4)[7] is that
case alone, on the CPU."""
import ctypes as C

import numpy as np
import pytest

import code_sweep as cs
import forms_sweep as fs
import gather_forms_planes as fp
import gather_planes as gp
import pkgload
from guarded import GUARD, Arena, first_diff
import test_gpu_planes_gather as t_gather
import test_gpu_planes_gather_forms as t_gforms

pytestmark = pytest.mark.gpu

OK, E_INVAL = 0, 1
IDS = [(e, lead) for e in fs.WIDTHS for lead in range(6)]
BIG_ROWS, BIG_ROW_ELEMS, BIG_STRIDE, BIG_BAD_ROW = 65536 + 3, 5, 11, 65537


def id_of(p):
    return "E%d-c%d" % p


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


@pytest.fixture(scope="module", autouse=True)
def sweep():
    """the cases, made once before the first id runs"""
    for e in fs.WIDTHS:
        fs.cases(e)
        fs.typed_rows(e)


def to_dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def filled(torch, arena, fills):
    """arena.alloc with {region: host bytes} already in place: one upload"""
    host = np.full(arena.at, GUARD, dtype=np.uint8)
    for k, data in fills.items():
        off, size = arena.regions[k]
        assert data.size == size
        host[off : off + size] = data
    arena.d = torch.from_numpy(host).cuda()
    assert arena.d.data_ptr() % 16 == 0
    return arena


def cases_of(e, lead):
    out = [c for c in fs.cases(e) if c.lead == lead]
    assert len(out) == fs.FORMS_CASES // 6
    return out


class Dev:
    """a forms_sweep.Case on the device: per slot its image (a raw plane: the plane) and, for a stream with a code, its seek
    table and its side-car; per sparse plane its rank table image; the base at an odd address -- each at exactly its size in
    one guarded arena; the codes as the oracle built them"""

    def __init__(self, env, c):
        ghf, ctx, torch = env
        self.c, self.e, self.n = c, c.e, c.n
        e = c.e
        self.slots = slots = c.slots()
        is_stream = [isinstance(s, fs.Stream) for s in slots]
        a, fills = Arena(), {}

        def put(data, skew=0):
            data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            k = a.add(data.size, skew)
            fills[k] = data
            return k

        self.k_stream = [None if s is None else put(s.image if st else s) for s, st in zip(slots, is_stream)]
        self.k_table = [put(s.table) if st else None for s, st in zip(slots, is_stream)]
        cars = [s.index if st else None for s, st in zip(slots, is_stream)]
        self.k_chunk = [None if x is None else put(x[0]) for x in cars]
        self.k_seg = [None if x is None else put(x[1]) for x in cars]
        self.k_rank = [put(p.rank) if p.kind == "sparse" else None for p in c.planes]
        self.k_base = put(c.base, skew=1)
        self.arena = filled(torch, a, fills)
        v = lambda k: None if k is None else a.view(k)
        self.streams = [v(k) for k in self.k_stream]
        self.sizes = [0 if k is None else a.regions[k][1] for k in self.k_stream]
        self.d_tables = [v(k) for k in self.k_table]
        self.infos = [ghf.seek_parse(s.table) if st else None for s, st in zip(slots, is_stream)]
        self.idx = (ghf.Index * (2 * e))()
        for j, (s, st) in enumerate(zip(slots, is_stream)):
            if st:
                self.idx[j] = ghf.Index(s.n, 4096, 64, -(-s.n // 4096), -(-s.n // 64), 0, 0, v(self.k_chunk[j]).data_ptr(), v(self.k_seg[j]).data_ptr())
        blank = bytes(C.sizeof(ghf.Code))
        self.d_codes = to_dev(torch, np.frombuffer(b"".join(bytes(s.entry.code) if st else blank for s, st in zip(slots, is_stream)), dtype=np.uint8))
        assert self.d_codes.data_ptr() % 16 == 0
        self.n_vals = [p.n_vals for p in c.planes]
        rinfo = [ghf.sparse_rank_parse(p.rank) if p.kind == "sparse" else None for p in c.planes]
        for p, ri in zip(c.planes, rinfo):
            assert ri is None or (ri.n, ri.n_vals) == (c.n, p.n_vals), c
        self.ranks_host = [None if ri is None else (ri, p.rank) for p, ri in zip(c.planes, rinfo)]
        self.ranks_dev = [None if ri is None else (ri, v(k)) for ri, k in zip(rinfo, self.k_rank)]
        self.d_base_odd = v(self.k_base)
        assert self.d_base_odd.data_ptr() % 2 == 1

    def source(self, which):
        return {"indexes": self.idx} if which == "side-cars" else {"infos": self.infos, "d_tables": self.d_tables}

    def inputs_intact(self):
        return self.arena.fetch()


# ------------------------------------------------------------------------------ a. the whole decode
def whole(env, c):
    ghf, ctx, torch = env
    d, nb = Dev(env, c), c.n * c.e
    a = Arena()
    r_out, r_in = a.add(nb), a.add(nb)
    filled(torch, a, {r_in: c.base})
    args = (d.streams, d.sizes, d.d_codes, c.raw, c.sparse, d.n_vals, c.n, c.e)
    _, nb_out = ctx.decode_planes_forms(*args, indexes=d.idx, d_out=a.view(r_out), cap=nb)
    _, nb_in = ctx.decode_planes_forms(*args, indexes=d.idx, d_base=a.view(r_in), d_out=a.view(r_in), cap=nb)
    ctx.sync()
    clean = a.fetch()
    assert int(nb_out.item()) == nb == int(nb_in.item()), (c, "decoded sizes")
    assert np.array_equal(a.got(r_out), c.tensor), (c, "decode_planes_forms without a base", first_diff(a.got(r_out), c.tensor))
    assert np.array_equal(a.got(r_in), c.new), (c, "decode_planes_forms in place", first_diff(a.got(r_in), c.new))
    assert clean and d.inputs_intact(), (c, "guard bytes")


# ------------------------------------------------------------------------------ b. ranges
def ranges(env, c):
    ghf, ctx, torch = env
    d, e = Dev(env, c), c.e
    at, cuts = 0, []
    for first, count in c.ranges:  # the base elements of every range, each part 16-byte aligned in one upload
        cuts.append((at, count * e))
        at += count * e + 15 & ~15
    h_parts = np.zeros(at, dtype=np.uint8)
    for (o, k), (first, count) in zip(cuts, c.ranges):
        h_parts[o : o + k] = c.base[first * e : (first + count) * e]
    d_parts = to_dev(torch, h_parts)
    a = Arena()
    regions = [[[a.add(count * e) for based in (0, 1)] for which in (0, 1)] for first, count in c.ranges]
    r_sparse = a.add(c.ranges[3][1] * e) if not c.raw else None
    a.alloc(torch)
    args = (d.streams, d.sizes, d.d_codes, c.raw, c.sparse, d.ranks_host, c.n, e)
    for (first, count), (o, k), by_source in zip(c.ranges, cuts, regions):
        for which, by_base in zip(("seek tables", "side-cars"), by_source):
            for based, reg in enumerate(by_base):
                ctx.decode_planes_forms_range(*args, first, count, d_base=d_parts[o : o + k] if based else None, d_out=a.view(reg), cap=count * e,
                                              **d.source(which))
    if r_sparse is not None:  # no raw plane: the sparse range call serves the tensor too
        (first, count), (o, k) = c.ranges[3], cuts[3]
        ctx.decode_planes_sparse_range_delta(d.streams, d.sizes, d.d_codes, d_parts[o : o + k], c.sparse, d.ranks_host, c.n, e, first, count,
                                             d_out=a.view(r_sparse), cap=count * e, **d.source("seek tables"))
    ctx.sync()
    clean = a.fetch()
    for (first, count), by_source in zip(c.ranges, regions):
        for which, by_base in zip(("seek tables", "side-cars"), by_source):
            for based, reg in enumerate(by_base):
                want = (c.new if based else c.tensor)[first * e : (first + count) * e]
                assert np.array_equal(a.got(reg), want), (c, "decode_planes_forms_range from " + which, "base" if based else "plain", first, count,
                                                          first_diff(a.got(reg), want))
    if r_sparse is not None:
        first, count = c.ranges[3]
        want = c.new[first * e : (first + count) * e]
        assert np.array_equal(a.got(r_sparse), want), (c, "decode_planes_sparse_range_delta", first, count, first_diff(a.got(r_sparse), want))
    assert clean and d.inputs_intact(), (c, "guard bytes")


# ------------------------------------------------------------------------------ c. and d. the gather calls
def check_rows(what, c, a, reg, d_status, n_rows, firsts, row_bytes, out_stride, src, e):
    status = d_status.cpu().numpy()
    assert status[:n_rows].tolist() == [OK] * n_rows and status[n_rows] == -1, (c, what, status.tolist())
    got = a.got(reg).reshape(n_rows, out_stride)
    want = np.full(got.shape, GUARD, dtype=np.uint8)
    for r, f in enumerate(firsts):
        want[r, :row_bytes] = src[f * e : f * e + row_bytes]
    assert np.array_equal(got, want), (c, what, first_diff(got.reshape(-1), want.reshape(-1)))


def gather_typed(env, case):
    """one launch of ghf_decode_planes_gather over a typed tensor of tests/code_sweep.py"""
    ghf, ctx, torch = env
    t, raw, row_elems, firsts = case
    e, n_rows = t.e, len(firsts)
    tables = [None if raw >> p & 1 else t.table(p) for p in range(e)]
    src, fills = Arena(), {}
    k_stream, k_table = [], []
    for p in range(e):
        data = t.planes[p] if raw >> p & 1 else t.image(p)
        k_stream.append(src.add(data.size))
        fills[k_stream[-1]] = data
        k_table.append(None if tables[p] is None else src.add(tables[p].size))
        if tables[p] is not None:
            fills[k_table[-1]] = tables[p]
    filled(torch, src, fills)
    d_codes = to_dev(torch, np.frombuffer(b"".join(bytes(en.code) for en in t.entries), dtype=np.uint8))
    out_stride = row_elems * e + 3
    a = Arena()
    reg = a.add(n_rows * out_stride)
    a.alloc(torch)
    d_index = to_dev(torch, np.asarray(firsts, dtype=np.int64))
    d_status = torch.full((n_rows + 1,), -1, dtype=torch.int32, device="cuda")
    ctx.decode_planes_gather([src.view(k) for k in k_stream], [src.regions[k][1] for k in k_stream], d_codes, raw, t.n, e, d_index, row_elems,
                             index_stride=1, infos=[None if tb is None else ghf.seek_parse(tb) for tb in tables],
                             d_tables=[None if k is None else src.view(k) for k in k_table], n_rows=n_rows, d_out=a.view(reg),
                             out_stride=out_stride, d_row_status=d_status)
    ctx.sync()
    assert ghf.lib().ghf_status(ctx.h) == OK
    clean = a.fetch()
    check_rows("decode_planes_gather, raw planes %s" % bin(raw), t, a, reg, d_status, n_rows, firsts, row_elems * e, out_stride, t.tensor, e)
    assert clean and src.fetch(), (t, "guard bytes")


def gather_forms(env, c):
    """ghf_decode_planes_gather_forms over a tensor of tests/forms_sweep.py: against the base at an odd address, and without"""
    ghf, ctx, torch = env
    d, e, row_elems, firsts = Dev(env, c), c.e, c.row_elems, c.firsts
    n_rows, out_stride = len(firsts), c.row_elems * c.e + 3
    a = Arena()
    regs = [a.add(n_rows * out_stride) for based in (0, 1)]
    a.alloc(torch)
    d_index = to_dev(torch, np.asarray(firsts, dtype=np.int64))
    d_status = [torch.full((n_rows + 1,), -1, dtype=torch.int32, device="cuda") for _ in regs]
    for based, reg in enumerate(regs):
        ctx.decode_planes_gather_forms(d.streams, d.sizes, d.d_codes, c.raw, c.sparse, d.ranks_dev, c.n, e, d_index, row_elems, index_stride=1,
                                       infos=d.infos, d_tables=d.d_tables, d_base=d.d_base_odd if based else None, n_rows=n_rows,
                                       d_out=a.view(reg), out_stride=out_stride, d_row_status=d_status[based])
    ctx.sync()
    assert ghf.lib().ghf_status(ctx.h) == OK
    clean = a.fetch()
    for based, reg in enumerate(regs):
        check_rows("decode_planes_gather_forms, " + ("base" if based else "plain"), c, a, reg, d_status[based], n_rows, firsts, row_elems * e,
                   out_stride, c.new if based else c.tensor, e)
    assert clean and d.inputs_intact(), (c, "guard bytes")


FAMILIES = {"whole": whole, "ranges": ranges, "gather_forms": gather_forms}


@pytest.fixture(scope="module", autouse=True)
def warm(env, sweep):
    """the first launch of a kernel loads its code object: every family runs once per width here, so that no id's time
    depends on the order in which the ids run.  Also: images beyond the library's own slot bound are among the cases"""
    ghf, ctx, torch = env
    for e in fs.WIDTHS:
        for run in FAMILIES.values():
            for c in fs.cases(e)[1:3]:  # without and (above bf16) with a raw plane
                run(env, c)
        gather_typed(env, fs.typed_rows(e)[2])
        assert any(s.image.size > ghf.planes_slot_bytes(s.n) for c in fs.cases(e) for s in c.streams()), e


@pytest.mark.parametrize("which", IDS, ids=id_of)
def test_whole_decode(env, which):
    """ghf_decode_planes_forms with side-cars written from code_sweep.expected_index: out of place without a base, and in place
    with d_base == d_out holding the base"""
    for c in cases_of(*which):
        whole(env, c)


@pytest.mark.parametrize("which", IDS, ids=id_of)
def test_range_decode(env, which):
    """ghf_decode_planes_forms_range over the case's four ranges, from seek tables (k_seek_expand_streams) and from side-cars,
    with and without the base elements of the range; without raw planes also ghf_decode_planes_sparse_range_delta from tables"""
    for c in cases_of(*which):
        ranges(env, c)


@pytest.mark.parametrize("which", IDS, ids=id_of)
def test_gather(env, which):
    """ghf_decode_planes_gather on the typed tensors of tests/code_sweep.py, one launch per tensor; every third with a raw plane"""
    e, lead = which
    mine = [case for case in fs.typed_rows(e) if case[0].variants[0] == lead]
    assert len(mine) >= cs.TYPED_CASES // 6
    for case in mine:
        gather_typed(env, case)


@pytest.mark.parametrize("which", IDS, ids=id_of)
def test_gather_forms(env, which):
    """ghf_decode_planes_gather_forms on the tensors of tests/forms_sweep.py, rank tables as device images"""
    for c in cases_of(*which):
        gather_forms(env, c)


# ------------------------------------------------------------------------------ e. the second grid line
def big_rows(n):
    index = (np.arange(BIG_ROWS, dtype=np.int64) * 7919) % (n - 4)
    index[BIG_BAD_ROW] = n  # passes the end
    return index


def check_big(got, status, index, src, e, what):
    n_rows, row_bytes = BIG_ROWS, BIG_ROW_ELEMS * e
    want_status = np.zeros(n_rows + 1, dtype=np.int32)
    want_status[BIG_BAD_ROW], want_status[n_rows] = E_INVAL, -1  # (the last entry is the guard behind the statuses)
    bad = np.flatnonzero(status != want_status)
    assert bad.size == 0, (what, "status of row %d: %d" % (int(bad[0]), int(status[bad[0]])), "%d rows differ" % bad.size)
    ok = index.copy()
    ok[BIG_BAD_ROW] = 0
    rows = src.reshape(-1, e)[ok[:, None] + np.arange(BIG_ROW_ELEMS)].reshape(n_rows, row_bytes)
    want = np.full((n_rows, BIG_STRIDE), GUARD, dtype=np.uint8)
    want[:, :row_bytes] = rows
    want[BIG_BAD_ROW] = GUARD
    got = got.reshape(n_rows, BIG_STRIDE)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "first wrong row %d (grid line %d)" % (int(bad[0]), int(bad[0]) >> 16), "%d rows differ" % bad.size)


def test_gather_beyond_65536_rows(env):
    """65 539 rows of five elements: rows 65 536.. are served by the second grid line of the launch, row 65 537 passes the end"""
    ghf, ctx, torch = env
    s = t_gather.Stored(ghf, torch, gp.tensor(2))
    index = big_rows(s.n)
    a = Arena()
    reg = a.add(BIG_ROWS * BIG_STRIDE)
    a.alloc(torch)
    d_status = torch.full((BIG_ROWS + 1,), -1, dtype=torch.int32, device="cuda")
    ctx.decode_planes_gather(d_index=to_dev(torch, index), row_elems=BIG_ROW_ELEMS, index_stride=1, n_rows=BIG_ROWS, d_out=a.view(reg),
                             out_stride=BIG_STRIDE, d_row_status=d_status, **s.args(0))
    ctx.sync()
    assert ghf.lib().ghf_status(ctx.h) == OK
    clean = a.fetch()
    check_big(a.got(reg), d_status.cpu().numpy(), index, s.t.bytes, 2, "decode_planes_gather")
    assert clean and s.arena.fetch(), "guard bytes"


def test_gather_forms_beyond_65536_rows(env):
    """the same rows of the sparse-and-dense bf16 tensor of tests/gather_forms_planes.py, against its base"""
    ghf, ctx, torch = env
    s = t_gforms.Stored(ghf, torch, fp.tensor(2))
    index = big_rows(s.n)
    a = Arena()
    reg = a.add(BIG_ROWS * BIG_STRIDE)
    a.alloc(torch)
    d_status = torch.full((BIG_ROWS + 1,), -1, dtype=torch.int32, device="cuda")
    ctx.decode_planes_gather_forms(d_index=to_dev(torch, index), row_elems=BIG_ROW_ELEMS, index_stride=1, n_rows=BIG_ROWS, d_out=a.view(reg),
                                   out_stride=BIG_STRIDE, d_row_status=d_status, **s.args(True))
    ctx.sync()
    assert ghf.lib().ghf_status(ctx.h) == OK
    clean = a.fetch()
    check_big(a.got(reg), d_status.cpu().numpy(), index, s.t.new, 2, "decode_planes_gather_forms")
    assert clean and s.arena.fetch(), "guard bytes"
