"""GPU: the plane batch calls with raw planes -- ghf_batch_planes_raw_auto, ghf_compress_batch_planes_forms,
ghf_decode_batch_planes_forms, ghf_decode_bodies_batch_planes_forms, ghf_decode_bodies_batch_planes_forms_seek (DESIGN.md
section 24).

The reference for a dense slot is ghf_compress_batch_planes_shared on the same batch (held against the CPU oracle by
tests/test_gpu_batch_planes.py); for a raw slot it is data[p::E] itself; for the rule it is tests/batch_forms_model.py.
Every case runs for E in {2, 4, 8}.  A batch has one item per element count in EDGE_ELEMS: the vector, segment and round
edges.  Inputs and decode outputs sit at odd addresses between 0xA5 guards, slots sit in guarded strides (the helpers'
approach of tests/test_gpu_batch_planes.py)."""
import ctypes as C

import numpy as np
import pytest

import batch_forms_model as model
import datagen as dg
import pkgload
from header_cases import bad_codes

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT, E_NOCODE = 0, 1, 3, 5, 6, 7, 10
GUARD = 0xA5
FILL = 0xCD  # what the side-car arrays hold before a compress call
COVER_ALL = 1
ES = [2, 4, 8]
EDGE_ELEMS = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8193]
FLOAT_MASK = {2: 0b01, 4: 0b0111, 8: 0b00111111}
KINDS = ["live", "bodies", "seek"]


def masks(e):
    """all four for E = 2; else 0, all planes, the float-typical mask, alternating bits, the top plane only"""
    if e == 2:
        return [0, 1, 2, 3]
    return [0, (1 << e) - 1, FLOAT_MASK[e], 0x55 & ((1 << e) - 1), 1 << (e - 1)]


CASES = [(e, m) for e in ES for m in masks(e)]


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def i64(torch, values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64).cuda()


def codes_to_device(torch, codes):
    t = torch.from_numpy(np.stack([np.frombuffer(bytes(c), dtype=np.uint8) for c in codes]).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


class Inputs:
    """items packed at odd addresses with three filler bytes between them; a None item is a null pointer of 96 bytes"""

    def __init__(self, torch, datas):
        self.datas, self.count = datas, len(datas)
        offs, at = [], 0
        for d in datas:
            at |= 1
            offs.append(at)
            at += (0 if d is None else d.size) + 3
        packed = np.full(at + 16, 0x5A, dtype=np.uint8)
        for o, d in zip(offs, datas):
            if d is not None:
                packed[o : o + d.size] = d
        self.d_in = torch.from_numpy(packed).cuda()
        self.sizes = [96 if d is None else int(d.size) for d in datas]
        self.in_ptrs = i64(torch, [0 if d is None else self.d_in.data_ptr() + o for o, d in zip(offs, datas)])
        self.in_bytes = i64(torch, self.sizes)


class Packed:
    """one compress call over `inp` under d_codes -- ghf_compress_batch_planes_shared (raw None) or .._forms (raw an int) --
    into guarded slots, the side-car arrays filled with FILL before it; everything the checks need is kept on the host"""

    def __init__(self, env, inp, d_codes, e, max_item, raw=None, caps=None):
        ghf, ctx, torch = env
        self.ghf, self.ctx, self.torch, self.inp, self.d_codes, self.e, self.max_item, self.raw = ghf, ctx, torch, inp, d_codes, e, max_item, raw
        self.count, self.slots, self.datas = inp.count, inp.count * e, inp.datas
        bound = ghf.compress_batch_planes_shared_bound(max_item, e)
        self.caps = [bound] * self.slots if caps is None else list(caps)
        self.stride = (max(self.caps) + 15 & ~15) + 64
        self.d_out = torch.full((self.slots * self.stride + 16,), GUARD, dtype=torch.uint8).cuda()
        self.out_ptrs = i64(torch, [self.d_out.data_ptr() + j * self.stride for j in range(self.slots)])
        self.out_caps = i64(torch, self.caps)
        self.out_bytes = torch.full((self.slots,), -1, dtype=torch.int64).cuda()
        self.status = torch.full((self.slots,), -1, dtype=torch.int32).cuda()
        self.bidx = ctx.batch_index_alloc(self.slots, max_item // e)
        L = ghf.lib()
        self.chunk_bytes, self.seg_bytes = 8 * self.slots * self.bidx.blocks_per_item, 4 * self.slots * self.bidx.segs_per_item
        assert L.ghf_memset_d(ctx.h, self.bidx.d_chunk_bit, FILL, self.chunk_bytes) == 0
        assert L.ghf_memset_d(ctx.h, self.bidx.d_seg_bit, FILL, self.seg_bytes) == 0

    def run(self):
        L = self.ghf.lib()
        head = (self.ctx.h, self.inp.in_ptrs.data_ptr(), self.inp.in_bytes.data_ptr(), self.max_item, self.count, self.e, self.d_codes.data_ptr())
        tail = (self.out_ptrs.data_ptr(), self.out_caps.data_ptr(), self.out_bytes.data_ptr(), C.byref(self.bidx), self.status.data_ptr())
        rc = L.ghf_compress_batch_planes_shared(*head, *tail) if self.raw is None else L.ghf_compress_batch_planes_forms(*head, self.raw, *tail)
        assert rc == 0, rc
        self.ctx.sync()  # raises if the context's status word was latched: per-slot failures must not do that
        self.h_out = self.d_out.cpu().numpy()
        self.h_bytes = self.out_bytes.cpu().numpy()
        self.h_status = self.status.cpu().numpy()
        chunk, seg = np.zeros(self.chunk_bytes // 8, dtype=np.uint64), np.zeros(self.seg_bytes // 4, dtype=np.uint32)
        assert L.ghf_copy_d2h(self.ctx.h, chunk.ctypes.data, self.bidx.d_chunk_bit, chunk.nbytes) == 0
        assert L.ghf_copy_d2h(self.ctx.h, seg.ctypes.data, self.bidx.d_seg_bit, seg.nbytes) == 0
        self.ctx.sync()
        self.h_chunk, self.h_seg = chunk.reshape(self.slots, -1), seg.reshape(self.slots, -1)
        return self

    def slot(self, j):
        return self.h_out[j * self.stride : (j + 1) * self.stride]

    def free(self):
        if self.bidx is not None:
            self.ctx.batch_index_free(self.bidx)
            self.bidx = None


class World:
    """the edge batch of one width: its codes from the library, the parent's compress and one forms compress per mask"""

    def __init__(self, env, e):
        ghf, ctx, torch = env
        self.env, self.e, self.max_item = env, e, 8193 * e
        self.datas = [dg.make(["uniform", "zipf", "sym16", "text"][k % 4], n * e, seed=2400 + 16 * e + k) for k, n in enumerate(EDGE_ELEMS)]
        self.inp = Inputs(torch, self.datas)
        d_hists = torch.empty((e, 257), dtype=torch.int64).cuda()
        rc = ghf.lib().ghf_histogram_batch_planes(ctx.h, self.inp.in_ptrs.data_ptr(), self.inp.in_bytes.data_ptr(), self.max_item,
                                                  self.inp.count, e, COVER_ALL, d_hists.data_ptr())
        assert rc == 0
        self.d_codes = ctx.build_codes(d_hists)
        ctx.sync()
        self.h_codes = [ghf.Code.from_buffer_copy(row.tobytes()) for row in self.d_codes.cpu().numpy()]
        self.parent = Packed(env, self.inp, self.d_codes, e, self.max_item).run()
        assert np.all(self.parent.h_status == OK)
        self.forms = {}
        self.recs = {}

    def packed(self, raw):
        if raw not in self.forms:
            self.forms[raw] = Packed(self.env, self.inp, self.d_codes, self.e, self.max_item, raw=raw).run()
        return self.forms[raw]

    def records(self, raw):
        """ghf_batch_seek_pack on the index of the forms compress (raw None: of the parent's)"""
        if raw not in self.recs:
            ghf, ctx, torch = self.env
            b = self.parent if raw is None else self.packed(raw)
            self.recs[raw] = ctx.batch_seek_pack(b.bidx, self.inp.in_bytes, elem_bytes=self.e)
            ctx.sync()
        return self.recs[raw]

    def free(self):
        self.parent.free()
        for b in self.forms.values():
            b.free()


_worlds = {}


def world(env, e):
    if e not in _worlds:
        _worlds[e] = World(env, e)
    return _worlds[e]


@pytest.fixture(scope="module", autouse=True)
def _free_worlds():
    yield
    for w in _worlds.values():
        w.free()
    _worlds.clear()


def decode(kind, w, b, raw, stream_ptrs=None, stream_bytes=None, d_codes=None, caps=None, sizes_only=False, null_recs=True):
    """one forms decode of the slots of `b`: "live" (ghf_decode_batch_planes_forms), "bodies" (.._bodies_.._forms) or "seek"
    (.._forms_seek, with the records ghf_batch_seek_pack makes of b's index; a raw slot gets a null record of 0 bytes).
    Every output sits at an unaligned address between guard bytes.  -> (status, out_bytes, outs, (front, back) guards)"""
    ghf, ctx, torch = w.env
    e, L = w.e, ghf.lib()
    want = list(w.inp.sizes)
    ostride = (w.max_item + 15 & ~15) + 64
    d_out = torch.full((b.count * ostride + 64,), GUARD, dtype=torch.uint8).cuda()
    ooff = [i * ostride + 17 + (i % 15) for i in range(b.count)]  # misalignments 1..15 (+ 17)
    out_ptrs = i64(torch, [d_out.data_ptr() + o for o in ooff])
    out_caps = i64(torch, [w.max_item] * b.count if caps is None else caps)
    out_bytes = torch.full((b.count,), -1, dtype=torch.int64).cuda()
    status = torch.full((b.count,), -1, dtype=torch.int32).cuda()
    sp = b.out_ptrs if stream_ptrs is None else i64(torch, stream_ptrs)
    sb = b.out_bytes if stream_bytes is None else i64(torch, stream_bytes)
    cd = b.d_codes if d_codes is None else d_codes
    tail = (None if sizes_only else out_ptrs.data_ptr(), out_caps.data_ptr(), out_bytes.data_ptr(), status.data_ptr())
    if kind == "live":
        assert not sizes_only
        n_elems = i64(torch, [s // e for s in want])
        rc = L.ghf_decode_batch_planes_forms(ctx.h, sp.data_ptr(), sb.data_ptr(), cd.data_ptr(), C.byref(b.bidx), n_elems.data_ptr(), b.count,
                                             e, raw, *tail)
    elif kind == "bodies":
        rc = L.ghf_decode_bodies_batch_planes_forms(ctx.h, sp.data_ptr(), sb.data_ptr(), cd.data_ptr(), b.count, e, raw, *tail)
    else:
        r = w.records(b.raw)
        rp, rb = r["rec_ptrs"].clone(), r["rec_bytes"].clone()
        if null_recs:
            for p in range(e):
                if raw >> p & 1:
                    rp[p::e] = 0
                    rb[p::e] = 0
        rc = L.ghf_decode_bodies_batch_planes_forms_seek(ctx.h, sp.data_ptr(), sb.data_ptr(), rp.data_ptr(), rb.data_ptr(), cd.data_ptr(),
                                                         b.count, e, raw, *tail)
    assert rc == 0, rc
    ctx.sync()
    h = d_out.cpu().numpy()
    outs, guards = [], []
    for i in range(b.count):
        n = 0 if sizes_only else int(want[i])
        outs.append(h[ooff[i] : ooff[i] + n])
        guards.append((h[i * ostride : ooff[i]], h[ooff[i] + n : (i + 1) * ostride]))
    return status.cpu().numpy(), out_bytes.cpu().numpy(), outs, guards


def garbage_codes(w, planes, seed):
    """the world's codes with the codes of `planes` overwritten by random bytes"""
    torch = w.env[2]
    h = w.d_codes.cpu().numpy().copy()
    rng = np.random.default_rng(seed)
    for p in planes:
        h[p] = rng.integers(0, 256, size=h[p].size, dtype=np.uint8)
    return torch.from_numpy(h).cuda()


def bad_code_on(w, p):
    """the world's codes with plane p's replaced by one whose Kraft sum is above 1"""
    torch = w.env[2]
    ghf = w.env[0]
    bad = bad_codes(w.h_codes[p], ghf.Code.from_buffer_copy)[1][1]
    return codes_to_device(torch, [bad if q == p else c for q, c in enumerate(w.h_codes)])


# ------------------------------------------------------------------------------ 1. compress
@pytest.mark.parametrize("e,raw", CASES)
def test_compress_dense_slots_equal_the_parent_and_raw_slots_hold_the_plane(env, e, raw):
    w = world(env, e)
    assert [d.size // e for d in w.datas] == EDGE_ELEMS
    a, b = w.parent, w.packed(raw)
    assert np.all(b.h_status == OK), b.h_status.tolist()
    for j in range(b.slots):
        i, p = divmod(j, e)
        if raw >> p & 1:
            n = w.datas[i].size // e
            assert int(b.h_bytes[j]) == n, j
            assert np.array_equal(b.slot(j)[:n], w.datas[i][p::e]), j
            assert np.all(b.slot(j)[n:] == GUARD), j  # nothing at or beyond n
            assert np.all(b.h_chunk[j] == np.uint64(int.from_bytes(bytes([FILL] * 8), "little"))), j  # the slice is not written
            assert np.all(b.h_seg[j] == np.uint32(int.from_bytes(bytes([FILL] * 4), "little"))), j
        else:
            assert int(b.h_bytes[j]) == int(a.h_bytes[j]), j
            assert np.array_equal(b.slot(j), a.slot(j)), j  # the body, and the guards behind it
            assert np.array_equal(b.h_chunk[j], a.h_chunk[j]) and np.array_equal(b.h_seg[j], a.h_seg[j]), j
    if raw == 0:  # the parent in every array
        assert np.array_equal(b.h_out, a.h_out) and np.array_equal(b.h_bytes, a.h_bytes) and np.array_equal(b.h_status, a.h_status)
        assert np.array_equal(b.h_chunk, a.h_chunk) and np.array_equal(b.h_seg, a.h_seg)


@pytest.mark.parametrize("e", ES)
def test_compress_failures_on_raw_slots(env, e):
    ghf, ctx, torch = env
    w = world(env, e)
    raw = FLOAT_MASK[e]
    max_item = w.max_item
    good = w.datas[7]  # 4095 elements
    datas = [good, np.zeros(0, dtype=np.uint8), None, dg.make("uniform", 7 * e + 1, seed=1), dg.make("zipf", 8194 * e, seed=2), w.datas[8],
             w.datas[3]]
    inp = Inputs(torch, datas)
    bound = ghf.compress_batch_planes_shared_bound(max_item, e)
    caps = [bound] * (len(datas) * e)
    caps[5 * e + 0] = 4096 - 1  # plane 0 is raw under every FLOAT_MASK: one byte short
    a = Packed(env, inp, w.d_codes, e, max_item, caps=[bound] * len(caps)).run()
    b = Packed(env, inp, w.d_codes, e, max_item, raw=raw, caps=caps).run()
    g = Packed(env, inp, garbage_codes(w, [p for p in range(e) if raw >> p & 1], 5), e, max_item, raw=raw, caps=caps).run()
    try:
        per_item = [OK, E_EMPTY, E_INVAL, E_INVAL, E_INVAL, OK, OK]
        want = [s for s in per_item for _ in range(e)]
        assert a.h_status.tolist() == want  # the parent's verdicts
        want[5 * e + 0] = E_CAP
        assert b.h_status.tolist() == want
        for j in range(b.slots):
            i, p = divmod(j, e)
            if want[j] != OK:
                assert int(b.h_bytes[j]) == 0 and np.all(b.slot(j) == GUARD), j  # a refused slot writes nothing at all
            elif raw >> p & 1:
                n = datas[i].size // e
                assert int(b.h_bytes[j]) == n and np.array_equal(b.slot(j)[:n], datas[i][p::e]) and np.all(b.slot(j)[n:] == GUARD), j
            else:
                assert int(b.h_bytes[j]) == int(a.h_bytes[j]) and np.array_equal(b.slot(j), a.slot(j)), j
        # garbage in d_codes[p] of the raw planes changes nothing
        assert np.array_equal(g.h_out, b.h_out) and np.array_equal(g.h_bytes, b.h_bytes) and np.array_equal(g.h_status, b.h_status)
        assert np.array_equal(g.h_chunk, b.h_chunk) and np.array_equal(g.h_seg, b.h_seg)
    finally:
        a.free()
        b.free()
        g.free()
    # a bad code on a dense plane: GHF_E_FORMAT on that plane's slots only
    dense = e - 1
    assert not raw >> dense & 1
    f = Packed(env, w.inp, bad_code_on(w, dense), e, max_item, raw=raw).run()
    try:
        assert f.h_status.tolist() == [E_FORMAT if j % e == dense else OK for j in range(f.slots)]
        ref = w.packed(raw)
        for j in range(f.slots):
            if j % e == dense:
                assert int(f.h_bytes[j]) == 0 and np.all(f.slot(j) == GUARD), j
            else:
                assert int(f.h_bytes[j]) == int(ref.h_bytes[j]) and np.array_equal(f.slot(j), ref.slot(j)), j
    finally:
        f.free()


# ------------------------------------------------------------------------------ 2. the three decoders
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("e,raw", CASES)
def test_round_trips(env, e, raw, kind):
    w = world(env, e)
    b = w.packed(raw)
    status, out_bytes, outs, guards = decode(kind, w, b, raw)
    assert np.all(status == OK), status.tolist()
    for i, d in enumerate(w.datas):
        assert int(out_bytes[i]) == d.size, i
        assert np.array_equal(outs[i], d), i
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    if kind != "live":  # the sizes-only mode: an item whose planes are all raw takes its size from the slots' sizes alone
        status, out_bytes, _, guards = decode(kind, w, b, raw, sizes_only=True)
        assert np.all(status == OK) and out_bytes.tolist() == [d.size for d in w.datas]
        assert all(np.all(g[0] == GUARD) and np.all(g[1] == GUARD) for g in guards)


@pytest.mark.parametrize("e,raw", CASES)
def test_seek_pack_on_the_forms_index_gives_the_parents_records_for_the_dense_slots(env, e, raw):
    w = world(env, e)
    ra, rb = w.records(None), w.records(raw)
    ha, hb = ra["rec"].cpu().numpy(), rb["rec"].cpu().numpy()
    sa, sb, na, nb = ra["status"].cpu().numpy(), rb["status"].cpu().numpy(), ra["rec_bytes"].cpu().numpy(), rb["rec_bytes"].cpu().numpy()
    assert np.all(sa == OK)
    stride = ra["rec_stride"]
    assert stride == rb["rec_stride"]
    for j in range(w.parent.slots):
        if not raw >> (j % e) & 1:  # (what the call reports for a raw slot is not specified)
            assert int(sb[j]) == OK and int(nb[j]) == int(na[j]), j
            assert np.array_equal(hb[j * stride : j * stride + int(nb[j])], ha[j * stride : j * stride + int(na[j])]), j


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("e", ES)
def test_decode_failures_on_raw_slots(env, e, kind):
    w = world(env, e)
    raw = FLOAT_MASK[e]
    b = w.packed(raw)
    n_of = [d.size // e for d in w.datas]
    ptrs = [int(x) for x in b.out_ptrs.cpu().tolist()]
    sizes = [int(x) for x in b.h_bytes]
    caps = [w.max_item] * b.count
    want = [OK] * b.count
    top_raw = max(p for p in range(e) if raw >> p & 1)
    ptrs[2 * e + 0] = 0  # a null pointer on a raw slot
    want[2] = E_INVAL
    ptrs[3 * e + top_raw] += 8  # a misaligned one
    want[3] = E_INVAL
    sizes[5 * e + 0] = 0  # a size of 0: no count in the bodies-only decoders, not n_elems in the live one
    want[5] = E_CORRUPT if kind == "live" else E_INVAL
    sizes[6 * e + top_raw] = n_of[6] + 1  # one more than the other planes
    want[6] = E_CORRUPT
    sizes[8 * e + 0] = n_of[8] - 1  # one fewer
    want[8] = E_CORRUPT
    caps[9] = n_of[9] * e - 1
    want[9] = E_CAP
    status, out_bytes, outs, guards = decode(kind, w, b, raw, stream_ptrs=ptrs, stream_bytes=sizes, caps=caps)
    assert status.tolist() == want
    for i, d in enumerate(w.datas):
        assert np.all(guards[i][0] == GUARD), i
        if want[i] == OK:
            assert int(out_bytes[i]) == d.size and np.array_equal(outs[i], d) and np.all(guards[i][1] == GUARD), i
            continue
        assert int(out_bytes[i]) == 0, i
        if want[i] == E_CORRUPT and kind == "bodies":
            # with nothing but the bytes a count that disagrees with a DENSE plane shows only once that plane is decoded: the
            # planes in front of it are written, below the cap (here the whole item stride) as the parent does
            back = np.concatenate((outs[i], guards[i][1]))
            assert np.all(back[caps[i] :] == GUARD), i
        else:  # seen before the item's first store: output and guards untouched
            assert np.all(outs[i] == GUARD) and np.all(guards[i][1] == GUARD), i
    # a bad code on a dense plane: GHF_E_FORMAT on every item, nothing written
    status, out_bytes, outs, guards = decode(kind, w, b, raw, d_codes=bad_code_on(w, e - 1))
    assert status.tolist() == [E_FORMAT] * b.count and np.all(out_bytes == 0)
    for i in range(b.count):
        assert np.all(outs[i] == GUARD) and np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    # garbage in the codes of the raw planes is ignored
    status, out_bytes, outs, guards = decode(kind, w, b, raw, d_codes=garbage_codes(w, [p for p in range(e) if raw >> p & 1], 9))
    assert np.all(status == OK)
    for i, d in enumerate(w.datas):
        assert int(out_bytes[i]) == d.size and np.array_equal(outs[i], d), i


@pytest.mark.parametrize("e", ES)
def test_seek_decoder_reads_no_record_of_a_raw_slot_and_holds_counts_against_the_dense_records(env, e):
    """the run-record decoder with the records of ANOTHER item on the dense planes: the raw counts disagree with them"""
    w = world(env, e)
    raw = FLOAT_MASK[e]
    b = w.packed(raw)
    ptrs = [int(x) for x in b.out_ptrs.cpu().tolist()]
    sizes = [int(x) for x in b.h_bytes]
    for p in range(e):  # item 4's raw planes claim the counts (and bytes) of item 3's
        if raw >> p & 1:
            ptrs[4 * e + p], sizes[4 * e + p] = ptrs[3 * e + p], sizes[3 * e + p]
    want = [OK] * b.count
    want[4] = E_CORRUPT
    for so in (True, False):
        status, out_bytes, outs, guards = decode("seek", w, b, raw, stream_ptrs=ptrs, stream_bytes=sizes, sizes_only=so)
        assert status.tolist() == want and int(out_bytes[4]) == 0
        assert so or np.all(outs[4] == GUARD)  # all counts of an item are vetted before its first store
        assert all(np.all(g[0] == GUARD) and np.all(g[1] == GUARD) for g in guards)


# ------------------------------------------------------------------------------ 3. the rule on the device
def _device_mask(env, datas, e, cover):
    ghf, ctx, torch = env
    tensors = [torch.from_numpy(d).cuda() for d in datas]
    d_hists = ctx.histogram_batch_planes(tensors, e, flags=COVER_ALL if cover else 0)
    d_codes = ctx.build_codes(d_hists)
    mask = ctx.batch_planes_raw_auto(d_hists, d_codes)
    ctx.sync()
    return int(mask.item()), tensors, d_hists, d_codes


@pytest.mark.parametrize("e", ES)
def test_raw_auto_equals_the_model_on_the_pinned_inputs(env, e):
    ghf, ctx, torch = env
    datas = model.normal_batch(e)
    got, _, d_hists, d_codes = _device_mask(env, datas, e, True)
    hists = model.plane_hists(datas, e, cover=True)
    assert np.array_equal(d_hists.cpu().numpy(), hists)
    assert got == model.raw_mask(hists, model.build_codes(hists)) == model.PINNED_NORMAL[e][0]
    # a code out of the length bounds leaves its plane dense; a plane without counts is not raw
    h = d_codes.cpu().numpy().copy()
    code = ghf.Code.from_buffer_copy(h[0].tobytes())
    code.max_len = 33
    h[0] = np.frombuffer(bytes(code), dtype=np.uint8)
    mask = ctx.batch_planes_raw_auto(d_hists, torch.from_numpy(h).cuda())
    zero = d_hists.clone()
    zero[0, :256] = 0
    mask1 = ctx.batch_planes_raw_auto(zero, d_codes)
    ctx.sync()
    assert int(mask.item()) == got & ~1 and int(mask1.item()) == got & ~1
    rng = np.random.default_rng(7)
    tiny = [model.normal_elems(rng, 17, e) for _ in range(3)]
    assert _device_mask(env, tiny, e, False)[0] == 0
    assert _device_mask(env, tiny, e, True)[0] == model.PINNED_TINY_COVER[e]


# ------------------------------------------------------------------------------ 4. the size claim, through the python helpers
@pytest.mark.parametrize("e", ES)
def test_stored_bytes_of_the_normal_batch_and_the_python_helpers(env, e):
    """64 items of 2048 standard-normal values under the mask the device picks: the stored bytes are the model's (bf16:
    175 120 against 175 235 all dense), and the Context helpers round-trip through all three decoders"""
    ghf, ctx, torch = env
    datas = model.normal_batch(e)
    mask, tensors, d_hists, d_codes = _device_mask(env, datas, e, True)
    want_mask, want_forms, want_dense = model.PINNED_NORMAL[e]
    assert mask == want_mask
    bidx = ctx.batch_index_alloc(len(datas) * e, 2048)
    try:
        dense = ctx.compress_batch_planes_shared(tensors, d_codes, e)
        r = ctx.compress_batch_planes_forms(tensors, d_codes, e, mask, index=bidx)
        ctx.sync()
        assert not dense["status"].any().item() and not r["status"].any().item()
        stored = (int(dense["out_bytes"].sum().item()), int(r["out_bytes"].sum().item()))
        print("E %d: %d bytes all dense, %d with raw planes %s" % (e, stored[0], stored[1], bin(mask)))
        assert stored == (want_dense, want_forms)
        recs = ctx.batch_seek_pack(bidx, r["in_bytes"], elem_bytes=e)
        live = ctx.decode_batch_planes_forms(r["out_ptrs"], r["out_bytes"], d_codes, bidx, r["n_elems"], e, mask)
        sizes = ctx.decode_bodies_batch_planes_forms(r["out_ptrs"], r["out_bytes"], d_codes, e, mask)
        bod = ctx.decode_bodies_batch_planes_forms(r["out_ptrs"], r["out_bytes"], d_codes, e, mask, out=True, caps=sizes["out_bytes"])
        seek = ctx.decode_bodies_batch_planes_forms_seek(r["out_ptrs"], r["out_bytes"], recs["rec_ptrs"], recs["rec_bytes"], d_codes, e, mask,
                                                         out=True, caps=sizes["out_bytes"])
        ctx.sync()
        assert sizes["out_bytes"].cpu().tolist() == [d.size for d in datas]
        for name, dec in (("live", live), ("bodies", bod), ("seek", seek)):
            assert dec["status"].cpu().tolist() == [OK] * len(datas), name
            h = dec["out"].cpu().numpy()
            for i, d in enumerate(datas):
                assert np.array_equal(h[i * dec["out_stride"] :][: d.size], d), (name, i)
    finally:
        ctx.batch_index_free(bidx)


# ------------------------------------------------------------------------------ 5. call-level errors
def test_call_level_argument_errors(env):
    ghf, ctx, torch = env
    L = ghf.lib()
    w = world(env, 4)
    b = Packed(env, w.inp, w.d_codes, 4, w.max_item, raw=0)
    r = w.records(None)
    codes = w.d_codes.data_ptr()
    word = torch.full((1,), 77, dtype=torch.int32).cuda()
    d_hists = torch.ones((4, 257), dtype=torch.int64).cuda()
    try:
        P = lambda t: None if t is None else t.data_ptr()
        comp = lambda raw=0, e=4, count=b.count, cd=codes, st=b.status: L.ghf_compress_batch_planes_forms(
            ctx.h, P(w.inp.in_ptrs), P(w.inp.in_bytes), w.max_item, count, e, cd, raw, P(b.out_ptrs), P(b.out_caps), P(b.out_bytes),
            C.byref(b.bidx), P(st))
        live = lambda raw=0, e=4, count=b.count, cd=codes, st=b.status: L.ghf_decode_batch_planes_forms(
            ctx.h, P(b.out_ptrs), P(b.out_bytes), cd, C.byref(b.bidx), P(w.inp.in_bytes), count, e, raw, P(b.out_ptrs), P(b.out_caps),
            P(b.out_bytes), P(st))
        bod = lambda raw=0, e=4, count=b.count, cd=codes, st=b.status: L.ghf_decode_bodies_batch_planes_forms(
            ctx.h, P(b.out_ptrs), P(b.out_bytes), cd, count, e, raw, P(b.out_ptrs), P(b.out_caps), P(b.out_bytes), P(st))
        seek = lambda raw=0, e=4, count=b.count, cd=codes, st=b.status, rp=r["rec_ptrs"]: L.ghf_decode_bodies_batch_planes_forms_seek(
            ctx.h, P(b.out_ptrs), P(b.out_bytes), P(rp), P(r["rec_bytes"]), cd, count, e, raw, P(b.out_ptrs), P(b.out_caps), P(b.out_bytes),
            P(st))
        auto = lambda e=4, h=d_hists, cd=codes, out=word: L.ghf_batch_planes_raw_auto(ctx.h, P(h), cd, e, P(out))
        for f in (comp, live, bod, seek):
            assert f(count=0) == OK and f(count=0, raw=0b1111) == OK  # queues nothing
            for raw in (0b10000, 0x80000000, 0xFFFFFFFF):  # a bit at or above elem_bytes
                assert f(raw=raw) == E_INVAL and f(raw=raw, count=0) == E_INVAL, raw
            assert f(e=2, raw=0b0100) == E_INVAL
            for e in (0, 1, 3, 16):
                assert f(e=e) == E_INVAL, e
            assert f(cd=None) == E_INVAL and f(cd=codes + 8) == E_INVAL and f(st=None) == E_INVAL
        assert seek(rp=None) == E_INVAL  # the record arrays themselves are required, whatever the mask
        assert seek(rp=None, raw=0b1111) == E_INVAL
        for e in (0, 1, 3, 16):
            assert auto(e=e) == E_INVAL
        assert auto(h=None) == E_INVAL and auto(cd=None) == E_INVAL and auto(cd=codes + 8) == E_INVAL and auto(out=None) == E_INVAL
        ctx.sync()
        assert np.all(b.status.cpu().numpy() == -1) and np.all(b.d_out.cpu().numpy() == GUARD) and int(word.item()) == 77
        assert comp(raw=0b0101) == OK  # and the context is still usable
        ctx.sync()
        assert b.status.cpu().tolist() == [OK] * b.slots
    finally:
        b.free()
