"""GPU: stored shared-code bodies -- ghf_batch_seek_pack, ghf_decode_bodies_batch_shared_seek and
ghf_decode_bodies_batch_planes_shared_seek.

Expected values never come from the code under test: bodies are written by orc_encode_body under an orc_build_code code
(oracle.lib(); pinned to the reference by tests/test_oracle_golden.py), and the expected RECORD of a body is computed from
the oracle's code lengths: np.add.reduceat(code.length[data], range(0, n, 128)) behind the 8 header bytes.  The library's
packer and its other decoders appear only where a test says so (the pack call needs a live side-car; the cross-check).
Streams and records are 16-byte aligned; outputs sit at odd addresses between guard bytes that are checked after every
call.  In the style of tests/test_gpu_batch_bodies.py."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import datagen as dg
import pkgload
from cases import CASES
from header_cases import bad_codes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT = 0, 1, 3, 5, 6, 7
GUARD = 0xA5
MAX_ITEM = 1 << 20
MAGIC = 0x31524247
RUN = 128
# the run's edges (127 .. 129), the side-car block's (4095 .. 4097), the round's (32767 .. 32769: 256 runs), three rounds
SIZES = [1, 127, 128, 129, 4095, 4096, 4097, 32767, 32768, 32769, 65536 + 77]
ES = [2, 4, 8]
PLANE_ELEMS = [1, 127, 128, 129, 2048, 40000]


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def i64(torch, values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64).cuda()


# ---- the oracle's side ------------------------------------------------------------------------------------------------
def cover_all_code(datas):
    """orc_build_code on the items' summed orc_histogram, every count of 0 raised to 1 (GHF_HIST_COVER_ALL)"""
    h = np.zeros(257, dtype=np.int64)
    for d in datas:
        h[:256] += orc.histogram(d)[:256]
    h[:256] = np.where(h[:256] == 0, 1, h[:256])
    h[256] = 1
    return orc.build_code(h)


def orc_body(data, code):
    a = np.ascontiguousarray(data, dtype=np.uint8)
    cap = 4 * a.size + 16
    out = np.zeros(cap, dtype=np.uint8)
    n = orc.lib().orc_encode_body(a.ctypes.data, a.size, C.byref(code), out.ctypes.data, cap)
    assert n != C.c_size_t(-1).value
    return out[:n].copy()


def record_of(run_bits, n, magic=MAGIC):
    """the bytes of a record: u32 magic, u32 n, u16 run_bits[], zeros up to a multiple of 8"""
    raw = struct.pack("<II", magic, n) + np.asarray(run_bits, dtype="<u2").tobytes()
    return np.frombuffer(raw + bytes(-len(raw) % 8), dtype=np.uint8).copy()


def run_bits_of(data, code):
    lens = np.asarray(list(code.length), dtype=np.int64)[np.ascontiguousarray(data, dtype=np.uint8)]
    return np.add.reduceat(lens, range(0, data.size, RUN))


def orc_record(data, code):
    bits = run_bits_of(data, code)
    assert bits.size == -(-data.size // RUN) and bits.max() <= 0xFFFF
    rec = record_of(bits, data.size)
    assert rec.size == (8 + 2 * bits.size + 7) // 8 * 8
    return rec


def codes_to_device(torch, codes):
    """ctypes code structs (ghf.Code, orc.OrcCode: the same layout) -> a CUDA uint8 tensor [len(codes), sizeof(Code)]"""
    t = torch.from_numpy(np.stack([np.frombuffer(bytes(c), dtype=np.uint8) for c in codes]).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def normal_elems(rng, n, e):
    """n standard-normal values as bf16 (the high half of the fp32), fp32 or fp64 -> uint8[n * e]"""
    x = rng.standard_normal(n)
    if e == 2:
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()
    return x.astype(np.float32 if e == 4 else np.float64).view(np.uint8).copy()


# ---- the calls --------------------------------------------------------------------------------------------------------
class Packed:
    """host uint8 arrays packed into one device buffer, each at a 16-byte aligned address (+ shift[k]), GUARD between them
    and at least 64 bytes of it behind each; a None entry is a null pointer; sizes[k] overrides the size that is passed"""

    def __init__(self, torch, arrays, sizes=None, shift=None):
        self.count = len(arrays)
        self.offs, at = [], 0
        for k, b in enumerate(arrays):
            self.offs.append(at + (shift[k] if shift else 0))
            at += ((0 if b is None else b.size) + 15 & ~15) + 64
        packed = np.full(at + 64, GUARD, dtype=np.uint8)
        for o, b in zip(self.offs, arrays):
            if b is not None:
                packed[o : o + b.size] = b
        self.d = torch.from_numpy(packed).cuda()
        assert self.d.data_ptr() % 16 == 0
        self.ptrs = i64(torch, [0 if b is None else self.d.data_ptr() + o for o, b in zip(self.offs, arrays)])
        self.sizes = [(0 if b is None else int(b.size)) if sizes is None or sizes[k] is None else int(sizes[k]) for k, b in enumerate(arrays)]
        self.bytes = i64(torch, self.sizes)


def run(env, bo, ro, d_codes, caps=None, null_out=(), e=1):
    """one ghf_decode_bodies_batch_shared_seek (e == 1) or .._planes_shared_seek call over the bodies `bo` and records `ro`;
    caps=None: sizes only, with a poisoned buffer named as d_out_caps that must stay as it is.  Every output sits at an
    address misaligned by 1..15 between GUARD bytes.  -> (status, out_bytes, outputs cut to their caps, guards)"""
    ghf, ctx, torch = env
    assert bo.count == ro.count and bo.count % e == 0
    n = bo.count // e
    out_bytes = torch.full((n,), -1, dtype=torch.int64).cuda()
    status = torch.full((n,), -1, dtype=torch.int32).cuda()
    L = ghf.lib()

    def call(out_ptrs, out_caps):
        head = (ctx.h, bo.ptrs.data_ptr(), bo.bytes.data_ptr(), ro.ptrs.data_ptr(), ro.bytes.data_ptr(), d_codes.data_ptr(), n)
        tail = (out_ptrs, out_caps, out_bytes.data_ptr(), status.data_ptr())
        rc = L.ghf_decode_bodies_batch_shared_seek(*head, *tail) if e == 1 else L.ghf_decode_bodies_batch_planes_shared_seek(*head, e, *tail)
        assert rc == 0, rc
        ctx.sync()  # raises if the context's status word was latched: per-item failures must not do that

    if caps is None:
        poison = torch.full((4096,), GUARD, dtype=torch.uint8).cuda()
        call(None, poison.data_ptr())
        assert bool((poison == GUARD).all())
        return status.cpu().numpy(), out_bytes.cpu().numpy(), None, None
    slots, at = [], 0
    for i, c in enumerate(caps):
        lo = at
        at += 17 + (i % 15)  # misalignments 1..15 (+ 17) behind a 16-byte boundary
        slots.append((lo, at, at + int(c)))
        at = (at + int(c) + 15 & ~15) + 48
    d_out = torch.full((at + 64,), GUARD, dtype=torch.uint8).cuda()
    assert d_out.data_ptr() % 16 == 0
    out_ptrs = i64(torch, [0 if i in null_out else d_out.data_ptr() + s[1] for i, s in enumerate(slots)])
    out_caps = i64(torch, caps)
    call(out_ptrs.data_ptr(), out_caps.data_ptr())
    h = d_out.cpu().numpy()
    ends = [s[0] for s in slots[1:]] + [h.size]
    outs = [h[s[1] : s[2]] for s in slots]
    guards = [(h[s[0] : s[1]], h[s[2] : e_]) for s, e_ in zip(slots, ends)]
    return status.cpu().numpy(), out_bytes.cpu().numpy(), outs, guards


def check_round_trip(env, bodies, records, datas, d_codes, e=1, stream_bytes=None):
    """sizes-only call -> the input sizes; decode call into exactly those caps -> the inputs (by SHA), guards intact"""
    torch = env[2]
    bo, ro = Packed(torch, bodies, sizes=stream_bytes), Packed(torch, records)
    want = [d.size for d in datas]
    status, nbytes, _, _ = run(env, bo, ro, d_codes, e=e)
    print("sizes:  status", status.tolist(), "bytes", nbytes.tolist())
    assert status.tolist() == [OK] * len(datas) and nbytes.tolist() == want
    status, nbytes, outs, guards = run(env, bo, ro, d_codes, caps=want, e=e)
    print("decode: status", status.tolist(), "bytes", nbytes.tolist())
    assert status.tolist() == [OK] * len(datas) and nbytes.tolist() == want
    for i, d in enumerate(datas):
        assert outs[i].size == d.size and sha(outs[i]) == sha(d), (i, d.size)
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i


def pack(env, bidx, in_bytes, e=1, caps=None, null=(), shift=None):
    """one ghf_batch_seek_pack call; slot j's record goes to a 16-byte aligned address (+ shift[j]) between GUARD bytes.
    caps=None: ghf_batch_seek_bound of the slice.  -> (status, rec_bytes, the slots' bytes up to the next slot)"""
    ghf, ctx, torch = env
    count = int(in_bytes.numel())
    slots = count * e
    stride = ghf.batch_seek_bound(int(bidx.max_item_bytes)) + 32
    d_rec = torch.full((slots * stride + 64,), GUARD, dtype=torch.uint8).cuda()
    assert d_rec.data_ptr() % 16 == 0
    ptrs = i64(torch, [0 if j in null else d_rec.data_ptr() + j * stride + (shift or {}).get(j, 0) for j in range(slots)])
    rec_caps = i64(torch, [stride - 32] * slots if caps is None else caps)
    rec_bytes = torch.full((slots,), -1, dtype=torch.int64).cuda()
    status = torch.full((slots,), -1, dtype=torch.int32).cuda()
    rc = ghf.lib().ghf_batch_seek_pack(ctx.h, C.byref(bidx), in_bytes.data_ptr(), count, e, ptrs.data_ptr(), rec_caps.data_ptr(),
                                       rec_bytes.data_ptr(), status.data_ptr())
    assert rc == 0, rc
    ctx.sync()
    h = d_rec.cpu().numpy()
    return status.cpu().numpy(), rec_bytes.cpu().numpy(), [h[j * stride : (j + 1) * stride] for j in range(slots)]


# ---- the worlds: items, a code, the oracle's bodies and records, computed once ---------------------------------------
class World:
    def __init__(self, torch, name, datas, code):
        self.name, self.datas, self.code = name, datas, code
        self.bodies = [orc_body(d, code) for d in datas]
        self.records = [orc_record(d, code) for d in datas]
        self.d_code = codes_to_device(torch, [code])


def skewed_items(sizes, seed):
    """two thirds of the bytes are one value: it gets the code of one bit"""
    rng = np.random.default_rng(seed)
    return [np.where(rng.random(n) < 0.67, np.uint8(7), rng.integers(0, 256, size=n, dtype=np.uint8)).astype(np.uint8) for n in sizes]


@pytest.fixture(scope="module")
def worlds(env):
    torch = env[2]
    sizes = SIZES + [MAX_ITEM]
    out = {}
    datas = skewed_items(sizes, seed=31)
    out["skewed"] = World(torch, "skewed", datas, cover_all_code(datas))
    assert out["skewed"].code.min_len == 1
    datas = [dg.make("uniform", n, seed=700 + k) for k, n in enumerate(sizes)]
    out["uniform"] = World(torch, "uniform", datas, cover_all_code(datas))
    assert 7 <= out["uniform"].code.min_len and out["uniform"].code.max_len <= 10
    code = orc.build_code(orc.histogram(CASES["fib32_maxlen32"]()))
    assert code.max_len == 32  # beyond the 12-bit table: tab_search runs
    used = np.array([s for s in range(256) if code.length[s]], dtype=np.uint8)
    rng = np.random.default_rng(32)
    datas = [used[rng.integers(0, used.size, size=n)] for n in sizes]
    datas[2] = np.full(128, next(s for s in range(256) if code.length[s] == 32), dtype=np.uint8)  # a run of 4096 bits, the longest
    out["fib32"] = World(torch, "fib32", datas, code)
    assert int(run_bits_of(datas[2], code)[0]) == 4096
    # a mixed code for the refusals (bad_codes wants min_len >= 2 and max_len >= min_len + 2)
    datas = [dg.make(["text", "zipf", "sym16", "uniform"][k % 4], n, seed=900 + k) for k, n in enumerate([300, 5000, 777, 4096, 9001, 129])]
    out["mixed"] = World(torch, "mixed", datas, cover_all_code(datas))
    return out


# ------------------------------------------------------------------------------ 1. pack
def test_pack_equals_the_oracles_records(env, worlds):
    """ghf_compress_batch_shared(index) -> ghf_batch_seek_pack: the oracle's records byte for byte, padding included, and
    nothing behind them; caps one byte short: GHF_E_CAP, nothing written; an index of ghf_compress_batch images:
    GHF_E_CORRUPT"""
    ghf, ctx, torch = env
    for name in ("skewed", "uniform"):
        w = worlds[name]
        datas, records = w.datas[: len(SIZES)], w.records[: len(SIZES)]
        tensors = [torch.from_numpy(d).cuda() for d in datas]
        bidx = ctx.batch_index_alloc(len(datas), max(SIZES))
        try:
            r = ctx.compress_batch_shared(tensors, w.d_code, max_item_bytes=max(SIZES), index=bidx)
            ctx.sync()
            assert r["status"].cpu().tolist() == [OK] * len(datas)
            h, nb = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
            for i, b in enumerate(w.bodies[: len(SIZES)]):  # the side-car is the one of the oracle's bodies
                assert np.array_equal(h[i * r["out_stride"] :][: int(nb[i])], b), (name, i)
            status, nbytes, slots = pack(env, bidx, r["in_bytes"])
            print(name, "pack: status", status.tolist(), "bytes", nbytes.tolist())
            assert status.tolist() == [OK] * len(datas)
            assert nbytes.tolist() == [rec.size for rec in records] == [ghf.batch_seek_bytes(d.size) for d in datas]
            for i, rec in enumerate(records):
                assert np.array_equal(slots[i][: rec.size], rec), (name, i, datas[i].size)
                assert np.all(slots[i][rec.size :] == GUARD), (name, i)
            # every cap one byte short, but item 3's
            caps = [rec.size - 1 for rec in records]
            caps[3] += 1
            status, nbytes, slots = pack(env, bidx, r["in_bytes"], caps=caps)
            assert status.tolist() == [OK if i == 3 else E_CAP for i in range(len(datas))]
            assert nbytes.tolist() == [records[3].size if i == 3 else 0 for i in range(len(datas))]
            for i in range(len(datas)):
                assert np.all(slots[i][records[3].size if i == 3 else 0 :] == GUARD), (name, i)
            assert np.array_equal(slots[3][: records[3].size], records[3])
            # per-slot refusals beside good neighbours: 0 bytes, more than a slice covers, a null and a misaligned pointer
            sizes = r["in_bytes"].clone()
            sizes[1], sizes[2] = 0, max(SIZES) + 1
            status, nbytes, slots = pack(env, bidx, sizes, null=(4,), shift={5: 8})
            assert status.tolist() == [OK, E_EMPTY, E_INVAL, OK, E_INVAL, E_INVAL] + [OK] * (len(datas) - 6)
            for i, rec in enumerate(records):
                good = status[i] == OK
                assert int(nbytes[i]) == (rec.size if good else 0), i
                assert np.array_equal(slots[i][: rec.size], rec) if good else np.all(slots[i] == GUARD), i
            # the images of ghf_compress_batch start behind their header: not the side-car of a body
            r2 = ctx.compress_batch(tensors, max_item_bytes=max(SIZES), index=bidx)
            ctx.sync()
            assert r2["status"].cpu().tolist() == [OK] * len(datas)
            status, nbytes, slots = pack(env, bidx, r["in_bytes"])
            assert status.tolist() == [E_CORRUPT] * len(datas) and np.all(nbytes == 0)
            assert all(np.all(s == GUARD) for s in slots)
        finally:
            ctx.batch_index_free(bidx)


# ------------------------------------------------------------------------------ 2. decode from oracle-made records
@pytest.mark.parametrize("name", ["skewed", "uniform", "fib32"])
def test_decode_from_the_oracles_bodies_and_records(env, worlds, name):
    """no library packer involved: the run, block and round edges, three rounds, one item of 1 MiB; a code of one bit, the
    8/9-bit codes of uniform bytes, codes of 32 bits"""
    w = worlds[name]
    check_round_trip(env, w.bodies, w.records, w.datas, w.d_code)


def test_stream_bytes_beyond_the_body_are_accepted(env, worlds):
    w = worlds["uniform"]
    k = len(SIZES)
    check_round_trip(env, w.bodies[:k], w.records[:k], w.datas[:k], w.d_code, stream_bytes=[b.size + 48 for b in w.bodies[:k]])


# ------------------------------------------------------------------------------ 3. cross-check
def test_packed_records_decode_to_what_the_other_decoders_give(env, worlds):
    ghf, ctx, torch = env
    w = worlds["mixed"]
    datas = w.datas
    tensors = [torch.from_numpy(d).cuda() for d in datas]
    bidx = ctx.batch_index_alloc(len(datas), 9001)
    try:
        r = ctx.compress_batch_shared(tensors, w.d_code, max_item_bytes=9001, index=bidx)
        p = ctx.batch_seek_pack(bidx, r["in_bytes"])
        sizes = ctx.decode_bodies_batch_shared_seek(r["out_ptrs"], r["out_bytes"], p["rec_ptrs"], p["rec_bytes"], w.d_code)
        mine = ctx.decode_bodies_batch_shared_seek(r["out_ptrs"], r["out_bytes"], p["rec_ptrs"], p["rec_bytes"], w.d_code, out=True,
                                                   caps=sizes["out_bytes"])
        car = ctx.decode_batch_shared(r["out_ptrs"], r["out_bytes"], w.d_code, bidx, r["in_bytes"])
        bsz = ctx.decode_bodies_batch_shared(r["out_ptrs"], r["out_bytes"], w.d_code)
        bod = ctx.decode_bodies_batch_shared(r["out_ptrs"], r["out_bytes"], w.d_code, out=True, caps=bsz["out_bytes"])
        ctx.sync()
        want = [d.size for d in datas]
        assert p["status"].cpu().tolist() == [OK] * len(datas)
        assert p["rec_bytes"].cpu().tolist() == [rec.size for rec in w.records]
        for res in (sizes, mine, car, bod):
            assert res["status"].cpu().tolist() == [OK] * len(datas) and res["out_bytes"].cpu().tolist() == want
        hm, hc, hb = mine["out"].cpu().numpy(), car["out"].cpu().numpy(), bod["out"].cpu().numpy()
        for i, d in enumerate(datas):
            got = hm[i * mine["out_stride"] :][: d.size]
            assert np.array_equal(got, d), i
            assert np.array_equal(hc[i * car["out_stride"] :][: d.size], got), i
            assert np.array_equal(hb[i * bod["out_stride"] :][: d.size], got), i
        with pytest.raises(ValueError):
            ctx.decode_bodies_batch_shared_seek(r["out_ptrs"], r["out_bytes"], p["rec_ptrs"], p["rec_bytes"], w.d_code, out=True)
    finally:
        ctx.batch_index_free(bidx)


# ------------------------------------------------------------------------------ 4. byte planes
class PlanesWorld:
    def __init__(self, torch, e):
        rng = np.random.default_rng(40 + e)
        self.e = e
        self.datas = [normal_elems(rng, n, e) for n in PLANE_ELEMS]
        h = np.zeros((e, 257), dtype=np.int64)
        for d in self.datas:
            for p in range(e):
                h[p, :256] += orc.histogram(np.ascontiguousarray(d[p::e]))[:256]
        h[h == 0] = 1
        h[:, 256] = 1
        self.codes = [orc.build_code(h[p]) for p in range(e)]
        planes = [(np.ascontiguousarray(d[p::e]), self.codes[p]) for d in self.datas for p in range(e)]  # slot i * e + p
        self.bodies = [orc_body(b, c) for b, c in planes]
        self.records = [orc_record(b, c) for b, c in planes]
        self.d_codes = codes_to_device(torch, self.codes)


@pytest.fixture(scope="module")
def planes_worlds(env):
    return {e: PlanesWorld(env[2], e) for e in ES}


@pytest.mark.parametrize("e", ES)
def test_planes_pack_and_decode_against_the_oracle(env, planes_worlds, e):
    ghf, ctx, torch = env
    w = planes_worlds[e]
    # decode from the oracle's per-plane bodies and records, byte-exact at unaligned addresses
    check_round_trip(env, w.bodies, w.records, w.datas, w.d_codes, e=e)
    # pack: the library's packer writes the oracle's bodies, and its side-car packs to the oracle's records
    max_item = max(PLANE_ELEMS) * e
    tensors = [torch.from_numpy(d).cuda() for d in w.datas]
    bidx = ctx.batch_index_alloc(len(w.datas) * e, max_item // e)
    try:
        r = ctx.compress_batch_planes_shared(tensors, w.d_codes, e, max_item_bytes=max_item, index=bidx)
        ctx.sync()
        assert r["status"].cpu().tolist() == [OK] * (len(w.datas) * e)
        h, nb = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
        for j, b in enumerate(w.bodies):
            assert np.array_equal(h[j * r["out_stride"] :][: int(nb[j])], b), j
        status, nbytes, slots = pack(env, bidx, r["in_bytes"], e=e)
        assert status.tolist() == [OK] * (len(w.datas) * e)
        assert nbytes.tolist() == [rec.size for rec in w.records]
        for j, rec in enumerate(w.records):
            assert np.array_equal(slots[j][: rec.size], rec), j
            assert np.all(slots[j][rec.size :] == GUARD), j
        # an item whose size is no whole number of elements: GHF_E_INVAL on all its slots, nothing written
        sizes = r["in_bytes"].clone()
        sizes[4] += 1
        status, nbytes, slots = pack(env, bidx, sizes, e=e)
        assert status.tolist() == [E_INVAL if j // e == 4 else OK for j in range(len(w.datas) * e)]
        assert all(np.all(slots[4 * e + p] == GUARD) and nbytes[4 * e + p] == 0 for p in range(e))
        # the wrapper, end to end
        p = ctx.batch_seek_pack(bidx, r["in_bytes"], elem_bytes=e)
        sz = ctx.decode_bodies_batch_planes_shared_seek(r["out_ptrs"], r["out_bytes"], p["rec_ptrs"], p["rec_bytes"], w.d_codes, e)
        dec = ctx.decode_bodies_batch_planes_shared_seek(r["out_ptrs"], r["out_bytes"], p["rec_ptrs"], p["rec_bytes"], w.d_codes, e, out=True,
                                                         caps=sz["out_bytes"])
        ctx.sync()
        assert dec["status"].cpu().tolist() == [OK] * len(w.datas) == sz["status"].cpu().tolist()
        assert dec["out_bytes"].cpu().tolist() == [d.size for d in w.datas] == sz["out_bytes"].cpu().tolist()
        ho = dec["out"].cpu().numpy()
        for i, d in enumerate(w.datas):
            assert np.array_equal(ho[i * dec["out_stride"] :][: d.size], d), i
    finally:
        ctx.batch_index_free(bidx)


@pytest.mark.parametrize("e", ES)
def test_planes_refusals_are_per_item(env, planes_worlds, e):
    ghf, ctx, torch = env
    w = planes_worlds[e]
    nitems = len(w.datas)
    bodies, records = list(w.bodies), list(w.records)
    sizes, shift, rshift = [None] * len(bodies), [0] * len(bodies), [0] * len(bodies)
    last = e - 1
    # item 1 (127 elements): the record of its last plane says 126 symbols -- a well-formed record, but the planes disagree
    n1 = PLANE_ELEMS[1]
    records[1 * e + last] = record_of(run_bits_of(np.ascontiguousarray(w.datas[1][last::e])[: n1 - 1], w.codes[last]), n1 - 1)
    # item 2: a wrong magic in plane 0; item 3: the last plane's body cut one byte short; item 4: a misaligned record
    records[2 * e] = record_of(run_bits_of(np.ascontiguousarray(w.datas[2][0::e]), w.codes[0]), PLANE_ELEMS[2], magic=MAGIC + 1)
    bodies[3 * e + last] = bodies[3 * e + last][:-1]
    rshift[4 * e + last] = 8
    caps = [d.size for d in w.datas]
    caps[5] -= 1  # item 5 (40 000 elements): a cap one byte short
    want = [OK, E_CORRUPT, E_FORMAT, E_CORRUPT, E_INVAL, E_CAP]
    bo, ro = Packed(torch, bodies, sizes=sizes, shift=shift), Packed(torch, records, shift=rshift)
    status, nbytes, outs, guards = run(env, bo, ro, w.d_codes, caps=caps, e=e)
    print("status", status.tolist(), "want", want, "bytes", nbytes.tolist())
    assert status.tolist() == want
    assert nbytes.tolist() == [w.datas[0].size, 0, 0, 0, 0, 0]
    assert np.array_equal(outs[0], w.datas[0])
    for i in range(nitems):
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    for i in (1, 2, 4, 5):  # refused before the first store
        assert np.all(outs[i] == GUARD), i
    # a code that is not complete, in the last plane only: GHF_E_FORMAT on every item, nothing written
    bad = ghf.Code.from_buffer_copy(bytes(w.codes[last]))
    bad.length[next(s for s in range(256) if bad.length[s] == bad.max_len)] -= 1  # one length shortened: Kraft above 1
    d_bad = codes_to_device(torch, list(w.codes[:last]) + [bad])
    bo, ro = Packed(torch, w.bodies), Packed(torch, w.records)
    status, nbytes, outs, guards = run(env, bo, ro, d_bad, caps=[d.size for d in w.datas], e=e)
    assert status.tolist() == [E_FORMAT] * nitems and np.all(nbytes == 0)
    assert all(np.all(o == GUARD) for o in outs)
    status, nbytes, _, _ = run(env, bo, ro, d_bad, e=e)
    assert status.tolist() == [E_FORMAT] * nitems and np.all(nbytes == 0)


# ------------------------------------------------------------------------------ 5. refusals, flat
def test_refusals_are_per_item(env, worlds):
    ghf, ctx, torch = env
    w = worlds["mixed"]
    code, d_code = w.code, w.d_code
    good, B, R = w.datas, w.bodies, w.records
    big = good[4]  # 9001 bytes: 71 runs
    bits = run_bits_of(big, code)

    def rec_with(change):
        b = bits.copy()
        change(b)
        return record_of(b, big.size)

    def swap(b):
        b[10] += 1
        b[11] -= 1

    def far(b):
        b[20] = 0xFFFF

    assert 8 * B[4].size < bits[:20].sum() + 0xFFFF  # the run sum points past the stream
    no_end = orc_body(np.concatenate([big, big[:8]]), code)  # data bits where the end mark should be
    over = ghf.compress_batch_shared_bound(MAX_ITEM) + 1
    #          body      stream_bytes  record                                       rec_bytes        data     cap           shifts  null out  want       sizes only
    items = [(B[0],      None,         R[0],                                        None,            good[0], None,         (0, 0), False,    OK,        OK),
             (B[4],      None,         record_of(bits, big.size, magic=MAGIC ^ 1),  None,            big,     None,         (0, 0), False,    E_FORMAT,  E_FORMAT),
             (B[4],      None,         record_of(bits, 0),                          None,            big,     None,         (0, 0), False,    E_FORMAT,  E_FORMAT),
             (B[1],      None,         R[1],                                        None,            good[1], None,         (0, 0), False,    OK,        OK),
             (B[4],      None,         record_of(bits, MAX_ITEM + 1),               None,            big,     None,         (0, 0), False,    E_FORMAT,  E_FORMAT),
             (B[4],      None,         R[4],                                        R[4].size + 8,   big,     None,         (0, 0), False,    E_FORMAT,  E_FORMAT),
             (B[4],      None,         R[4],                                        R[4].size - 8,   big,     None,         (0, 0), False,    E_FORMAT,  E_FORMAT),
             (B[2],      None,         R[2],                                        None,            good[2], None,         (0, 0), False,    OK,        OK),
             (B[4],      None,         rec_with(swap),                              None,            big,     None,         (0, 0), False,    E_CORRUPT, OK),
             (B[4],      None,         rec_with(far),                               None,            big,     None,         (0, 0), False,    E_CORRUPT, OK),
             (B[4][:-1], None,         R[4],                                        None,            big,     None,         (0, 0), False,    E_CORRUPT, OK),
             (no_end,    None,         R[4],                                        None,            big,     None,         (0, 0), False,    E_CORRUPT, OK),
             (B[3],      None,         R[3],                                        None,            good[3], None,         (0, 0), False,    OK,        OK),
             (B[4],      None,         R[4],                                        None,            big,     big.size - 1, (0, 0), False,    E_CAP,     OK),
             (None,      100,          R[4],                                        None,            big,     None,         (0, 0), False,    E_INVAL,   E_INVAL),
             (B[4],      None,         None,                                        72,              big,     None,         (0, 0), False,    E_INVAL,   E_INVAL),
             (B[4],      None,         R[4],                                        None,            big,     None,         (8, 0), False,    E_INVAL,   E_INVAL),
             (B[4],      None,         R[4],                                        None,            big,     None,         (0, 8), False,    E_INVAL,   E_INVAL),
             (B[4],      over,         R[4],                                        None,            big,     None,         (0, 0), False,    E_INVAL,   E_INVAL),
             (B[4],      None,         R[4],                                        None,            big,     None,         (0, 0), True,     E_INVAL,   OK),
             (B[5],      None,         R[5],                                        None,            good[5], None,         (0, 0), False,    OK,        OK)]
    bo = Packed(torch, [it[0] for it in items], sizes=[it[1] for it in items], shift=[it[6][0] for it in items])
    ro = Packed(torch, [it[2] for it in items], sizes=[it[3] for it in items], shift=[it[6][1] for it in items])
    caps = [it[4].size if it[5] is None else it[5] for it in items]
    want, want0 = [it[8] for it in items], [it[9] for it in items]
    null_out = tuple(i for i, it in enumerate(items) if it[7])
    status, nbytes, outs, guards = run(env, bo, ro, d_code, caps=caps, null_out=null_out)  # run() ends with ctx.sync(): it stays OK
    print("status", status.tolist(), "want", want, "bytes", nbytes.tolist())
    assert status.tolist() == want
    for i, it in enumerate(items):
        if want[i] == OK:
            assert int(nbytes[i]) == it[4].size and np.array_equal(outs[i], it[4]), i
        else:
            assert int(nbytes[i]) == 0, i
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i  # nothing at or beyond the cap
        if want[i] in (E_FORMAT, E_INVAL, E_CAP):  # refused before anything was stored
            assert np.all(outs[i] == GUARD), i
    # sizes only: the records' shapes alone; neither the stream's bits nor the cap nor the output pointer plays a part
    status, nbytes, _, _ = run(env, bo, ro, d_code)
    print("sizes only: status", status.tolist(), "want", want0, "bytes", nbytes.tolist())
    assert status.tolist() == want0
    assert nbytes.tolist() == [it[4].size if s == OK else 0 for it, s in zip(items, want0)]
    assert ghf.lib().ghf_sync(ctx.h) == OK


def test_a_code_that_is_not_complete_is_refused_on_every_item(env, worlds):
    ghf, ctx, torch = env
    w = worlds["mixed"]
    good = ghf.Code.from_buffer_copy(bytes(w.code))
    lone = ghf.Code()  # the one-symbol code of GHF_EMPTY_OK: the end mark alone, code "0"
    for i in range(257):
        lone.symbol[i] = 0xFFFFFFFF
    lone.symbol[0] = 256
    lone.length[256] = 1
    lone.min_len = lone.max_len = 1
    bo, ro = Packed(torch, w.bodies), Packed(torch, w.records)
    n = len(w.datas)
    for name, c in bad_codes(good, ghf.Code.from_buffer_copy) + [("the lone end mark of GHF_EMPTY_OK", lone)]:
        d_bad = codes_to_device(torch, [c])
        status, nbytes, outs, guards = run(env, bo, ro, d_bad, caps=[d.size for d in w.datas])
        assert status.tolist() == [E_FORMAT] * n, name
        assert np.all(nbytes == 0), name
        for i in range(n):
            assert np.all(outs[i] == GUARD) and np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (name, i)
        status, nbytes, _, _ = run(env, bo, ro, d_bad)
        assert status.tolist() == [E_FORMAT] * n and np.all(nbytes == 0), name
    assert ghf.lib().ghf_sync(ctx.h) == OK


# ------------------------------------------------------------------------------ 6. call level
def test_call_level(env, worlds):
    ghf, ctx, torch = env
    L = ghf.lib()
    w = worlds["mixed"]
    n = len(w.datas)
    bo, ro = Packed(torch, w.bodies), Packed(torch, w.records)
    d_out = torch.full((n * 9008 + 64,), GUARD, dtype=torch.uint8).cuda()
    out_ptrs = i64(torch, [d_out.data_ptr() + i * 9008 for i in range(n)])
    out_caps = i64(torch, [9008] * n)
    out_bytes = torch.full((n,), -1, dtype=torch.int64).cuda()
    status = torch.full((n,), -1, dtype=torch.int32).cuda()
    a = [ctx.h, bo.ptrs.data_ptr(), bo.bytes.data_ptr(), ro.ptrs.data_ptr(), ro.bytes.data_ptr(), w.d_code.data_ptr(), n,
         out_ptrs.data_ptr(), out_caps.data_ptr(), out_bytes.data_ptr(), status.data_ptr()]

    def call(**kw):
        b = list(a)
        for k, v in kw.items():
            b[int(k[1:])] = v
        return L.ghf_decode_bodies_batch_shared_seek(*b)

    assert call(_6=0) == OK  # count == 0 queues nothing
    for k in ("_1", "_2", "_3", "_4", "_9", "_10"):
        assert call(**{k: None}) == E_INVAL, k
    assert call(_8=None) == E_INVAL  # output pointers without caps
    assert call(_5=None) == E_INVAL and call(_5=w.d_code.data_ptr() + 8) == E_INVAL  # a null or misaligned d_code
    assert call(_5=None, _6=0) == E_INVAL  # the argument checks come before the count
    assert L.ghf_decode_bodies_batch_shared_seek(None, *a[1:]) == E_INVAL
    planes = L.ghf_decode_bodies_batch_planes_shared_seek
    assert planes(*a[:7], 3, *a[7:]) == E_INVAL and planes(*a[:7], 1, *a[7:]) == E_INVAL  # elem_bytes is 2, 4 or 8
    bidx = ctx.batch_index_alloc(n, 9001)
    try:
        rec = torch.full((n * 160,), GUARD, dtype=torch.uint8).cuda()
        rp, rc_, rb, rs = i64(torch, [rec.data_ptr() + 160 * i for i in range(n)]), i64(torch, [160] * n), out_bytes.clone(), status.clone()
        sizes = i64(torch, [d.size for d in w.datas])
        p = [ctx.h, C.byref(bidx), sizes.data_ptr(), n, 1, rp.data_ptr(), rc_.data_ptr(), rb.data_ptr(), rs.data_ptr()]
        for k in (1, 2, 5, 6, 7, 8):
            assert L.ghf_batch_seek_pack(*[None if j == k else v for j, v in enumerate(p)]) == E_INVAL, k
        assert L.ghf_batch_seek_pack(*p[:4], 3, *p[5:]) == E_INVAL  # elem_bytes is 1, 2, 4 or 8
        assert L.ghf_batch_seek_pack(*p[:3], n + 1, *p[4:]) == E_INVAL  # the index does not cover the count
        assert L.ghf_batch_seek_pack(*p[:4], 2, *p[5:]) == E_INVAL  # ... nor count * elem_bytes slots
        assert L.ghf_batch_seek_pack(*p[:3], 0, *p[4:]) == OK
        ctx.sync()
        assert np.all(rec.cpu().numpy() == GUARD) and np.all(rs.cpu().numpy() == -1)
    finally:
        ctx.batch_index_free(bidx)
    ctx.sync()
    assert np.all(status.cpu().numpy() == -1) and np.all(out_bytes.cpu().numpy() == -1) and np.all(d_out.cpu().numpy() == GUARD)
    assert call() == OK  # the context is usable afterwards
    ctx.sync()
    assert status.cpu().tolist() == [OK] * n and out_bytes.cpu().tolist() == [d.size for d in w.datas]
    h = d_out.cpu().numpy()
    for i, d in enumerate(w.datas):
        assert np.array_equal(h[i * 9008 :][: d.size], d), i
        assert np.all(h[i * 9008 + d.size : (i + 1) * 9008] == GUARD), i
