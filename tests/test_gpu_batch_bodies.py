"""GPU: ghf_decode_bodies_batch_shared -- bodies under ONE code decoded from nothing but their bytes, one launch per call.

Expected values come from the CPU oracle through oracle.lib() (orc_histogram, orc_build_code, orc_encode_body; pinned to
the reference by tests/test_oracle_golden.py) and from the reference's recorded files (tests/golden/golden.json), never
from the library's packer: every body the call is given was written by orc_encode_body or by the reference.  The
library's other paths (ghf_decode_images_batch, ghf_compress_batch_shared + ghf_decode_batch_shared) are cross-checks
only.  Streams are 16-byte aligned; outputs sit at odd addresses between guard bytes that are checked after every call."""
import base64
import ctypes as C
import hashlib

import numpy as np
import pytest

import datagen as dg
import pkgload
from cases import CASES
from header_cases import bad_codes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_CAP, E_FORMAT, E_CORRUPT = 0, 1, 5, 6, 7
GUARD = 0xA5
MAX_ITEM = 1 << 20
ROUND_BITS = 256 * 512


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


def small_items(count, seed):
    """the recipe of tests/test_gpu_batch_shared.py: `count` seeded items of 1..8192 bytes, mixed kinds; every seventh
    folded to a few values"""
    out = []
    for i in range(count):
        n = int(dg.splitmix64(np.uint64(seed + i)) % np.uint64(8192)) + 1
        kind = ["uniform", "zipf", "sym16", "text"][i % 4]
        d = dg.make(kind, n, seed=seed + 7 * i)
        if i % 7 == 0:
            d = d % np.uint8(1 + i % 5)
        out.append(d)
    return out


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


def code_to_device(torch, code):
    """any ctypes code struct (ghf.Code, orc.OrcCode: the same layout) -> a CUDA uint8 tensor"""
    t = torch.from_numpy(np.frombuffer(bytes(code), dtype=np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def data_bits(data, code):
    return int(np.asarray(list(code.length), dtype=np.int64)[data].sum())


def item_of_bits(code, bits, seed):
    """a data item whose codes take exactly `bits` bits under `code`: a random walk, then a tail found by coin change"""
    lens = sorted({int(code.length[s]) for s in range(256) if code.length[s]})
    by_len = {l: [s for s in range(256) if code.length[s] == l] for l in lens}
    rng = np.random.default_rng(seed)
    out, left = [], bits
    while left > 6 * lens[-1]:
        s = int(rng.integers(0, 256))
        if code.length[s]:
            out.append(s)
            left -= int(code.length[s])
    reach = {0: []}
    for t in range(1, left + 1):
        for l in lens:
            if t - l in reach:
                reach[t] = reach[t - l] + [l]
                break
    assert left in reach, (bits, lens)
    out += [by_len[l][int(rng.integers(0, len(by_len[l])))] for l in reach[left]]
    d = np.array(out, dtype=np.uint8)
    assert data_bits(d, code) == bits
    return d


# ---- the call ---------------------------------------------------------------------------------------------------------
class Bodies:
    """bodies (host uint8 arrays) packed into one device buffer, each at a 16-byte aligned address, GUARD between them; a
    None body is a null pointer"""

    def __init__(self, torch, bodies, stream_bytes=None, shift=None):
        self.count = len(bodies)
        self.offs, at = [], 0
        for k, b in enumerate(bodies):
            self.offs.append(at + (shift[k] if shift else 0))
            at += ((0 if b is None else b.size) + 15 & ~15) + 64
        packed = np.full(at + 64, GUARD, dtype=np.uint8)
        for o, b in zip(self.offs, bodies):
            if b is not None:
                packed[o : o + b.size] = b
        self.d = torch.from_numpy(packed).cuda()
        assert self.d.data_ptr() % 16 == 0
        self.ptrs = i64(torch, [0 if b is None else self.d.data_ptr() + o for o, b in zip(self.offs, bodies)])
        self.sizes = [(0 if b is None else int(b.size)) if stream_bytes is None or stream_bytes[k] is None else int(stream_bytes[k])
                      for k, b in enumerate(bodies)]
        self.bytes = i64(torch, self.sizes)


def run(env, bo, d_code, caps=None, null_out=()):
    """one ghf_decode_bodies_batch_shared call; caps=None: sizes only.  Every output sits at an address misaligned by
    1..15 between GUARD bytes.  -> (status, out_bytes, outputs cut to their caps, guards (front, behind the cap))"""
    ghf, ctx, torch = env
    n = bo.count
    out_bytes = torch.full((n,), -1, dtype=torch.int64).cuda()
    status = torch.full((n,), -1, dtype=torch.int32).cuda()
    fn = ghf.lib().ghf_decode_bodies_batch_shared
    if caps is None:
        rc = fn(ctx.h, bo.ptrs.data_ptr(), bo.bytes.data_ptr(), d_code.data_ptr(), n, None, None, out_bytes.data_ptr(), status.data_ptr())
        assert rc == 0, rc
        ctx.sync()  # raises if the context's status word was latched: per-item failures must not do that
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
    rc = fn(ctx.h, bo.ptrs.data_ptr(), bo.bytes.data_ptr(), d_code.data_ptr(), n, out_ptrs.data_ptr(), out_caps.data_ptr(),
            out_bytes.data_ptr(), status.data_ptr())
    assert rc == 0, rc
    ctx.sync()
    h = d_out.cpu().numpy()
    ends = [s[0] for s in slots[1:]] + [h.size]
    outs = [h[s[1] : s[2]] for s in slots]
    guards = [(h[s[0] : s[1]], h[s[2] : e]) for s, e in zip(slots, ends)]
    return status.cpu().numpy(), out_bytes.cpu().numpy(), outs, guards


def check_round_trip(env, bodies, datas, d_code, labels=None, stream_bytes=None):
    """sizes-only call -> the input sizes; decode call into exactly those caps -> the inputs, guards intact"""
    labels = labels or ["item %d (%d bytes)" % (i, d.size) for i, d in enumerate(datas)]
    bo = Bodies(env[2], bodies, stream_bytes=stream_bytes)
    status, nbytes, _, _ = run(env, bo, d_code)
    bad = [(labels[i], int(status[i]), int(nbytes[i])) for i, d in enumerate(datas) if status[i] != OK or nbytes[i] != d.size]
    print("sizes:  %d items, %d wrong %s" % (len(datas), len(bad), bad[:8]))
    assert not bad
    status, nbytes, outs, guards = run(env, bo, d_code, caps=[d.size for d in datas])
    bad = [(labels[i], int(status[i]), int(nbytes[i])) for i, d in enumerate(datas) if status[i] != OK or nbytes[i] != d.size]
    print("decode: %d items, %d wrong %s" % (len(datas), len(bad), bad[:8]))
    assert not bad
    for i, d in enumerate(datas):
        assert np.array_equal(outs[i], d), labels[i]
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), labels[i]


@pytest.fixture(scope="module")
def bulk(env):
    """1024 mixed items of 1..8192 bytes under one COVER_ALL code; bodies from orc_encode_body"""
    datas = small_items(1024, seed=21000)
    code = cover_all_code(datas)
    return datas, code, [orc_body(d, code) for d in datas], code_to_device(env[2], code)


# ------------------------------------------------------------------------------ 1. edges
def test_edge_sizes_and_bit_edges(env, bulk):
    """1 .. 65 bytes; bodies whose data bits, and whose bits with the end mark, are 511 .. 513 and 1023 .. 1025: the end
    mark starts, or ends, one bit either side of a subsequence's edge"""
    _, code, _, d_code = bulk
    end_len = int(code.length[256])
    datas = [dg.make(["uniform", "zipf", "sym16", "text"][k % 4], n, seed=500 + k) for k, n in enumerate([1, 15, 16, 17, 63, 64, 65])]
    labels = ["%d bytes" % d.size for d in datas]
    for t in (511, 512, 513, 1023, 1024, 1025):
        datas += [item_of_bits(code, t, seed=t), item_of_bits(code, t - end_len, seed=2000 + t)]
        labels += ["data ends at bit %d" % t, "end mark ends at bit %d" % t]
    bodies = [orc_body(d, code) for d in datas]
    for d, b, l in zip(datas, bodies, labels):
        assert b.size == -(-(data_bits(d, code) + end_len) // 8), l
    check_round_trip(env, bodies, datas, d_code, labels)


def test_rounds_and_the_carry_across_them(env):
    """uniform bytes under their own 8/9-bit code, the slow-settling case: 20 KiB and 40 KiB are two and three rounds with
    a code that crosses the round's edge; 40 000 bytes likewise; one item of 1 MiB"""
    datas = [dg.make("uniform", n, seed=600 + k) for k, n in enumerate([20 * 1024 + 3, 40 * 1024 + 5, 40000, MAX_ITEM])]
    code = cover_all_code(datas)
    assert 7 <= code.min_len and code.max_len <= 10
    bodies = [orc_body(d, code) for d in datas]
    assert [-(-8 * b.size // ROUND_BITS) for b in bodies[:3]] == [2, 3, 3]
    ends = np.cumsum(np.asarray(list(code.length), dtype=np.int64)[datas[1]])
    assert ROUND_BITS not in ends and 2 * ROUND_BITS not in ends  # a code straddles each round's edge: the carry is not 0
    check_round_trip(env, bodies, datas, code_to_device(env[2], code))


def test_one_bit_codes_slice_the_stage(env):
    """200 000 bytes of two skewed values under their own code: about one bit per symbol, so a round holds far more than
    the 16 Ki symbols of the stage"""
    rng = np.random.default_rng(61)
    d = np.where(rng.random(200000) < 0.04, np.uint8(200), np.uint8(7)).astype(np.uint8)
    code = orc.build_code(orc.histogram(d))
    assert code.length[7] == 1 and code.max_len == 2
    body = orc_body(d, code)
    assert 200000 < 8 * body.size < 1.1 * 200000 and ROUND_BITS / 1.1 > 4 * 16384
    check_round_trip(env, [body, body[:]], [d, d], code_to_device(env[2], code))


# ------------------------------------------------------------------------------ 2. bulk
def test_1024_mixed_items(env, bulk):
    datas, code, bodies, d_code = bulk
    check_round_trip(env, bodies, datas, d_code)


# ------------------------------------------------------------------------------ 3. codes of 32 bits
def test_codes_of_32_bits(env):
    """the search beyond the 12-bit table, with the code of the golden case fib32_maxlen32"""
    code = orc.build_code(orc.histogram(CASES["fib32_maxlen32"]()))
    assert code.max_len == 32
    rarest = next(s for s in range(256) if code.length[s] == 32)
    used = [s for s in range(256) if code.length[s]]
    rng = np.random.default_rng(32)
    mixed = np.array(used, dtype=np.uint8)[rng.integers(0, len(used), size=9001)]
    datas = [np.full(4097, rarest, dtype=np.uint8), mixed, mixed[:1]]
    bodies = [orc_body(d, code) for d in datas]
    assert bodies[0].size == 4 * 4097 + -(-int(code.length[256]) // 8)
    check_round_trip(env, bodies, datas, code_to_device(env[2], code))


# ------------------------------------------------------------------------------ 4. files the reference wrote
def test_reference_written_files(env, golden):
    """the code from ghf_parse_header, copied up; the body behind the header, copied to an aligned buffer -> the input"""
    ghf, ctx, torch = env
    names = [k for k in golden if "crs2_b64" in golden[k] and golden[k]["n"] <= MAX_ITEM]
    assert len(names) >= 4
    for k in names:
        g = golden[k]
        img = np.frombuffer(base64.b64decode(g["crs2_b64"]), dtype=np.uint8)
        assert img.size == g["crs2_bytes"] and sha(img) == g["crs2_sha256"], k
        code, hs = ghf.parse_header(img)
        assert hs == g["header_bytes"], k
        data = CASES[k]()
        assert data.size == g["n"] and sha(data) == g["input_sha256"] == g["decoded_sha256"], k
        check_round_trip(env, [img[hs:].copy()], [data], code_to_device(torch, code), [k])


# ------------------------------------------------------------------------------ 5. cross-checks
def test_same_bytes_as_the_images_call_and_the_side_car_call(env, bulk):
    ghf, ctx, torch = env
    datas, code, bodies, d_code = bulk[0][:256], bulk[1], bulk[2][:256], bulk[3]
    # the library's packer under the same code: the same bodies, and a live side-car
    tensors = [torch.from_numpy(d).cuda() for d in datas]
    bidx = ctx.batch_index_alloc(len(datas), 8192)
    try:
        r = ctx.compress_batch_shared(tensors, d_code, max_item_bytes=8192, index=bidx)
        ctx.sync()
        assert r["status"].cpu().tolist() == [OK] * len(datas)
        h, nb = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
        for i, b in enumerate(bodies):
            assert np.array_equal(h[i * r["out_stride"] :][: int(nb[i])], b), i
        sizes = ctx.decode_bodies_batch_shared(r["out_ptrs"], r["out_bytes"], d_code)
        mine = ctx.decode_bodies_batch_shared(r["out_ptrs"], r["out_bytes"], d_code, out=True, caps=sizes["out_bytes"])
        car = ctx.decode_batch_shared(r["out_ptrs"], r["out_bytes"], d_code, bidx, r["in_bytes"])
        ctx.sync()
        assert mine["status"].cpu().tolist() == [OK] * len(datas) == car["status"].cpu().tolist()
        assert mine["out_bytes"].cpu().tolist() == [d.size for d in datas] == car["out_bytes"].cpu().tolist()
        hm, hc = mine["out"].cpu().numpy(), car["out"].cpu().numpy()
        for i, d in enumerate(datas):
            got = hm[i * mine["out_stride"] :][: d.size]
            assert np.array_equal(got, d), i
            assert np.array_equal(hc[i * car["out_stride"] :][: d.size], got), i
    finally:
        ctx.batch_index_free(bidx)
    # header || body through ghf_decode_images_batch
    hdr = orc.header_bytes(code)
    assert hdr.size % 8 == 0
    images = [np.concatenate((hdr, b)) for b in bodies]
    stride = (max(im.size for im in images) + 15 & ~15) + 16
    packed = np.zeros(len(images) * stride, dtype=np.uint8)
    for i, im in enumerate(images):
        packed[i * stride : i * stride + im.size] = im
    d = torch.from_numpy(packed).cuda()
    ptrs = i64(torch, [d.data_ptr() + i * stride for i in range(len(images))])
    nbytes = i64(torch, [im.size for im in images])
    isz = ctx.decode_images_batch(ptrs, nbytes)
    idec = ctx.decode_images_batch(ptrs, nbytes, out=True, caps=isz["out_bytes"])
    ctx.sync()
    assert idec["status"].cpu().tolist() == [OK] * len(images)
    assert idec["out_bytes"].cpu().tolist() == mine["out_bytes"].cpu().tolist()
    hi = idec["out"].cpu().numpy()
    for i, dd in enumerate(datas):
        assert np.array_equal(hi[i * idec["out_stride"] :][: dd.size], hm[i * mine["out_stride"] :][: dd.size]), i


def test_bytes_behind_the_end_mark_change_nothing(env, bulk):
    datas, code, bodies, d_code = bulk[0][:256], bulk[1], bulk[2][:256], bulk[3]
    rng = np.random.default_rng(11)
    longer = [np.concatenate([b, rng.integers(0, 256, size=1 + i % 40, dtype=np.uint8)]) for i, b in enumerate(bodies)]
    check_round_trip(env, longer, datas, d_code)
    # and a stream_bytes that reaches into the guard bytes behind the body
    check_round_trip(env, bodies, datas, d_code, stream_bytes=[b.size + 48 for b in bodies])


# ------------------------------------------------------------------------------ 6. per-item failures
def test_failures_are_per_item(env, bulk):
    ghf, ctx, torch = env
    code, d_code = bulk[1], bulk[3]
    good = small_items(6, seed=4100)
    t = dg.make("text", 7000, seed=92)
    u = dg.make("uniform", 3000, seed=77)
    z = dg.make("zipf", 5000, seed=78)
    none = np.zeros(0, dtype=np.uint8)
    B = lambda d: orc_body(d, code)
    end_only = B(none)
    assert end_only.size == -(-int(code.length[256]) // 8)
    over = ghf.compress_batch_shared_bound(MAX_ITEM) + 1
    #          body          stream_bytes  data     cap          shift  null out  want       want, sizes only
    items = [(B(good[0]),    None,         good[0], None,        0,     False,    OK,        OK),
             (None,          100,          z,       None,        0,     False,    E_INVAL,   E_INVAL),
             (B(good[1]),    None,         good[1], None,        0,     False,    OK,        OK),
             (B(z),          None,         z,       None,        8,     False,    E_INVAL,   E_INVAL),
             (B(u),          over,         u,       None,        0,     False,    E_INVAL,   E_INVAL),
             (B(good[2]),    None,         good[2], None,        0,     False,    OK,        OK),
             (B(z),          None,         z,       None,        0,     True,     E_INVAL,   OK),
             (B(u),          None,         u,       u.size - 1,  0,     False,    E_CAP,     OK),
             (B(good[3]),    None,         good[3], None,        0,     False,    OK,        OK),
             (B(t)[:-1],     None,         t,       None,        0,     False,    E_CORRUPT, E_CORRUPT),
             (B(t),          0,            t,       None,        0,     False,    E_CORRUPT, E_CORRUPT),
             (B(good[4]),    None,         good[4], None,        0,     False,    OK,        OK),
             (end_only,      None,         none,    64,          0,     False,    OK,        OK),
             (B(good[5]),    None,         good[5], None,        0,     False,    OK,        OK)]
    bodies = [it[0] for it in items]
    caps = [it[2].size if it[3] is None else it[3] for it in items]
    want, want0 = [it[6] for it in items], [it[7] for it in items]
    bo = Bodies(torch, bodies, stream_bytes=[it[1] for it in items], shift=[it[4] for it in items])
    null_out = tuple(i for i, it in enumerate(items) if it[5])
    status, nbytes, outs, guards = run(env, bo, d_code, caps=caps, null_out=null_out)  # run() ends with ctx.sync(): it stays OK
    print("status", status.tolist(), "want", want, "bytes", nbytes.tolist())
    assert status.tolist() == want
    for i, it in enumerate(items):
        if want[i] == OK:
            assert int(nbytes[i]) == it[2].size and np.array_equal(outs[i][: it[2].size], it[2]), i
            assert np.all(outs[i][it[2].size :] == GUARD), i  # only out[0 .. n) is written
        else:
            assert int(nbytes[i]) == 0, i
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i  # nothing at or beyond the cap
    for i in (1, 3, 4, 6):  # refused before anything was written
        assert np.all(outs[i] == GUARD), i
    # sizes only: neither the cap nor the output pointer plays a part, the true count comes back
    status, nbytes, _, _ = run(env, bo, d_code)
    print("sizes only: status", status.tolist(), "want", want0, "bytes", nbytes.tolist())
    assert status.tolist() == want0
    assert nbytes.tolist() == [it[2].size if w == OK else 0 for it, w in zip(items, want0)]


def test_a_code_that_is_not_complete_is_refused_on_every_item(env, bulk):
    ghf, ctx, torch = env
    datas, code, bodies = bulk[0][12:18], bulk[1], bulk[2][12:18]
    good = ghf.Code.from_buffer_copy(bytes(code))
    lone = ghf.Code()  # the one-symbol code of GHF_EMPTY_OK: the end mark alone, code "0"
    for i in range(257):
        lone.symbol[i] = 0xFFFFFFFF
    lone.symbol[0] = 256
    lone.length[256] = 1
    lone.min_len = lone.max_len = 1
    bo = Bodies(torch, bodies)
    for name, c in bad_codes(good, ghf.Code.from_buffer_copy) + [("the lone end mark of GHF_EMPTY_OK", lone)]:
        d_bad = code_to_device(torch, c)
        status, nbytes, outs, guards = run(env, bo, d_bad, caps=[d.size for d in datas])
        assert status.tolist() == [E_FORMAT] * len(datas), name
        assert np.all(nbytes == 0), name
        for i in range(len(datas)):
            assert np.all(outs[i] == GUARD) and np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (name, i)
        status, nbytes, _, _ = run(env, bo, d_bad)
        assert status.tolist() == [E_FORMAT] * len(datas) and np.all(nbytes == 0), name


# ------------------------------------------------------------------------------ 7. call level, wrapper, counters
def test_call_level(env, bulk):
    ghf, ctx, torch = env
    L = ghf.lib()
    datas, code, bodies, d_code = bulk[0][20:24], bulk[1], bulk[2][20:24], bulk[3]
    bo = Bodies(torch, bodies)
    d_out = torch.full((4 * 8192 + 64,), GUARD, dtype=torch.uint8).cuda()
    out_ptrs = i64(torch, [d_out.data_ptr() + i * 8192 for i in range(4)])
    out_caps = i64(torch, [8192] * 4)
    out_bytes = torch.full((4,), -1, dtype=torch.int64).cuda()
    status = torch.full((4,), -1, dtype=torch.int32).cuda()
    a = [ctx.h, bo.ptrs.data_ptr(), bo.bytes.data_ptr(), d_code.data_ptr(), 4, out_ptrs.data_ptr(), out_caps.data_ptr(),
         out_bytes.data_ptr(), status.data_ptr()]

    def call(**kw):
        b = list(a)
        for k, v in kw.items():
            b[int(k[1:])] = v
        return L.ghf_decode_bodies_batch_shared(*b)

    assert call(_4=0) == OK  # count == 0 queues nothing
    assert call(_1=None) == E_INVAL and call(_2=None) == E_INVAL and call(_7=None) == E_INVAL and call(_8=None) == E_INVAL
    assert call(_6=None) == E_INVAL  # output pointers without caps
    assert call(_3=None) == E_INVAL and call(_3=d_code.data_ptr() + 8) == E_INVAL  # a null or misaligned d_code
    assert call(_3=None, _4=0) == E_INVAL  # the argument checks come before the count
    assert L.ghf_decode_bodies_batch_shared(None, *a[1:]) == E_INVAL
    ctx.sync()
    assert np.all(status.cpu().numpy() == -1) and np.all(out_bytes.cpu().numpy() == -1) and np.all(d_out.cpu().numpy() == GUARD)
    assert call() == OK  # the context is usable afterwards
    ctx.sync()
    assert status.cpu().tolist() == [OK] * 4 and out_bytes.cpu().tolist() == [d.size for d in datas]
    h = d_out.cpu().numpy()
    for i, d in enumerate(datas):
        assert np.array_equal(h[i * 8192 :][: d.size], d), i
        assert np.all(h[i * 8192 + d.size : (i + 1) * 8192] == GUARD), i


def test_python_wrapper_sizes_pass_then_decode_pass(env, bulk):
    ghf, ctx, torch = env
    datas, code, bodies, d_code = bulk[0][30:46], bulk[1], bulk[2][30:46], bulk[3]
    bo = Bodies(torch, bodies)
    sizes = ctx.decode_bodies_batch_shared(bo.ptrs, bo.bytes, d_code)
    assert set(sizes) == {"out_bytes", "status"}
    dec = ctx.decode_bodies_batch_shared(bo.ptrs, bo.bytes, d_code, out=True, caps=sizes["out_bytes"])
    ctx.sync()
    assert sizes["status"].cpu().tolist() == [OK] * 16 and sizes["out_bytes"].cpu().tolist() == [d.size for d in datas]
    assert dec["status"].cpu().tolist() == [OK] * 16 and dec["out_bytes"].cpu().tolist() == [d.size for d in datas]
    ho = dec["out"].cpu().numpy()
    for i, d in enumerate(datas):
        assert np.array_equal(ho[i * dec["out_stride"] :][: d.size], d), i
    with pytest.raises(ValueError):
        ctx.decode_bodies_batch_shared(bo.ptrs, bo.bytes, d_code, out=True)


def test_pass_counters(env, bulk):
    """the words of ghf_decode_images_batch_stats receive this call's rounds and passes: at least one round per item that
    reached its body, and a round never takes more passes than it has subsequences"""
    ghf, ctx, torch = env
    datas, code, bodies, d_code = bulk[0][50:60], bulk[1], bulk[2][50:60], bulk[3]
    bo = Bodies(torch, [bodies[0], None] + bodies[1:], stream_bytes=[None, 100] + [None] * 9)  # the null pointer reaches no body
    stats = torch.zeros(2, dtype=torch.int64).cuda()
    ctx.decode_images_batch_stats(stats)
    try:
        status, nbytes, _, _ = run(env, bo, d_code)
    finally:
        ctx.decode_images_batch_stats(None)
    assert status.tolist() == [OK, E_INVAL] + [OK] * 9
    rounds, passes = stats.cpu().tolist()
    want_rounds = sum(-(-8 * b.size // ROUND_BITS) for b in bodies)
    print("10 items: rounds %d (bodies span %d) passes %d" % (rounds, want_rounds, passes))
    assert 10 <= rounds <= want_rounds
    assert rounds <= passes <= 256 * rounds
    run(env, bo, d_code)  # switched off: the words stay
    assert stats.cpu().tolist() == [rounds, passes]
