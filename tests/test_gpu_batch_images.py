"""GPU: ghf_decode_images_batch -- standalone .crs2 images decoded from nothing but their bytes, one launch per call.

Expected values come from the reference's recorded outputs (tests/golden/golden.json, golden_sweeps.json) and the CPU
oracle, never from the library under test: every image is either bytes the compiled reference wrote, or the oracle's
compression with its SHA-256 checked against the reference's record first.  ghf_compress_batch / ghf_decode_batch only
appear where the point is that their images and outputs agree with this path."""
import base64
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import datagen as dg
import pkgload
from cases import CASES, sweep_crs2_inputs
from header_cases import header_cases
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_CAP, E_FORMAT, E_CORRUPT = 0, 1, 5, 6, 7
GUARD = 0xA5
MAX_ITEM = 1 << 20
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


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


class Images:
    """images (host uint8 arrays) packed into one device buffer, every image at a 16-byte aligned address, GUARD between"""

    def __init__(self, torch, images, stream_bytes=None, shift=None):
        self.torch, self.count = torch, len(images)
        self.offs, at = [], 0
        for k, im in enumerate(images):
            self.offs.append(at + (shift[k] if shift else 0))
            at += (im.size + 15 & ~15) + 64
        packed = np.full(at + 64, GUARD, dtype=np.uint8)
        for o, im in zip(self.offs, images):
            packed[o : o + im.size] = im
        self.d = torch.from_numpy(packed).cuda()
        assert self.d.data_ptr() % 16 == 0
        self.ptrs = i64(torch, [self.d.data_ptr() + o for o in self.offs])
        self.sizes = [int(im.size) for im in images] if stream_bytes is None else [int(v) for v in stream_bytes]
        self.bytes = i64(torch, self.sizes)


def run(env, im, caps=None, want_codes=False, null_out=()):
    """one ghf_decode_images_batch call; caps=None: sizes only.  Every output sits at an address misaligned by 1..15
    between GUARD bytes.  -> (status, out_bytes, outputs cut to their caps, guards (front, behind the cap), codes)"""
    ghf, ctx, torch = env
    n = im.count
    out_bytes = torch.full((n,), -1, dtype=torch.int64).cuda()
    status = torch.full((n,), -1, dtype=torch.int32).cuda()
    codes = torch.zeros((n, C.sizeof(ghf.Code)), dtype=torch.uint8).cuda() if want_codes else None
    if caps is None:
        rc = ghf.lib().ghf_decode_images_batch(ctx.h, im.ptrs.data_ptr(), im.bytes.data_ptr(), n, None, None, out_bytes.data_ptr(),
                                               None if codes is None else codes.data_ptr(), status.data_ptr())
        assert rc == 0, rc
        ctx.sync()  # raises if the context's status word was latched: per-item failures must not do that
        return status.cpu().numpy(), out_bytes.cpu().numpy(), None, None, None if codes is None else codes.cpu().numpy()
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
    rc = ghf.lib().ghf_decode_images_batch(ctx.h, im.ptrs.data_ptr(), im.bytes.data_ptr(), n, out_ptrs.data_ptr(), out_caps.data_ptr(),
                                           out_bytes.data_ptr(), None if codes is None else codes.data_ptr(), status.data_ptr())
    assert rc == 0, rc
    ctx.sync()
    h = d_out.cpu().numpy()
    ends = [s[0] for s in slots[1:]] + [h.size]
    outs = [h[s[1] : s[2]] for s in slots]
    guards = [(h[s[0] : s[1]], h[s[2] : e]) for s, e in zip(slots, ends)]
    return status.cpu().numpy(), out_bytes.cpu().numpy(), outs, guards, None if codes is None else codes.cpu().numpy()


def check_round_trip(env, images, datas, labels, stream_bytes=None):
    """sizes-only call -> the input sizes; decode call into exactly those caps -> the inputs, guards intact"""
    im = Images(env[2], images, stream_bytes=stream_bytes)
    status, nbytes, _, _, _ = run(env, im)
    for i, d in enumerate(datas):
        print("sizes  %-28s status %d bytes %d (want %d)" % (labels[i], status[i], nbytes[i], d.size))
    assert status.tolist() == [OK] * len(datas)
    assert nbytes.tolist() == [d.size for d in datas]
    status, nbytes, outs, guards, _ = run(env, im, caps=[d.size for d in datas])
    for i, d in enumerate(datas):
        print("decode %-28s status %d bytes %d (want %d)" % (labels[i], status[i], nbytes[i], d.size))
    assert status.tolist() == [OK] * len(datas)
    for i, d in enumerate(datas):
        assert int(nbytes[i]) == d.size, labels[i]
        assert np.array_equal(outs[i], d), labels[i]
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), labels[i]


def small_items(count, seed):
    """the recipe of tests/test_gpu_batch.py: `count` seeded items of 1..8192 bytes, mixed kinds; every seventh folded to
    a few values (ties, tiny alphabets)"""
    out = []
    for i in range(count):
        n = int(dg.splitmix64(np.uint64(seed + i)) % np.uint64(8192)) + 1
        kind = ["uniform", "zipf", "sym16", "text"][i % 4]
        d = dg.make(kind, n, seed=seed + 7 * i)
        if i % 7 == 0:
            d = d % np.uint8(1 + i % 5)
        out.append(d)
    return out


# ------------------------------------------------------------------------------ 1. files the reference wrote
def test_reference_written_files(env, golden):
    ghf, ctx, torch = env
    names = [k for k in golden if "crs2_b64" in golden[k]]
    assert len(names) == 8
    images = [np.frombuffer(base64.b64decode(golden[k]["crs2_b64"]), dtype=np.uint8) for k in names]
    for k, img in zip(names, images):
        assert img.size == golden[k]["crs2_bytes"] and sha(img) == golden[k]["crs2_sha256"], k
    im = Images(torch, images)
    status, nbytes, outs, guards, codes = run(env, im, caps=[golden[k]["n"] for k in names], want_codes=True)
    assert status.tolist() == [OK] * 8
    for i, k in enumerate(names):
        g = golden[k]
        assert int(nbytes[i]) == g["n"], k
        assert sha(outs[i]) == g["decoded_sha256"], k
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), k
        d = ghf.Code.from_buffer_copy(codes[i].tobytes()).as_dict()
        for f in ("length", "codeword", "symbol", "first_code", "start_pos", "min_len", "max_len"):
            assert d[f] == g[f], (k, f)
        # and byte for byte what the host parser returns for the same header, unused tails included
        want, _ = ghf.parse_header(images[i])
        assert codes[i].tobytes() == bytes(want), k


# ------------------------------------------------------------------------------ 2. every golden case of at most 1 MiB
def test_every_golden_case_up_to_1_mib(env, golden):
    names = [k for k in CASES if CASES[k]().size <= MAX_ITEM]
    assert sorted(set(CASES) - set(names)) == ["fib30", "fib32_maxlen32"]
    assert len(names) == 44
    datas = [CASES[k]() for k in names]
    images = [orc.compress(d) for d in datas]
    for k, d, img in zip(names, datas, images):
        assert sha(d) == golden[k]["input_sha256"], k
        assert sha(img) == golden[k]["crs2_sha256"], k  # the image is the reference's file
    check_round_trip(env, images, datas, names)


# ------------------------------------------------------------------------------ 3. the reference's recorded sweeps
def test_the_recorded_sweeps(env):
    with open(os.path.join(ROOT, "tests", "golden", "golden_sweeps.json")) as f:
        ref = json.load(f)["crs2"]
    inputs = sweep_crs2_inputs()
    assert len(inputs) == len(ref) == 40
    images = []
    for (label, data), r in zip(inputs, ref):
        assert label == r["label"] and sha(data) == r["input_sha256"]
        img = orc.compress(data)
        assert img.size == r["ref_bytes"] and sha(img) == r["ref_sha256"], label
        images.append(img)
    check_round_trip(env, images, [d for _, d in inputs], [l for l, _ in inputs])


# ------------------------------------------------------------------------------ 4. + 5. many small items
@pytest.fixture(scope="module")
def small(env):
    """1024 seeded items compressed by ghf_compress_batch (images checked against the oracle), side-car kept alive"""
    ghf, ctx, torch = env
    datas = small_items(1024, seed=9000)
    tensors = [torch.from_numpy(d).cuda() for d in datas]
    bidx = ctx.batch_index_alloc(len(datas), 8192)
    r = ctx.compress_batch(tensors, max_item_bytes=8192, index=bidx)
    ctx.sync()
    assert r["status"].cpu().tolist() == [OK] * 1024
    h, nb = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
    images = [h[i * r["out_stride"] :][: int(nb[i])].copy() for i in range(1024)]
    for i in (0, 1, 7, 500, 1023):
        assert np.array_equal(images[i], orc.compress(datas[i])), i
    yield datas, images, r, bidx
    ctx.batch_index_free(bidx)


def test_1024_small_items_from_the_images_alone(env, small):
    ghf, ctx, torch = env
    datas, images, r, bidx = small
    # from the very buffers ghf_compress_batch wrote: only pointers and sizes are handed over
    caps = i64(torch, [d.size for d in datas])
    sizes = ctx.decode_images_batch(r["out_ptrs"], r["out_bytes"])
    dec = ctx.decode_images_batch(r["out_ptrs"], r["out_bytes"], out=True, caps=caps)
    with_car = ctx.decode_batch(r["out_ptrs"], r["out_bytes"], r["codes"], bidx, r["in_bytes"])
    ctx.sync()  # stays OK
    assert sizes["status"].cpu().tolist() == [OK] * 1024
    assert sizes["out_bytes"].cpu().tolist() == [d.size for d in datas]
    assert dec["status"].cpu().tolist() == [OK] * 1024
    assert dec["out_bytes"].cpu().tolist() == [d.size for d in datas]
    assert with_car["status"].cpu().tolist() == [OK] * 1024
    ho, hc = dec["out"].cpu().numpy(), with_car["out"].cpu().numpy()
    for i, d in enumerate(datas):
        got = ho[i * dec["out_stride"] :][: d.size]
        assert np.array_equal(got, d), i
        assert np.array_equal(hc[i * with_car["out_stride"] :][: d.size], got), i
    # and from copies of the images between guards, outputs misaligned
    check_round_trip(env, images[:128], datas[:128], ["item %d" % i for i in range(128)])


def test_bytes_behind_the_stream_change_nothing(env, small):
    datas, images = small[0][:256], small[1][:256]
    rng = np.random.default_rng(11)
    longer = [np.concatenate([im, rng.integers(0, 256, size=1 + i % 40, dtype=np.uint8)]) for i, im in enumerate(images)]
    check_round_trip(env, longer, datas, ["item %d + %d" % (i, 1 + i % 40) for i in range(256)])


# ------------------------------------------------------------------------------ 6. per-item failures
def test_failures_are_per_item(env, golden):
    ghf, ctx, torch = env
    good = small_items(6, seed=4100)
    z = CASES["zipf_64k"]()
    zimg = orc.compress(z)
    assert sha(zimg) == golden["zipf_64k"]["crs2_sha256"]
    hdr_bytes = golden["zipf_64k"]["header_bytes"]
    assert zimg[:hdr_bytes].tobytes() == base64.b64decode(golden["zipf_64k"]["header_b64"])
    bad_headers = []
    for pos, val in ((3, 0), (1035, 99), (1039, 40), (8, 7), (1047, 5)):  # test_parse_header_rejects_garbage
        b = zimg.copy()
        b[pos] = val
        with pytest.raises(ghf.GhfError):
            ghf.parse_header(b[:hdr_bytes])
        with pytest.raises(ghf.GhfError):
            ghf.parse_header(b)
        bad_headers.append(b)
    with pytest.raises(ghf.GhfError):
        ghf.parse_header(zimg[:500])
    t = dg.make("text", 7000, seed=92)
    timg = orc.compress(t)
    cut = (orc.build_code(orc.histogram(t)).as_dict()["max_len"] + 7) // 8 + 1
    u = dg.make("uniform", 3000, seed=77)
    uimg = orc.compress(u)
    gimg = [orc.compress(d) for d in good]
    #          image             stream_bytes        data     cap          shift  want
    items = [(gimg[0],           None,               good[0], None,        0,     OK),
             (bad_headers[0],    None,               z,       None,        0,     E_FORMAT),
             (bad_headers[1],    None,               z,       None,        0,     E_FORMAT),
             (gimg[1],           None,               good[1], None,        0,     OK),
             (bad_headers[2],    None,               z,       None,        0,     E_FORMAT),
             (bad_headers[3],    None,               z,       None,        0,     E_FORMAT),
             (bad_headers[4],    None,               z,       None,        0,     E_FORMAT),
             (zimg[:500],        None,               z,       None,        0,     E_FORMAT),
             (gimg[2],           None,               good[2], None,        0,     OK),
             (timg[:-cut],       None,               t,       None,        0,     E_CORRUPT),
             (gimg[3],           None,               good[3], None,        0,     OK),
             (uimg,              None,               u,       u.size - 1,  0,     E_CAP),
             (gimg[4],           None,               good[4], None,        0,     OK),
             (zimg,              None,               z,       None,        8,     E_INVAL),
             (uimg,              ghf.compress_bound(MAX_ITEM) + 1, u, None, 0,    E_INVAL),
             (gimg[5],           None,               good[5], None,        0,     OK),
             (zimg,              None,               z,       None,        0,     OK)]
    images = [it[0] for it in items]
    sb = [it[0].size if it[1] is None else it[1] for it in items]
    caps = [it[2].size if it[3] is None else it[3] for it in items]
    want = [it[5] for it in items]
    im = Images(torch, images, stream_bytes=sb, shift=[it[4] for it in items])
    status, nbytes, outs, guards, _ = run(env, im, caps=caps)  # run() ends with ctx.sync(): it stays OK
    print("status", status.tolist(), "want", want, "bytes", nbytes.tolist())
    assert status.tolist() == want
    for i, it in enumerate(items):
        if want[i] == OK:
            assert int(nbytes[i]) == it[2].size and np.array_equal(outs[i], it[2]), i
        else:
            assert int(nbytes[i]) == 0, i
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i  # nothing at or beyond the cap
    for i in (1, 2, 4, 5, 6, 7, 13, 14):  # refused before anything was written
        assert np.all(outs[i] == GUARD), i
    # sizes only: the cap plays no part, the true count comes back
    status, nbytes, _, _, _ = run(env, im)
    want0 = [OK if w == E_CAP else w for w in want]
    assert status.tolist() == want0
    assert nbytes.tolist() == [it[2].size if w == OK else 0 for it, w in zip(items, want0)]
    # a null output pointer in decode mode is the item's own failure
    status, nbytes, outs, guards, _ = run(env, Images(torch, gimg[:3]), caps=[d.size for d in good[:3]], null_out=(1,))
    assert status.tolist() == [OK, E_INVAL, OK] and int(nbytes[1]) == 0
    assert np.array_equal(outs[0], good[0]) and np.array_equal(outs[2], good[2]) and np.all(outs[1] == GUARD)


# ------------------------------------------------------------------------------ 6b. host and device state the same rules
def test_header_rules_agree_with_the_host_parser(env):
    """every corrupted header of tests/header_cases.py (one broken rule each), good items between them, in one launch:
    GHF_E_FORMAT exactly where ghf_parse_header refuses, with outputs and sizes-only"""
    ghf, ctx, torch = env
    data, img, empty, cases = header_cases()
    images, datas, labels = [img], [data], ["good"]
    for name, bad in cases:
        images += [bad, img]
        datas += [data, data]
        labels += [name, "good"]
    images.append(empty)
    datas.append(data[:0])
    labels.append("empty")
    want = []
    for im_ in images:
        try:
            ghf.parse_header(im_)
            want.append(OK)
        except ghf.GhfError as e:
            assert e.status == E_FORMAT
            want.append(E_FORMAT)
    assert want == [OK] + [E_FORMAT, OK] * len(cases) + [OK]  # tests/test_header_rules_cpu.py, case by case
    im = Images(torch, images)
    status, nbytes, outs, guards, _ = run(env, im, caps=[4096] * len(images))
    for i, l in enumerate(labels):
        print("decode %-40s status %d bytes %d (want %d)" % (l, status[i], nbytes[i], want[i]))
    assert status.tolist() == want
    for i, l in enumerate(labels):
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), l
        if want[i] != OK:
            assert int(nbytes[i]) == 0 and np.all(outs[i] == GUARD), l  # refused before anything was written
        elif l == "empty":
            assert int(nbytes[i]) == 0 and np.all(outs[i] == GUARD), l
        else:
            assert int(nbytes[i]) == data.size and np.array_equal(outs[i], data), l
    status, nbytes, _, _, _ = run(env, im)
    assert status.tolist() == want
    assert nbytes.tolist() == [d.size if w == OK else 0 for d, w in zip(datas, want)]


# ------------------------------------------------------------------------------ 7. the empty image
def test_empty_image(env):
    ghf, ctx, torch = env
    e = orc.compress_empty()
    assert e.size == 1049
    d = dg.make("zipf", 3000, seed=5)
    im = Images(torch, [orc.compress(d), e, e])
    status, nbytes, outs, guards, codes = run(env, im, caps=[d.size, 0, 64], want_codes=True)
    assert status.tolist() == [OK, OK, OK] and nbytes.tolist() == [d.size, 0, 0]
    assert np.array_equal(outs[0], d) and np.all(outs[2] == GUARD)  # nothing written
    for g in guards:
        assert np.all(g[0] == GUARD) and np.all(g[1] == GUARD)
    want, hs = ghf.parse_header(e)
    assert hs == 1048 and codes[1].tobytes() == bytes(want) == codes[2].tobytes()
    status, nbytes, _, _, _ = run(env, im)
    assert status.tolist() == [OK, OK, OK] and nbytes.tolist() == [d.size, 0, 0]


# ------------------------------------------------------------------------------ 8. call level
def test_call_level(env):
    ghf, ctx, torch = env
    L = ghf.lib()
    datas = small_items(4, seed=6300)
    im = Images(torch, [orc.compress(d) for d in datas])
    d_out = torch.full((4 * 8192 + 64,), GUARD, dtype=torch.uint8).cuda()
    out_ptrs = i64(torch, [d_out.data_ptr() + i * 8192 for i in range(4)])
    out_caps = i64(torch, [8192] * 4)
    out_bytes = torch.full((4,), -1, dtype=torch.int64).cuda()
    status = torch.full((4,), -1, dtype=torch.int32).cuda()
    a = [ctx.h, im.ptrs.data_ptr(), im.bytes.data_ptr(), 4, out_ptrs.data_ptr(), out_caps.data_ptr(), out_bytes.data_ptr(), None,
         status.data_ptr()]

    def call(**kw):
        b = list(a)
        for k, v in kw.items():
            b[int(k[1:])] = v
        return L.ghf_decode_images_batch(*b)

    assert call(_3=0) == OK  # count == 0 queues nothing
    assert call(_1=None) == E_INVAL and call(_2=None) == E_INVAL and call(_6=None) == E_INVAL and call(_8=None) == E_INVAL
    assert call(_5=None) == E_INVAL  # output pointers without caps
    assert L.ghf_decode_images_batch(None, *a[1:]) == E_INVAL
    ctx.sync()
    assert np.all(status.cpu().numpy() == -1) and np.all(out_bytes.cpu().numpy() == -1) and np.all(d_out.cpu().numpy() == GUARD)
    assert call() == OK  # the context is usable afterwards
    ctx.sync()
    assert status.cpu().tolist() == [OK] * 4 and out_bytes.cpu().tolist() == [d.size for d in datas]
    h = d_out.cpu().numpy()
    for i, d in enumerate(datas):
        assert np.array_equal(h[i * 8192 :][: d.size], d), i
        assert np.all(h[i * 8192 + d.size : (i + 1) * 8192] == GUARD), i


def test_python_wrapper_sizes_pass_then_decode_pass(env):
    ghf, ctx, torch = env
    datas = small_items(16, seed=7400)
    im = Images(torch, [orc.compress(d) for d in datas])
    sizes = ctx.decode_images_batch(im.ptrs, im.bytes)
    assert set(sizes) == {"out_bytes", "status"}
    dec = ctx.decode_images_batch(im.ptrs, im.bytes, out=True, caps=sizes["out_bytes"], codes=True)
    ctx.sync()
    assert sizes["status"].cpu().tolist() == [OK] * 16 and sizes["out_bytes"].cpu().tolist() == [d.size for d in datas]
    assert dec["status"].cpu().tolist() == [OK] * 16 and dec["out_bytes"].cpu().tolist() == [d.size for d in datas]
    ho, hc = dec["out"].cpu().numpy(), dec["codes"].cpu().numpy()
    for i, d in enumerate(datas):
        assert np.array_equal(ho[i * dec["out_stride"] :][: d.size], d), i
        assert hc[i].tobytes() == bytes(ghf.parse_header(orc.compress(d))[0]), i


def test_pass_counters(env):
    """ghf_decode_images_batch_stats: rounds and passes are counted, and a round never takes more passes than it has
    subsequences"""
    ghf, ctx, torch = env
    d = dg.make("uniform", 65536, seed=3)
    im = Images(torch, [orc.compress(d)] * 4)
    stats = torch.zeros(2, dtype=torch.int64).cuda()
    ctx.decode_images_batch_stats(stats)
    try:
        r = ctx.decode_images_batch(im.ptrs, im.bytes)
        ctx.sync()
    finally:
        ctx.decode_images_batch_stats(None)
    assert r["status"].cpu().tolist() == [OK] * 4 and r["out_bytes"].cpu().tolist() == [d.size] * 4
    rounds, passes = stats.cpu().tolist()
    body_bits = 8 * (im.sizes[0] - ghf.parse_header(orc.compress(d))[1])
    print("uniform 64 KiB: rounds %d passes %d per item" % (rounds // 4, passes // 4))
    assert rounds % 4 == 0 and 1 <= rounds // 4 <= -(-body_bits // (256 * 512))  # the end mark sits in the last round
    assert rounds <= passes <= 256 * rounds
    r = ctx.decode_images_batch(im.ptrs, im.bytes)  # switched off: the words stay
    ctx.sync()
    assert stats.cpu().tolist() == [rounds, passes]
