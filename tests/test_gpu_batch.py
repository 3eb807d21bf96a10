"""GPU: ghf_compress_batch / ghf_decode_batch -- many small independent .crs2 streams in one launch.

Expected values come from the reference's recorded outputs (tests/golden/golden.json, golden_sweeps.json) and the CPU
oracle; the single-stream path (ghf_compress / ghf_decode) is only used as a cross-check that both paths agree byte for
byte, side-car included."""
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
from header_cases import bad_codes, header_cases, vet_branch_codes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_CORRUPT = 0, 1, 3, 5, 6, 7
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


class Batch:
    """one ghf_compress_batch call over `datas` with everything the checks need kept on the host side"""

    def __init__(self, ghf, ctx, torch, datas, odd=False, caps=None, max_item=None, with_index=True):
        self.ghf, self.ctx, self.torch, self.datas = ghf, ctx, torch, datas
        self.count = len(datas)
        self.sizes = [int(d.size) for d in datas]
        self.max_item = max(self.sizes) if max_item is None else max_item
        # packed input; odd: every item starts at an odd address (the tensor's base is at least 256-byte aligned)
        offs, at = [], 0
        for n in self.sizes:
            if odd:
                at |= 1
            offs.append(at)
            at += n + (3 if odd else 0)
        packed = np.full(at + 16, 0x5A, dtype=np.uint8)
        for o, d in zip(offs, datas):
            packed[o : o + d.size] = d
        self.d_in = torch.from_numpy(packed).cuda()
        assert self.d_in.data_ptr() % 16 == 0
        self.in_ptrs = i64(torch, [self.d_in.data_ptr() + o for o in offs])
        self.in_bytes = i64(torch, self.sizes)
        bound = ghf.compress_batch_bound(min(self.max_item, MAX_ITEM))
        self.caps = [bound] * self.count if caps is None else list(caps)
        self.stride = (max(self.caps) + 15 & ~15) + 64
        self.d_out = torch.full((self.count * self.stride + 16,), GUARD, dtype=torch.uint8).cuda()
        self.out_ptrs = i64(torch, [self.d_out.data_ptr() + i * self.stride for i in range(self.count)])
        self.out_caps = i64(torch, self.caps)
        self.out_bytes = torch.full((self.count,), -1, dtype=torch.int64).cuda()
        self.status = torch.full((self.count,), -1, dtype=torch.int32).cuda()
        self.codes = torch.zeros((self.count, C.sizeof(ghf.Code)), dtype=torch.uint8).cuda()
        self.bidx = ctx.batch_index_alloc(self.count, min(self.max_item, MAX_ITEM)) if with_index else None

    def run(self):
        rc = self.ghf.lib().ghf_compress_batch(
            self.ctx.h, self.in_ptrs.data_ptr(), self.in_bytes.data_ptr(), self.max_item, self.count, self.out_ptrs.data_ptr(),
            self.out_caps.data_ptr(), self.out_bytes.data_ptr(), self.codes.data_ptr(),
            None if self.bidx is None else C.byref(self.bidx), self.status.data_ptr())
        assert rc == 0, rc
        self.ctx.sync()  # raises if the context's status word was latched: per-item failures must not do that
        self.h_out = self.d_out.cpu().numpy()
        self.h_bytes = self.out_bytes.cpu().numpy()
        self.h_status = self.status.cpu().numpy()
        self.h_codes = self.codes.cpu().numpy()
        return self

    def image(self, i):
        return self.h_out[i * self.stride : i * self.stride + int(self.h_bytes[i])]

    def slot(self, i):
        return self.h_out[i * self.stride : (i + 1) * self.stride]

    def code(self, i):
        return self.ghf.Code.from_buffer_copy(self.h_codes[i].tobytes())

    def free(self):
        if self.bidx is not None:
            self.ctx.batch_index_free(self.bidx)
            self.bidx = None


def decode_batch(b, n_symbols=None, stream_bytes=None, codes=None, d_stream=None, caps=None):
    """ghf_decode_batch on the outputs of Batch `b`: every output at an unaligned address between guard bytes.
    -> (status, out_bytes, list of decoded arrays, list of (front guard, back guard) arrays)"""
    ghf, ctx, torch = b.ghf, b.ctx, b.torch
    n_symbols = b.sizes if n_symbols is None else n_symbols
    ostride = (b.max_item + 15 & ~15) + 64
    d_out = torch.full((b.count * ostride + 64,), GUARD, dtype=torch.uint8).cuda()
    ooff = [i * ostride + 17 + (i % 15) for i in range(b.count)]  # misalignments 1..15 (+ 17)
    out_ptrs = i64(torch, [d_out.data_ptr() + o for o in ooff])
    out_caps = i64(torch, [b.max_item] * b.count if caps is None else caps)
    out_bytes = torch.full((b.count,), -1, dtype=torch.int64).cuda()
    status = torch.full((b.count,), -1, dtype=torch.int32).cuda()
    sp = b.out_ptrs if d_stream is None else i64(torch, [d_stream.data_ptr() + i * b.stride for i in range(b.count)])
    sb = b.out_bytes if stream_bytes is None else i64(torch, stream_bytes)
    cd = b.codes if codes is None else codes
    rc = ghf.lib().ghf_decode_batch(ctx.h, sp.data_ptr(), sb.data_ptr(), cd.data_ptr(), C.byref(b.bidx),
                                    i64(torch, n_symbols).data_ptr(), b.count, out_ptrs.data_ptr(), out_caps.data_ptr(),
                                    out_bytes.data_ptr(), status.data_ptr())
    assert rc == 0, rc
    ctx.sync()
    h = d_out.cpu().numpy()
    outs, guards = [], []
    for i in range(b.count):
        n = int(n_symbols[i])
        outs.append(h[ooff[i] : ooff[i] + n])
        lo = i * ostride
        guards.append((h[lo : ooff[i]], h[ooff[i] + n : lo + ostride]))
    return status.cpu().numpy(), out_bytes.cpu().numpy(), outs, guards


def small_items(count, seed):
    """`count` seeded items of 1..8192 bytes, mixed kinds; every seventh folded to a few values (ties, tiny alphabets)"""
    out = []
    for i in range(count):
        n = int(dg.splitmix64(np.uint64(seed + i)) % np.uint64(8192)) + 1
        kind = ["uniform", "zipf", "sym16", "text"][i % 4]
        d = dg.make(kind, n, seed=seed + 7 * i)
        if i % 7 == 0:
            d = d % np.uint8(1 + i % 5)
        out.append(d)
    return out


# ------------------------------------------------------------------------------ 1. every golden case in one call
@pytest.fixture(scope="module")
def golden_batch(env):
    ghf, ctx, torch = env
    names = [k for k in CASES if CASES[k]().size <= MAX_ITEM]
    b = Batch(ghf, ctx, torch, [CASES[k]() for k in names]).run()
    yield names, b
    b.free()


def test_all_golden_cases_in_one_call(env, golden, golden_batch):
    names, b = golden_batch
    assert sorted(set(CASES) - set(names)) == ["fib30", "fib32_maxlen32"]
    assert len(names) == 44
    for i, name in enumerate(names):
        g = golden[name]
        assert sha(b.datas[i]) == g["input_sha256"], name
        assert b.h_status[i] == OK, name
        assert int(b.h_bytes[i]) == g["crs2_bytes"], name
        img = b.image(i)
        assert img[: g["header_bytes"]].tobytes() == base64.b64decode(g["header_b64"]), name
        assert sha(img) == g["crs2_sha256"], name
        d = b.code(i).as_dict()
        for k in ("length", "codeword", "symbol", "first_code", "start_pos", "min_len", "max_len"):
            assert d[k] == g[k], (name, k)
        assert np.all(b.slot(i)[b.caps[i] :] == GUARD), name  # nothing at or beyond the cap


# ------------------------------------------------------------------------------ 2. the reference's recorded sweeps
def test_reference_sweeps_from_odd_addresses(env):
    ghf, ctx, torch = env
    with open(os.path.join(ROOT, "tests", "golden", "golden_sweeps.json")) as f:
        ref = json.load(f)["crs2"]
    inputs = sweep_crs2_inputs()
    assert len(inputs) == len(ref) == 40
    b = Batch(ghf, ctx, torch, [d for _, d in inputs], odd=True).run()
    try:
        for i, ((label, data), r) in enumerate(zip(inputs, ref)):
            assert label == r["label"] and sha(data) == r["input_sha256"]
            assert b.h_status[i] == OK, label
            assert int(b.h_bytes[i]) == r["ref_bytes"], label
            assert sha(b.image(i)) == r["ref_sha256"], label
    finally:
        b.free()


# ------------------------------------------------------------------------------ 3. many small items
@pytest.fixture(scope="module")
def small_batch(env):
    ghf, ctx, torch = env
    b = Batch(ghf, ctx, torch, small_items(1024, seed=9000)).run()
    yield b
    b.free()


SAMPLE = [int(x) for x in np.random.default_rng(5).choice(1024, size=32, replace=False)]


def test_many_small_items_equal_the_oracle(env, small_batch):
    b = small_batch
    assert b.count == 1024 and min(b.sizes) >= 1 and max(b.sizes) <= 8192
    assert np.all(b.h_status == OK)
    for i, d in enumerate(b.datas):
        want = orc.compress(d)
        assert int(b.h_bytes[i]) == want.size, i
        assert np.array_equal(b.image(i), want), i


def test_sampled_items_equal_the_single_stream_path_with_side_car(env, small_batch):
    ghf, ctx, torch = env
    b = small_batch
    for i in SAMPLE:
        d = b.datas[i]
        d_in = torch.from_numpy(d).cuda()
        idx = ctx.index_alloc(d.size)
        d_out, nbytes, _ = ctx.compress(d_in, index=idx)
        ctx.sync()
        nb = int(nbytes.item())
        assert nb == int(b.h_bytes[i]), i
        assert np.array_equal(d_out[:nb].cpu().numpy(), b.image(i)), i
        want_chunk, want_seg = ctx.index_to_host(idx)
        view = ghf.batch_index_item(b.bidx, i, d.size)
        assert (view.n_chunks, view.n_segs) == (idx.n_chunks, idx.n_segs)
        got_chunk, got_seg = ctx.index_to_host(view)
        assert np.array_equal(got_chunk, want_chunk), i
        assert np.array_equal(got_seg, want_seg), i
        ctx.index_free(idx)


# ------------------------------------------------------------------------------ 4. round trip
def _check_round_trip(b, sample):
    ghf, ctx, torch = b.ghf, b.ctx, b.torch
    status, out_bytes, outs, guards = decode_batch(b)
    assert np.all(status == OK)
    for i, d in enumerate(b.datas):
        assert int(out_bytes[i]) == d.size, i
        assert np.array_equal(outs[i], d), i
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    for i in sample:  # the single-stream decoder reads the same image with the item's view of the side-car
        d = b.datas[i]
        view = ghf.batch_index_item(b.bidx, i, d.size)
        d_stream = b.d_out[i * b.stride : i * b.stride + int(b.h_bytes[i])]
        d_code = b.codes[i]
        back, nout = ctx.decode(d_stream, int(b.h_bytes[i]), d_code, view)
        ctx.sync()
        assert int(nout.item()) == d.size
        assert np.array_equal(back[: d.size].cpu().numpy(), d), i


def test_round_trip_of_the_golden_cases(env, golden_batch):
    names, b = golden_batch
    _check_round_trip(b, [names.index(k) for k in ("aaaabbc", "single_x", "uniform_64k", "uniform_1m", "zipf_64k")])


def test_round_trip_of_many_small_items(env, small_batch):
    _check_round_trip(small_batch, SAMPLE[:8])


def length_changing_flip(data):
    """A body bit of oracle.compress(data) whose flip makes a segment miss its end: decoding the segment's 64 symbols from
    the flipped bits (here, on the host, with the oracle's code) uses another number of bits than the original did.  (A
    flip that turns a code into another one of the same length cannot be seen by any decoder: the format has no checksum.)"""
    code = orc.build_code(orc.histogram(data)).as_dict()
    length, codeword = code["length"], code["codeword"]
    book = {(length[s], codeword[s]): s for s in range(257) if length[s]}
    hdr = 1040 + 8 * code["max_len"]
    bits = np.unpackbits(orc.compress(data))
    lens = np.asarray(length, dtype=np.int64)[data]
    starts = 8 * hdr + np.concatenate(([0], np.cumsum(lens)))
    seg = 20  # symbols [1280, 1344)
    a, e = int(starts[64 * seg]), int(starts[64 * seg + 64])
    for k in range(5, 40):
        cand = int(starts[64 * seg + k])  # the first bit of the k-th code of the segment
        work = bits.copy()
        work[cand] ^= 1
        at, ok = a, True
        for _ in range(64):
            v, l = 0, 0
            while (l, v) not in book and l < 33:
                v, l = (v << 1) | int(work[at + l]), l + 1
            if (l, v) not in book:
                ok = False
                break
            at += l
        if not ok or at != e:
            return cand
    raise AssertionError("no length-changing flip found")


# ------------------------------------------------------------------------------ 5. per-item failures
def test_compress_failures_are_per_item(env):
    ghf, ctx, torch = env
    good = small_items(6, seed=4100)
    short = dg.make("uniform", 3000, seed=77)
    big = dg.make("zipf", 5000, seed=78)
    datas = [good[0], np.zeros(0, dtype=np.uint8), good[1], short, good[2], big, good[3], good[4], good[5]]
    max_item = 4999  # `big` is one byte too long; everything else fits
    assert max(d.size for d in datas if d is not big) <= 8192
    datas = [d if d is big or d.size <= max_item else d[:max_item] for d in datas]
    bound = ghf.compress_batch_bound(max_item)
    caps = [bound] * len(datas)
    caps[3] = orc.compress(short).size - 1  # one byte short
    b = Batch(ghf, ctx, torch, datas, caps=caps, max_item=max_item).run()  # run() ends with ctx.sync(): it stays OK
    try:
        want = [OK, E_EMPTY, OK, E_CAP, OK, E_INVAL, OK, OK, OK]
        assert b.h_status.tolist() == want
        for i, d in enumerate(datas):
            if want[i] == OK:
                assert np.array_equal(b.image(i), orc.compress(d)), i
            else:
                assert int(b.h_bytes[i]) == 0, i
            assert np.all(b.slot(i)[caps[i] :] == GUARD), i
        assert np.all(b.slot(1) == GUARD) and np.all(b.slot(5) == GUARD)  # refused before anything was written
    finally:
        b.free()


def test_decode_failures_are_per_item(env):
    ghf, ctx, torch = env
    datas = small_items(8, seed=5200)
    datas[2] = dg.make("zipf", 6000, seed=91)
    datas[6] = dg.make("text", 7000, seed=92)
    b = Batch(ghf, ctx, torch, datas).run()
    try:
        assert np.all(b.h_status == OK)
        # corrupt copies, built in host memory from the known-good images
        h = b.h_out.copy()
        flip_bit = length_changing_flip(datas[2])
        h[2 * b.stride + flip_bit // 8] ^= 0x80 >> (flip_bit % 8)
        d_stream = torch.from_numpy(h).cuda()
        codes = b.h_codes.copy()
        c4 = ghf.Code.from_buffer_copy(codes[4].tobytes())
        present = [s for s in range(256) if c4.length[s]]
        c4.length[present[0]] += 1  # the Kraft sum is no longer 1
        codes[4] = np.frombuffer(bytes(c4), dtype=np.uint8)
        d_codes = torch.from_numpy(codes).cuda()
        stream_bytes = [int(x) for x in b.h_bytes]
        stream_bytes[6] -= 40  # the stream ends before its last segments do
        status, out_bytes, outs, guards = decode_batch(b, stream_bytes=stream_bytes, codes=d_codes, d_stream=d_stream)
        want = [OK, OK, E_CORRUPT, OK, E_FORMAT, OK, E_CORRUPT, OK]
        assert status.tolist() == want
        for i, d in enumerate(datas):
            if want[i] == OK:
                assert int(out_bytes[i]) == d.size and np.array_equal(outs[i], d), i
            else:
                assert int(out_bytes[i]) == 0, i
            assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    finally:
        b.free()


def test_decode_refuses_codes_that_are_not_complete(env):
    """the code rules of ghf_code_rules.h through k_decode_batch: the four corrupted tables of tests/header_cases.py
    (tests/test_gpu_parity.py puts the same four through k_build_decode_tables) and two good ones in one launch"""
    ghf, ctx, torch = env
    data = header_cases()[0]
    b = Batch(ghf, ctx, torch, [data] * 6).run()
    try:
        assert np.all(b.h_status == OK) and np.array_equal(b.image(0), header_cases()[1])
        bad = bad_codes(b.code(0), ghf.Code.from_buffer_copy)
        assert len(bad) == 4
        codes = b.h_codes.copy()
        for i, (name, c) in zip((0, 1, 3, 4), bad):
            codes[i] = np.frombuffer(bytes(c), dtype=np.uint8)
        status, out_bytes, outs, guards = decode_batch(b, codes=torch.from_numpy(codes).cuda())
        print("status", status.tolist(), [name for name, _ in bad])
        assert status.tolist() == [E_FORMAT, E_FORMAT, OK, E_FORMAT, E_FORMAT, OK]
        for i in range(6):
            if status[i] == OK:
                assert int(out_bytes[i]) == data.size and np.array_equal(outs[i], data), i
            else:
                assert int(out_bytes[i]) == 0 and np.all(outs[i] == GUARD), i
            assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), i
    finally:
        b.free()


@pytest.mark.parametrize("refusal", ["empty", "cap"])
def test_an_items_own_refusal_comes_before_its_codes(env, refusal):
    """the order of k_decode_batch's verdicts: GHF_E_EMPTY / GHF_E_CAP of an item are reported although its code is
    broken as well (by its length bounds, by its Kraft sum: the two ways batch_code_ok refuses), never GHF_E_FORMAT.
    Three items of 65 bytes: one whole segment and a ragged one"""
    ghf, ctx, torch = env
    datas = [dg.make("zipf", 65, seed=6100 + i) for i in range(3)]
    b = Batch(ghf, ctx, torch, datas).run()
    try:
        assert np.all(b.h_status == OK)
        n_symbols, caps = [65, 65, 65], [b.max_item] * 3
        if refusal == "empty":
            n_symbols[1] = 0
        else:
            caps[1] = 64
        want = [OK, E_EMPTY if refusal == "empty" else E_CAP, OK]
        for name, c in vet_branch_codes(b.code(1), ghf.Code.from_buffer_copy):
            codes = b.h_codes.copy()
            codes[1] = np.frombuffer(bytes(c), dtype=np.uint8)
            d_codes = torch.from_numpy(codes).cuda()
            status, out_bytes, outs, guards = decode_batch(b, codes=d_codes)  # the code alone: it is refused
            assert status.tolist() == [OK, E_FORMAT, OK], name
            status, out_bytes, outs, guards = decode_batch(b, n_symbols=n_symbols, codes=d_codes, caps=caps)
            print(name, status.tolist(), out_bytes.tolist())
            assert status.tolist() == want, name
            assert out_bytes.tolist() == [65, 0, 65], name
            for i in (0, 2):
                assert np.array_equal(outs[i], datas[i]), (name, i)
            assert np.all(outs[1] == GUARD), name  # nothing of the refused item is written
            for i in range(3):
                assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (name, i)
    finally:
        b.free()


# ------------------------------------------------------------------------------ 6. call-level argument errors
def test_call_level_argument_errors(env):
    ghf, ctx, torch = env
    L = ghf.lib()
    datas = small_items(4, seed=6300)
    b = Batch(ghf, ctx, torch, datas)
    try:
        args = lambda max_item, count, bidx: (ctx.h, b.in_ptrs.data_ptr(), b.in_bytes.data_ptr(), max_item, count,
                                              b.out_ptrs.data_ptr(), b.out_caps.data_ptr(), b.out_bytes.data_ptr(),
                                              b.codes.data_ptr(), bidx, b.status.data_ptr())
        assert L.ghf_compress_batch(*args(b.max_item, 0, C.byref(b.bidx))) == OK  # count == 0: nothing is launched
        ctx.sync()
        assert np.all(b.status.cpu().numpy() == -1) and np.all(b.d_out.cpu().numpy() == GUARD)
        assert L.ghf_compress_batch(*args(MAX_ITEM + 1, 4, None)) == E_INVAL
        assert L.ghf_compress_batch(*args(0, 4, None)) == E_INVAL
        small = ctx.batch_index_alloc(2, b.max_item)  # too few items
        assert L.ghf_compress_batch(*args(b.max_item, 4, C.byref(small))) == E_INVAL
        ctx.batch_index_free(small)
        narrow = ctx.batch_index_alloc(4, b.max_item - 1)  # items too small
        assert L.ghf_compress_batch(*args(b.max_item, 4, C.byref(narrow))) == E_INVAL
        ctx.batch_index_free(narrow)
        bent = ghf.BatchIndex.from_buffer_copy(bytes(b.bidx))
        bent.segs_per_item += 1  # strides that are not the ones the geometry implies
        assert L.ghf_compress_batch(*args(b.max_item, 4, C.byref(bent))) == E_INVAL
        assert L.ghf_compress_batch(ctx.h, None, b.in_bytes.data_ptr(), b.max_item, 4, b.out_ptrs.data_ptr(), b.out_caps.data_ptr(),
                                    b.out_bytes.data_ptr(), None, None, b.status.data_ptr()) == E_INVAL
        assert L.ghf_decode_batch(ctx.h, b.out_ptrs.data_ptr(), b.out_bytes.data_ptr(), b.codes.data_ptr(), None,
                                  b.in_bytes.data_ptr(), 4, b.out_ptrs.data_ptr(), b.out_caps.data_ptr(), b.out_bytes.data_ptr(),
                                  b.status.data_ptr()) == E_INVAL
        assert L.ghf_decode_batch(ctx.h, b.out_ptrs.data_ptr(), b.out_bytes.data_ptr(), b.codes.data_ptr(), C.byref(bent),
                                  b.in_bytes.data_ptr(), 4, b.out_ptrs.data_ptr(), b.out_caps.data_ptr(), b.out_bytes.data_ptr(),
                                  b.status.data_ptr()) == E_INVAL
        ctx.sync()
        assert np.all(b.d_out.cpu().numpy() == GUARD)  # none of the refused calls queued anything
        b.run()  # and the context is still usable: d_codes == NULL is covered by the python wrapper below
        assert np.all(b.h_status == OK)
    finally:
        b.free()


def test_python_wrapper_round_trip_without_caller_codes_buffer(env):
    """Context.compress_batch / decode_batch on a list of tensors and on a packed tensor + sizes"""
    ghf, ctx, torch = env
    datas = small_items(16, seed=7400)
    tensors = [torch.from_numpy(d).cuda() for d in datas]
    bidx = ctx.batch_index_alloc(len(datas), 8192)
    try:
        r = ctx.compress_batch(tensors, max_item_bytes=8192, index=bidx)
        packed = torch.from_numpy(np.concatenate(datas)).cuda()
        r2 = ctx.compress_batch(packed, sizes=[d.size for d in datas], max_item_bytes=8192)
        ctx.sync()
        assert r["status"].cpu().tolist() == [OK] * 16 == r2["status"].cpu().tolist()
        h, nb = r["out"].cpu().numpy(), r["out_bytes"].cpu().numpy()
        h2 = r2["out"].cpu().numpy()
        for i, d in enumerate(datas):
            want = orc.compress(d)
            assert np.array_equal(h[i * r["out_stride"] :][: nb[i]], want), i
            assert np.array_equal(h2[i * r2["out_stride"] :][: want.size], want), i
        dec = ctx.decode_batch(r["out_ptrs"], r["out_bytes"], r["codes"], bidx, r["in_bytes"])
        ctx.sync()
        assert dec["status"].cpu().tolist() == [OK] * 16
        ho = dec["out"].cpu().numpy()
        for i, d in enumerate(datas):
            assert np.array_equal(ho[i * dec["out_stride"] :][: d.size], d), i
        # d_codes == NULL: the context lends its own table buffer
        r3_status = torch.full((16,), -1, dtype=torch.int32).cuda()
        rc = ghf.lib().ghf_compress_batch(ctx.h, r["in_ptrs"].data_ptr(), r["in_bytes"].data_ptr(), 8192, 16, r["out_ptrs"].data_ptr(),
                                          r["out_caps"].data_ptr(), r["out_bytes"].data_ptr(), None, None, r3_status.data_ptr())
        assert rc == 0
        ctx.sync()
        assert r3_status.cpu().tolist() == [OK] * 16
        assert np.array_equal(r["out"].cpu().numpy()[: nb[0]], orc.compress(datas[0]))
    finally:
        ctx.batch_index_free(bidx)
