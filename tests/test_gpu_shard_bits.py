"""GPU (-m gpu): K5 (ghf_encode_emit) as the sharded encode drives it, at the start bits of BASELINE config 4 (32 GiB over 8
GPUs: rank 7 starts near 2^38) and at every bit phase, against the exact model of tests/shard_model.py.  One process, one
context, the staged C ABI: the ranks are emulated one after the other -- K1 per shard, the histograms summed (slot 256 back
to 1), ghf_build_code once, then per shard ghf_encode_plan, the totals, ghf_shard_start_bit, ghf_shard_bytes and
ghf_encode_emit with the flags ghf_encode_sharded uses.  A start bit is only a number K5 reads, so one plan serves emits at
many start bits, and config-4 start bits need no 32 GiB of data in front of them."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import datagen as dg  # noqa: E402
import pkgload  # noqa: E402
import shard_model as sm  # noqa: E402

LAST, REBASE, HEADER, LONG = 1, 2, 4, 8
CANARY = 0xA5
SLACK = 64  # canary bytes behind every buffer K5 is given
E_INVAL, E_CAP = 1, 5

CONFIG4_S = 275_000_000_000  # BASELINE config 4, rank 7: about 2.75e11 bits into the stream
MAGNITUDES = {  # S is placed a little in front of these bits, so that the shard's bits cross them inside its first chunk
    "2^31": 1 << 31, "2^32": 1 << 32, "2^35": 1 << 35, "2^38": 1 << 38, "2^40": 1 << 40, "2^44-2^20": (1 << 44) - (1 << 20),
    "config4_rank7": CONFIG4_S,
}
PHASES8 = (0, 1, 7, 8, 63, 64, 121, 127)


def s_at(mag, phase):
    """a start bit with S mod 128 == phase, 256..383 bits in front of the magnitude"""
    return ((MAGNITUDES[mag] - 256) // 128) * 128 + phase


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    ghf = pkgload.load().ghf
    ctx = ghf.Context(0)
    yield ghf, ctx, torch
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- helpers
def code_from_hist(ctx, torch, counts):
    """device tables of ghf_build_code for the 256 counts (slot 256 = 1) and their host copy"""
    h = np.concatenate([np.asarray(counts, dtype=np.int64), [1]])
    d_code = ctx.build_code(torch.from_numpy(h).cuda())
    ctx.sync()
    return d_code, ctx.code_to_host(d_code)


def global_codes(ctx, torch):
    """four global codes that are not a shard's own, and a data generator for each that leans on its long codes"""
    rng = np.random.default_rng(2024)
    zipf = np.bincount(dg.zipf_bytes(1 << 16, seed=3), minlength=256) + 1
    uni = np.bincount(dg.uniform_bytes(1 << 16, seed=4), minlength=256) + 1
    s16 = np.zeros(256, dtype=np.int64)
    s16[:16] = 1 << 16
    s16[200] = 1  # one rare byte: a code far longer than the others
    fib = np.zeros(256, dtype=np.int64)
    fib[:32] = dg.fib_counts(32)  # max_len 32
    out = {}
    for name, counts in (("zipf", zipf), ("uniform", uni), ("sym16_rare", s16), ("fib32_maxlen32", fib)):
        d_code, code = code_from_hist(ctx, torch, counts)
        lens = np.array(list(code.length)[:256], dtype=np.float64)
        used = np.nonzero(lens)[0]
        p = lens[used] ** 3
        p /= p.sum()
        out[name] = (d_code, code, used.astype(np.uint8), p)
    assert out["fib32_maxlen32"][1].max_len == 32 and out["sym16_rare"][1].length[200] > out["sym16_rare"][1].length[0]
    return out, rng


def shard_data(codes, name, n, seed):
    _, _, used, p = codes[name]
    return np.random.default_rng(seed).choice(used, size=n, p=p).astype(np.uint8)


class Shard:
    """one shard on the device, planned under one code; emit() may then run at any start bit"""

    def __init__(self, ghf, ctx, torch, data, d_code):
        self.ghf, self.ctx, self.torch = ghf, ctx, torch
        self.data = data
        self.n = data.size
        self.d_code = d_code
        self.d_in = torch.from_numpy(data).cuda() if data.size else torch.zeros(16, dtype=torch.uint8, device="cuda")
        # K1 first, as ghf_encode_sharded runs it: the plan reuses the per-chunk histograms of the last K1 whenever its
        # (pointer, n) match -- and a fresh tensor may sit at the address of a freed one that held other bytes
        ctx.histogram(self.d_in, n=self.n)
        self.total = ctx.encode_plan(self.d_in, d_code, n=self.n)

    def emit(self, S, flags, cap, out=None, index=None):
        """-> (out, d_end tensor).  out: a fresh buffer of cap + SLACK canary bytes unless given; K5 is told `cap`."""
        torch = self.torch
        if out is None:
            out = torch.full((cap + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
        assert cap <= out.numel()
        start = torch.tensor([S], dtype=torch.int64, device="cuda")
        end = torch.zeros(2, dtype=torch.int64, device="cuda")
        rc = self.ctx.L.ghf_encode_emit(self.ctx.h, self.d_in.data_ptr(), self.n, self.d_code.data_ptr(), start.data_ptr(), flags,
                                        out.data_ptr(), cap, None if index is None else C.byref(index), end.data_ptr())
        assert rc == 0, (rc, self.ctx.L.ghf_last_error(self.ctx.h))
        return out, end


def check_emit(ghf, ctx, torch, sh, code, S, flags, bits, with_index=True, decode=True):
    """one emit against the model: bytes, zeros in front of S and behind the end, d_end, canary, side-car, K7 round trip"""
    last = bool(flags & LAST)
    exp, (end, nbytes) = sm.expected_shard(sh.data, code, S, rebase=True, last=last, bits=bits)
    origin = sm.origin_of(S, True)
    cap = sm.min_cap(S, end, origin)
    idx = ctx.index_alloc(sh.n) if with_index else None
    out, d_end = sh.emit(S, flags, cap, index=idx)
    ctx.sync()
    got = out.cpu().numpy()
    assert [int(x) for x in d_end.tolist()] == [end, nbytes], (S, flags)
    # [0, cap): the model's bytes, then zeros up to the end of the last unit written; behind cap the canary
    want = np.zeros(cap, dtype=np.uint8)
    want[:nbytes] = exp
    assert np.array_equal(got[:cap], want), (S, flags, sm_first_diff(got[:cap], want))
    assert (got[cap:] == CANARY).all(), (S, flags)
    if with_index:
        chunk_bit, seg_bit = ctx.index_to_host(idx)
        e_chunk, e_seg = sm.expected_index(sh.data, code, S, origin)
        assert np.array_equal(chunk_bit, e_chunk) and np.array_equal(seg_bit, e_seg), (S, flags)
        if decode:
            idx.flags = 0 if last else ghf.INDEX_NO_END_MARK
            back, nout = ctx.decode(out, cap, sh.d_code, idx)
            ctx.sync()
            assert int(nout.item()) == sh.n and np.array_equal(back[: sh.n].cpu().numpy(), sh.data), (S, flags)
        ctx.index_free(idx)


def sm_first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return (int(d[0]) if d.size else None, a.size, b.size)


# ----------------------------------------------------------------------------------------------- a. start-bit sweep
@pytest.mark.parametrize("n", [0, 1, 3, 64, 4097, 3 * 16384 + 5, (1 << 20) + 3])
def test_start_bits_at_config4_magnitudes(env, n):
    """every magnitude x phases {0, 1, 7, 8, 63, 64, 121, 127} x four global codes x {REBASE, REBASE|LAST}: bytes, d_end, the
    side-car and a K7 round trip, all exact.  n == 0 is an empty shard (k_emit_empty).  The 1 MiB shard runs at three
    magnitudes (its chunks are many: the carry path between chunks is what it adds, and that does not depend on S's size)."""
    ghf, ctx, torch = env
    codes, _ = global_codes(ctx, torch)
    mags = list(MAGNITUDES) if n < (1 << 20) else ["2^32", "2^38", "config4_rank7"]
    checked = 0
    for ci, name in enumerate(codes):
        d_code, code = codes[name][:2]
        data = shard_data(codes, name, n, seed=n + ci)
        sh = Shard(ghf, ctx, torch, data, d_code)
        bits = sm.code_bits(data, code)
        ctx.sync()
        assert int(sh.total.item()) == bits.size
        for mag in mags:
            for ph in PHASES8:
                for flags in (REBASE, REBASE | LAST):
                    check_emit(ghf, ctx, torch, sh, code, s_at(mag, ph), flags, bits, decode=n < (1 << 20) or ph in (0, 121))
                    checked += 1
    assert checked == len(codes) * len(mags) * len(PHASES8) * 2


@pytest.mark.parametrize("mag", ["2^35", "config4_rank7"])
def test_every_phase_mod_128(env, mag):
    """all 128 values of S mod 128 for n in {0, 1, 3, 64, 4097}, zipf and max_len-32 codes, {REBASE, REBASE|LAST}: bytes and d_end
    (the 8-phase sweep above checks the side-car and the decode).  128 emits into one buffer, one synchronisation."""
    ghf, ctx, torch = env
    codes, _ = global_codes(ctx, torch)
    for name in ("zipf", "fib32_maxlen32"):
        d_code, code = codes[name][:2]
        for n in (0, 1, 3, 64, 4097):
            data = shard_data(codes, name, n, seed=7 * n)
            sh = Shard(ghf, ctx, torch, data, d_code)
            bits = sm.code_bits(data, code)
            for flags in (REBASE, REBASE | LAST):
                exps = [sm.expected_shard(data, code, s_at(mag, ph), True, bool(flags & LAST), bits=bits) for ph in range(128)]
                caps = [sm.min_cap(s_at(mag, ph), e[1][0], sm.origin_of(s_at(mag, ph), True)) for ph, e in enumerate(exps)]
                stride = (max(caps) + SLACK + 15) // 16 * 16
                big = torch.full((128 * stride,), CANARY, dtype=torch.uint8, device="cuda")
                ends = []
                for ph in range(128):
                    _, d_end = sh.emit(s_at(mag, ph), flags, caps[ph], out=big[ph * stride : (ph + 1) * stride])
                    ends.append(d_end)
                ctx.sync()
                host = big.cpu().numpy().reshape(128, stride)
                for ph in range(128):
                    exp, (end, nbytes) = exps[ph]
                    assert [int(x) for x in ends[ph].tolist()] == [end, nbytes], (name, n, flags, ph)
                    want = np.full(stride, CANARY, dtype=np.uint8)
                    want[: caps[ph]] = 0
                    want[:nbytes] = exp
                    assert np.array_equal(host[ph], want), (name, n, flags, ph, sm_first_diff(host[ph], want))


# ------------------------------------------------------------------------------------------------- b. capacity edge
def test_capacity_edge(env):
    """cap = the smallest value K5's `fits` rule accepts succeeds and leaves the canary alone (ends inside a unit and exactly
    on a 128-bit boundary); cap - 1 latches GHF_E_CAP and writes nothing; ghf_shard_bytes is never below that minimum and at
    most 16 bytes above d_end[1]."""
    ghf, ctx, torch = env
    codes, _ = global_codes(ctx, torch)
    seen_boundary = 0
    for ci, name in enumerate(codes):
        d_code, code = codes[name][:2]
        for n in (0, 1, 5, 4097, 3 * 16384 + 5):
            data = shard_data(codes, name, n, seed=100 + n + ci)
            sh = Shard(ghf, ctx, torch, data, d_code)
            T = sm.body_bits(data, code)
            el = code.length[256]
            for flags in (REBASE, REBASE | LAST):
                tail = el if flags & LAST else 0
                base = s_at("2^35", 0)
                # one start bit whose end falls inside a unit, one whose end lands exactly on a unit boundary
                for S in (base + 37, base + (-(T + tail)) % 128):  # inside a unit / exactly on a unit boundary
                    exp, (end, nbytes) = sm.expected_shard(data, code, S, True, bool(flags & LAST))
                    origin = sm.origin_of(S, True)
                    cap = sm.min_cap(S, end, origin)
                    seen_boundary += end % 128 == 0
                    out, d_end = sh.emit(S, flags, cap)
                    ctx.sync()
                    got = out.cpu().numpy()
                    assert [int(x) for x in d_end.tolist()] == [end, nbytes]
                    assert np.array_equal(got[:nbytes], exp) and not got[nbytes:cap].any() and (got[cap:] == CANARY).all(), (name, n, S)
                    if cap > 0:  # (an empty non-last shard that starts on a unit boundary defines no byte at all)
                        out, _ = sh.emit(S, flags, cap - 1)
                        with pytest.raises(ghf.GhfError) as e:
                            ctx.sync()
                        assert e.value.status == E_CAP
                        assert (out.cpu().numpy() == CANARY).all(), (name, n, S, "wrote behind a refused capacity")
                    # ghf_shard_bytes for the same start and total: rank 1 of 2 behind a rank 0 of S - header bits
                    world = 2 if flags & LAST else 3
                    totals = [S - sm.header_bits(code), T] + ([5] if world == 3 else [])
                    d_tot = torch.tensor(totals, dtype=torch.int64, device="cuda")
                    sb = ctx.shard_bytes(d_code, d_tot, world, 1)
                    assert sb == sm.shard_bytes(code, totals, world, 1)
                    assert cap <= sb <= nbytes + 16, (cap, sb, nbytes)
    assert seen_boundary >= 8


# --------------------------------------------------------------------------------------------- c. shard arithmetic
def test_shard_start_bit_and_shard_bytes_against_integers(env):
    ghf, ctx, torch = env
    codes, _ = global_codes(ctx, torch)
    rng = np.random.default_rng(77)
    for world in (1, 2, 8, 64, 4096):
        totals = rng.integers(0, 1 << 40, size=world, dtype=np.int64)
        totals[rng.random(world) < 0.25] = 0
        if world > 1:
            totals[0] = 0
            totals[-1] = 0
        d_tot = torch.from_numpy(totals).cuda()
        ranks = list(range(world)) if world <= 64 else sorted(set([0, 1, world // 2, world - 2, world - 1] + rng.integers(0, world, 59).tolist()))
        for name in codes:
            d_code, code = codes[name][:2]
            starts = torch.zeros(len(ranks), dtype=torch.int64, device="cuda")
            for k, r in enumerate(ranks):
                ctx.shard_start_bit(d_code, d_tot, world, r, out=starts[k : k + 1])
            got = [int(x) for x in starts.cpu().tolist()]
            assert got == [sm.start_bit(code, totals.tolist(), r) for r in ranks], (world, name)
            for r in ranks:
                assert ctx.shard_bytes(d_code, d_tot, world, r) == sm.shard_bytes(code, totals.tolist(), world, r), (world, name, r)
    d_code = codes["zipf"][0]
    d_tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    for world, rank in ((4, 4), (4, 9), (0, 0), (4, -1)):
        for f in (lambda: ctx.shard_start_bit(d_code, d_tot, world, rank), lambda: ctx.shard_bytes(d_code, d_tot, world, rank)):
            with pytest.raises(ghf.GhfError) as e:
                f()
            assert e.value.status == E_INVAL, (world, rank)


# ------------------------------------------------------------------------------------------ d. adjacent pairs at large S
def test_adjacent_pairs_merge_at_large_start_bits(env):
    ghf, ctx, torch = env
    codes, _ = global_codes(ctx, torch)
    for ci, name in enumerate(codes):
        d_code, code = codes[name][:2]
        for na, nb in ((3, 4097), (4097, 1), (3 * 16384 + 5, 70)):
            a = shard_data(codes, name, na, seed=na + ci)
            b = shard_data(codes, name, nb, seed=nb + 31 * ci)
            sa = Shard(ghf, ctx, torch, a, d_code)
            Ta = sm.body_bits(a, code)
            both = np.concatenate([a, b])
            for mag in ("2^35", "config4_rank7"):
                for ph in (0, 5, 64, 127):
                    Sa = s_at(mag, ph)
                    Sb = Sa + Ta
                    for last in (False, True):
                        ea = sm.expected_shard(a, code, Sa, True, False)[1]
                        eb = sm.expected_shard(b, code, Sb, True, last)[1]
                        oa, ob = sm.origin_of(Sa, True), sm.origin_of(Sb, True)
                        out_a, end_a = sa.emit(Sa, REBASE, sm.min_cap(Sa, ea[0], oa))
                        sb_ = Shard(ghf, ctx, torch, b, d_code)  # (the plan is the context's: re-plan b after a's emit)
                        out_b, end_b = sb_.emit(Sb, REBASE | (LAST if last else 0), sm.min_cap(Sb, eb[0], ob))
                        ctx.sync()
                        pieces = [(oa - oa, int(end_a[0].item()), out_a[: int(end_a[1].item())].cpu().numpy()),
                                  (ob - oa, int(end_b[0].item()), out_b[: int(end_b[1].item())].cpu().numpy())]
                        got = np.zeros(max(o + p.size for o, _, p in pieces), dtype=np.uint8)
                        for o, _, p in pieces:
                            got[o : o + p.size] |= p
                        exp, (end, nbytes) = sm.expected_shard(both, code, Sa, True, last)
                        assert int(end_b[0].item()) == end and got.size == nbytes and np.array_equal(got, exp), (name, na, nb, mag, ph, last)
                        sa = Shard(ghf, ctx, torch, a, d_code)


# ------------------------------------------------------------------------- e. whole streams from shards vs the reference
def _cuts(n):
    cuts = {"w2": sm.cuts_even(n, 2), "w8": sm.cuts_even(n, 8), "w8_random": sm.cuts_random(n, 8, seed=n)}
    if n <= 64:
        cuts["w_n+1"] = sm.cuts_random(n, n + 1, seed=1)
        cuts["w_n+3"] = sm.cuts_random(n, n + 3, seed=3)
    return cuts


def encode_cut(ghf, ctx, torch, d_all, data, cuts):
    """the ranks of one cut in sequence, as ghf_encode_sharded runs them -> (merged stream, d_code, [(out, idx, n, flags)])"""
    world = len(cuts) - 1
    views = [d_all[cuts[g] : cuts[g + 1]] for g in range(world)]
    hist = torch.zeros(257, dtype=torch.int64, device="cuda")
    for g in range(world):
        hist += ctx.histogram(views[g], n=cuts[g + 1] - cuts[g])
    hist[256] = 1
    d_code = ctx.build_code(hist)
    totals = torch.zeros(world, dtype=torch.int64, device="cuda")
    for g in range(world):
        ctx.encode_plan(views[g], d_code, n=cuts[g + 1] - cuts[g], total=totals[g : g + 1])
    shards, pieces = [], []
    for g in range(world):
        n = cuts[g + 1] - cuts[g]
        start = ctx.shard_start_bit(d_code, totals, world, g)
        cap = ctx.shard_bytes(d_code, totals, world, g)  # (synchronises)
        flags = (LAST if g == world - 1 else 0) | (REBASE if g > 0 else HEADER)
        out = torch.full((cap + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
        idx = ctx.index_alloc(n)
        idx.flags = 0 if g == world - 1 else ghf.INDEX_NO_END_MARK
        ctx.encode_plan(views[g], d_code, n=n)
        end = torch.zeros(2, dtype=torch.int64, device="cuda")
        rc = ctx.L.ghf_encode_emit(ctx.h, views[g].data_ptr(), n, d_code.data_ptr(), start.data_ptr() if g > 0 else None, flags,
                                   out.data_ptr(), cap, C.byref(idx), end.data_ptr())
        assert rc == 0
        ctx.sync()
        S = int(start.item())
        e = [int(x) for x in end.tolist()]
        host = out.cpu().numpy()
        assert (host[cap:] == CANARY).all(), ("canary", g)
        assert e[1] <= cap <= e[1] + 16
        origin = sm.origin_of(S, g > 0)
        pieces.append((origin, e[0], host[: e[1]]))
        shards.append((out, idx, n, cuts[g], e[1]))
    return sm.merge(pieces), d_code, shards


@pytest.mark.parametrize("name", sorted(__import__("cases").CASES))
def test_whole_stream_from_shards_equals_the_reference(env, golden, name):
    """every golden case at world 2 and 8 (even), world 8 with empty shards at rank 0, in the middle and at the last rank, and
    -- for the tiny cases -- more ranks than bytes: the merged shards have the reference's SHA-256, every shard decodes with
    its own side-car, the merged stream decodes without one (K6)"""
    from cases import CASES

    ghf, ctx, torch = env
    data = CASES[name]()
    d_all = torch.from_numpy(data).cuda()
    stream = None
    for label, cuts in _cuts(data.size).items():
        stream, d_code, shards = encode_cut(ghf, ctx, torch, d_all, data, cuts)
        assert hashlib.sha256(stream.tobytes()).hexdigest() == golden[name]["crs2_sha256"], (name, label)
        for out, idx, n, lo, nb in shards:
            back, nout = ctx.decode(out, nb, d_code, idx)
            ctx.sync()
            assert int(nout.item()) == n and np.array_equal(back[:n].cpu().numpy(), data[lo : lo + n]), (name, label, lo)
            ctx.index_free(idx)
    # the merged stream is the reference's (asserted for every cut above): once through K6, no side-car
    d_stream = torch.from_numpy(np.concatenate([stream, np.zeros(64, dtype=np.uint8)])).cuda()
    hcode, _ = ghf.parse_header(stream)
    back, nout = ctx.decode(d_stream, stream.size, ctx.code_to_device(hcode), None, cap=data.size + 64)
    ctx.sync()
    assert int(nout.item()) == data.size and np.array_equal(back[: data.size].cpu().numpy(), data)


# ---------------------------------------------------------------------------------------------------- f. long codes
def test_long_codes_at_large_start_bits(env):
    """codes of 40 and 64 bits (a hand-built comb, as in test_gpu_crs.py) packed by k_emit_long under REBASE at S >= 2^36"""
    from test_gpu_crs import _comb

    ghf, ctx, torch = env
    for depth in (40, 64):
        _, codes, lens = _comb(depth)
        code = ghf.Code()
        for s in range(ghf.NSYM):
            code.length[s], code.codeword[s], code.symbol[s] = 0, 0, 0xFFFFFFFF
        for s, (c, l) in enumerate(zip(codes, lens)):
            code.length[s], code.codeword[s], code.symbol[s] = l, c & 0xFFFFFFFF, c >> 32
        code.min_len, code.max_len = 1, depth
        d_code = ctx.code_to_device(code)
        rng = np.random.default_rng(depth)
        data = rng.choice(np.arange(depth + 1), size=5000 + depth, p=np.array([1.0] * (depth - 1) + [30.0, 30.0]) / (depth + 59.0)).astype(np.uint8)
        ref_bits = "".join(format(codes[v], "0%db" % lens[v]) for v in data.tolist())
        bits = sm.code_bits(data, code)
        assert "".join(map(str, bits.tolist())) == ref_bits
        sh = Shard(ghf, ctx, torch, data, d_code)
        for ph in (0, 1, 63, 64, 127):
            S = (1 << 36) + 128 * 1000 + ph
            check_emit(ghf, ctx, torch, sh, code, S, REBASE | LONG, bits, with_index=True, decode=False)


# ------------------------------------------------------------------------------------------------- g. real sizes, once
def test_config4_ranks_3_and_7_at_their_real_start_bits(env):
    """BASELINE config 4's global code from eight 4 GiB uniform shards generated one at a time on the device; rank 3 (REBASE)
    and rank 7 (REBASE|LAST) emitted at their real start bits and again at S' = 128 k + (S mod 128): identical bytes and
    side-cars (chunk_bit counts from d_out[0]); the first MiB and the last 64 KiB against the model; both decode back."""
    import importlib

    ghf, ctx, torch = env
    synth = importlib.import_module("golden_huffman_amd.synth")
    G, world = 4 << 30, 8
    gen = lambda r: synth.make(torch, "uniform", G, device="cuda", seed=dg.DEFAULT_SEED, offset=r * G)  # noqa: E731
    hist = torch.zeros(257, dtype=torch.int64, device="cuda")
    for r in range(world):
        d = gen(r)
        hist += ctx.histogram(d)
        ctx.sync()
        del d
    hist[256] = 1
    d_code = ctx.build_code(hist)
    code = ctx.code_to_host(d_code)
    totals = torch.zeros(world, dtype=torch.int64, device="cuda")
    for r in range(world - 1):
        d = gen(r)
        ctx.histogram(d)  # (K1 in front of every plan: see Shard)
        ctx.encode_plan(d, d_code, total=totals[r : r + 1])
        ctx.sync()
        del d
    m, t = 1 << 20, 64 << 10
    for rank in (3, 7):
        d_in = gen(rank)
        ctx.histogram(d_in)
        ctx.encode_plan(d_in, d_code, total=totals[rank : rank + 1])
        start = ctx.shard_start_bit(d_code, totals, world, rank)
        cap = ctx.shard_bytes(d_code, totals, world, rank)
        S = int(start.item())
        assert S == sm.start_bit(code, totals.cpu().tolist(), rank) and S > (1 << 36)
        flags = REBASE | (LAST if rank == world - 1 else 0)
        outs, idxs, ends = [], [], []
        for s_k in (S, 128 * 3 + S % 128):
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            idx = ctx.index_alloc(G)
            idx.flags = 0 if flags & LAST else ghf.INDEX_NO_END_MARK
            st = torch.tensor([s_k], dtype=torch.int64, device="cuda")
            end = torch.zeros(2, dtype=torch.int64, device="cuda")
            assert ctx.L.ghf_encode_emit(ctx.h, d_in.data_ptr(), G, d_code.data_ptr(), st.data_ptr(), flags, out.data_ptr(), cap,
                                         C.byref(idx), end.data_ptr()) == 0
            ctx.sync()
            outs.append(out)
            idxs.append(idx)
            ends.append([int(x) for x in end.tolist()])
        del out
        nb = ends[0][1]
        assert ends[0][0] == sm.end_bit(code, totals.cpu().tolist(), world, rank) and ends[1][1] == nb
        assert ends[0][0] - ends[1][0] == S - (128 * 3 + S % 128)
        assert bool(torch.equal(outs[0][:nb], outs[1][:nb]))
        h0, h1 = ctx.index_to_host(idxs[0]), ctx.index_to_host(idxs[1])
        assert np.array_equal(h0[0], h1[0]) and np.array_equal(h0[1], h1[1])
        # first MiB and last 64 KiB against the model
        origin = sm.origin_of(S, True)
        head_n = m + 4096
        head_data = d_in[:head_n].cpu().numpy()
        exp, _ = sm.expected_shard(head_data, code, S, True, False)
        assert np.array_equal(outs[0][:m].cpu().numpy(), exp[:m])
        tail_data = d_in[G - 2 * t :].cpu().numpy()
        S_tail = ends[0][0] - sm.body_bits(tail_data, code) - (ends[0][0] - S - int(totals[rank].item()))
        exp_t, (end_t, nb_t) = sm.expected_shard(tail_data, code, S_tail, True, bool(flags & LAST))
        o_t = sm.origin_of(S_tail, True) - origin
        assert end_t == ends[0][0] and o_t + nb_t == nb
        assert np.array_equal(outs[0][nb - t : nb].cpu().numpy(), exp_t[nb_t - t :])
        e_chunk, _ = sm.expected_index(head_data, code, S, origin)
        assert np.array_equal(h0[0][: e_chunk.size], e_chunk)
        del outs[1], h0, h1
        ctx.index_free(idxs[1])
        back, nout = ctx.decode(outs[0], nb, d_code, idxs[0])
        ctx.sync()
        assert int(nout.item()) == G
        for lo in range(0, G, 1 << 30):
            assert bool(torch.equal(back[lo : lo + (1 << 30)], d_in[lo : lo + (1 << 30)])), (rank, lo)
        ctx.index_free(idxs[0])
        del back, outs, d_in
        torch.cuda.empty_cache()
