"""GPU (-m gpu): K5 (ghf_encode_emit) across chunk seams -- every packer at every carry (tier A), every route a chunk takes
behind a seam and every front of chunk 0 (tier B), and the plan behind them (tier C) -- against the exact model of
tests/emit_seams.py.  The calls are K1, ghf_encode_plan and ghf_encode_emit as test_gpu_shard_bits.py's Shard makes them.
Every output buffer is 0xA5 (or, where the emit must keep what d_out holds, a seeded pattern) with 64 guard bytes behind
the smallest cap K5 accepts; d_end, every byte of [0, cap), the guard and the side-car are compared.  A mismatch names the
code, the fill, the size, the start bit's phase, the seam with its carry, and the routes of the emit."""
import ctypes as C

import numpy as np
import pytest

import emit_seams as es
import test_gpu_shard_bits as t_sb
from test_gpu_shard_bits import CANARY, SLACK, env  # noqa: F401  (env: the module's context)

pytestmark = pytest.mark.gpu

ids_of = lambda code: "%d_%d-%s" % (code.shape + (code.label.replace("/", "."),))  # noqa: E731


def device_code(torch, code):
    t = torch.from_numpy(np.frombuffer(bytes(code.code), dtype=np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


class SeamShard(t_sb.Shard):
    """a Shard whose bytes stand `offset` bytes behind a 16-byte boundary, planned behind K1 of the same buffer or -- after
    K1 of another one -- by the plan's own direct pass"""

    def __init__(self, ghf, ctx, torch, data, d_code, offset=0, plan="behind_k1"):
        self.ghf, self.ctx, self.torch = ghf, ctx, torch
        self.data, self.n, self.d_code = data, data.size, d_code
        self.whole = torch.zeros(offset + data.size + 16, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.d_in = self.whole[offset : offset + data.size]
        self.d_in.copy_(torch.from_numpy(data.copy()))  # (the cases' arrays are read-only)
        if plan == "behind_k1":
            ctx.histogram(self.d_in, n=self.n)
        else:
            self.other = torch.zeros(4096, dtype=torch.uint8, device="cuda")
            ctx.histogram(self.other)  # the context's chunk histograms now describe another buffer
        self.total = ctx.encode_plan(self.d_in, d_code, n=self.n)

    def emit(self, S, flags, cap, out=None, index=None):
        if S is not None:
            return super().emit(S, flags, cap, out=out, index=index)
        end = self.torch.zeros(2, dtype=self.torch.int64, device="cuda")  # d_start_bit = NULL: the header's end
        rc = self.ctx.L.ghf_encode_emit(self.ctx.h, self.d_in.data_ptr(), self.n, self.d_code.data_ptr(), None, flags, out.data_ptr(), cap,
                                        None if index is None else C.byref(index), end.data_ptr())
        assert rc == 0, (rc, self.ctx.L.ghf_last_error(self.ctx.h))
        return out, end


def run(env, sh, cs_, variants, decode=()):  # noqa: F811
    """every variant's emit of one planned shard into one arena, one synchronisation, then every comparison.
    decode: the variants that are decoded back as well (with their side-car; header fronts also without one).
    -> the bytes [0, cap) of every emit"""
    ghf, ctx, torch = env
    exps = [cs_.expect(v) for v in variants]
    stride = (max(e.cap for e in exps) + SLACK + 15) // 16 * 16
    host = np.full((len(exps), stride), CANARY, dtype=np.uint8)
    for j, e in enumerate(exps):
        if e.held is not None:
            host[j, : e.cap] = e.held
    want = host.copy()
    big = torch.from_numpy(host).cuda()
    ends, idxs = [], []
    for j, (v, e) in enumerate(zip(variants, exps)):
        idx = ctx.index_alloc(cs_.n) if v.car else None
        _, d_end = sh.emit(e.S, e.flags, e.cap, out=big[j], index=idx)
        ends.append(d_end)
        idxs.append(idx)
    ctx.sync()
    got = big.cpu().numpy()
    for j, (v, e) in enumerate(zip(variants, exps)):
        tag = (repr(cs_), v, "seams (chunk, carry): %r" % (cs_.seams(e.lead % 128),), "routes: %s" % ",".join(sorted(es.routes(cs_, v))))
        assert [int(x) for x in ends[j].tolist()] == [e.end, e.nbytes], tag + ("d_end",)
        want[j, : e.cap] = e.image
        if not np.array_equal(got[j], want[j]):
            at = int(np.flatnonzero(got[j] != want[j])[0])
            where = "the guard behind cap" if at >= e.cap else cs_.blame(e, at)
            raise AssertionError(tag + ("first wrong byte %d of cap %d: %s" % (at, e.cap, where),))
        if v.car:
            chunk_bit, seg_bit = ctx.index_to_host(idxs[j])
            e_chunk, e_seg = cs_.index(e.lead)
            assert np.array_equal(chunk_bit, e_chunk) and np.array_equal(seg_bit, e_seg), tag + ("side-car",)
        if v in decode:
            for idx in ([idxs[j]] if v.car else []) + ([None] if v.front == "header_last" else []):  # None: K6 finds its own way
                if idx is not None:
                    idx.flags = 0 if e.flags & es.LAST else ghf.INDEX_NO_END_MARK
                nb = e.nbytes if v.front == "header_last" else e.cap  # (a whole stream ends with its end mark's byte)
                back, nout = ctx.decode(big[j], nb, sh.d_code, idx, cap=cs_.n + 64)
                ctx.sync()
                assert int(nout.item()) == cs_.n and np.array_equal(back[: cs_.n].cpu().numpy(), cs_.data), tag + ("decode", idx is not None)
        if idxs[j] is not None:
            ctx.index_free(idxs[j])
    return [got[j, : e.cap] for j, e in enumerate(exps)]


# ------------------------------------------------------------------------------------------- A. every carry at every seam
@pytest.mark.parametrize("code", es.codes(), ids=ids_of)
def test_every_carry_at_both_seams(env, code):  # noqa: F811
    """n = 2 * 16384 + 1029 (two seams; the last chunk: a full tile and 5 symbols), the last 128 symbols in front of either
    seam all of the least length / all the deepest symbol / as drawn / all the symbol with the most 1 bits, S = 2^35 + ph for all 128 ph, REBASE | LAST with a side-car
    (the codes beyond 32 bits: REBASE | LONG_CODES; ghf_decode takes no such code, so they have no round trip).  Both seams
    take every carry 0..127 (test_emit_seams_cpu.py); for ph in PHASES8 the bytes also decode back through K7."""
    ghf, ctx, torch = env
    d_code = device_code(torch, code)
    checked = 0
    for cs_, variants in es.tier_a(code):
        sh = SeamShard(ghf, ctx, torch, cs_.data, d_code)
        assert int(sh.total.item()) == cs_.bits.size, cs_
        run(env, sh, cs_, variants, decode=() if code.long else [v for v in variants if v.ph in es.PHASES8])
        cs_.forget()
        checked += len(variants)
    assert checked == 4 * 128


# --------------------------------------------------------------------------------------------------------- B. every route
@pytest.mark.parametrize("align", es.ALIGNS)
@pytest.mark.parametrize("code", es.route_codes(), ids=lambda c: es.PACKERS[c.packer].replace("<=", "_le_"))
def test_every_route_behind_a_seam(env, code, align):  # noqa: F811
    """one code per packer, nothing but its deepest code in front of every seam, then nothing but its code with the most 1
    bits; n = 16384 + {1, 15, 16, 17, 1023, 1024, 1025,
    4095, 4096, 4097, 5120, 5121, 9223}, 2 * 16384 and 3 * 16384; d_in `align` bytes behind a 16-byte boundary; with and
    without a side-car; ph in PHASES8 under REBASE, REBASE | LAST, and flags 0 and LAST into a buffer that holds a seeded
    pattern (which the emit must keep in front of its start bit and behind its last unit); HEADER | LAST with d_start_bit =
    NULL, which must be header || oracle body (the model is: test_emit_seams_cpu.py) and decode with and without its
    side-car.  k_emit_long has no end mark and no header."""
    ghf, ctx, torch = env
    d_code = device_code(torch, code)
    checked = 0
    for cs_, variants in es.tier_b(code, align):
        sh = SeamShard(ghf, ctx, torch, cs_.data, d_code, offset=align)
        assert (sh.d_in.data_ptr() - align) % 16 == 0
        assert int(sh.total.item()) == cs_.bits.size, cs_
        run(env, sh, cs_, variants, decode=[v for v in variants if v.front == "header_last"])
        cs_.forget()
        checked += len(variants)
    assert checked == 2 * 15 * 2 * (2 * 8 if code.long else 4 * 8 + 1)


# ------------------------------------------------------------------------------------------ C. the plan behind the seams
@pytest.mark.parametrize("code", es.short_codes(), ids=ids_of)
def test_the_plan_behind_k1_and_its_direct_pass(env, code):  # noqa: F811
    """ghf_encode_plan behind ghf_histogram of the same buffer (it sums K1's per-chunk histograms) and after a histogram of
    another buffer (its own pass over the bytes), at offsets 0 and 3: the model's total, and the same emitted bytes"""
    ghf, ctx, torch = env
    d_code = device_code(torch, code)
    ((cs_, variants),) = es.tier_c(code)
    assert [(v.align, v.plan) for v in variants] == [(0, "behind_k1"), (0, "direct"), (3, "behind_k1"), (3, "direct")]
    outs = []
    for v in variants:
        sh = SeamShard(ghf, ctx, torch, cs_.data, d_code, offset=v.align, plan=v.plan)
        assert int(sh.total.item()) == cs_.bits.size, (cs_, v)
        outs += run(env, sh, cs_, [v])
    assert all(np.array_equal(outs[0], o) for o in outs[1:])
    cs_.forget()
