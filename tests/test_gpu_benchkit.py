"""GPU: tools/benchkit.py on the device.  Its timed loop with the real cache sweep gives finite, positive samples, and an
empty callable measures less than a 256 MiB copy: the sweep copy, which is as large and runs in front of every sample, is
outside the events (inside them, the empty variant would cost a 256 MiB copy too).  Only the order is held, no ratio.  Every
input generator of the kit gives the same bytes for the same seed, of the asked size."""
import math
import os
import sys

import pytest

import pkgload

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

import benchkit  # noqa: E402

pytestmark = pytest.mark.gpu

N = 64 << 10
SEED = 7


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    ghf = pkgload.load().ghf
    ctx = ghf.Context(0)
    yield ghf, ctx, torch
    ctx.close()


def test_timed_with_the_sweep_on_the_device(env):
    ghf, ctx, torch = env
    L = ghf.lib()
    big = benchkit.SWEEP_BYTES
    d_src, d_dst = ctx.empty_u8(big), ctx.empty_u8(big)
    d_src.zero_()

    def copy(n):
        return lambda: benchkit.ok(L.ghf_copy_d2d(ctx.h, d_dst.data_ptr(), d_src.data_ptr(), n, 0))

    med, times = benchkit.timed([("empty", lambda: None), ("copy_1mib", copy(1 << 20)), ("copy_256mib", copy(big))], reps=5, warmup=1,
                                sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))
    print({k: [round(x, 4) for x in v] for k, v in times.items()})
    assert list(times) == ["empty", "copy_1mib", "copy_256mib"]
    for name, v in times.items():
        assert len(v) == 5, name
        assert all(math.isfinite(x) and x > 0 for x in v), (name, v)
    assert med["empty"] < med["copy_256mib"], med


def generators(torch):
    """(name, call with the seed, dtype, bytes) of every generator of the kit at N bytes"""
    k = benchkit
    return [("normal_fp32", lambda s: k.normal_fp(torch, N, 4, s)), ("normal_fp64", lambda s: k.normal_fp(torch, N, 8, s)),
            ("normal_bf16_truncated", lambda s: k.normal_bf16_truncated(torch, N, s)),
            ("normal_bf16_rounded", lambda s: k.normal_bf16_rounded(torch, N, s)),
            ("normal_elems_2", lambda s: k.normal_elems(torch, N, 2, s)), ("normal_elems_8", lambda s: k.normal_elems(torch, N, 8, s)),
            ("uniform_bytes", lambda s: k.uniform_bytes(torch, N, s)), ("sparse_bytes_1pct", lambda s: k.sparse_bytes_1pct(torch, N, s)),
            ("zipf_bytes", lambda s: k.zipf_bytes(torch, N, s))]


def test_generators_repeat_for_one_seed(env):
    _, _, torch = env
    for name, make in generators(torch):
        a, b, other = make(SEED), make(SEED), make(SEED + 1)
        assert a.dtype == torch.uint8 and a.is_cuda and a.numel() == N, name
        assert torch.equal(a, b), name
        assert not torch.equal(a, other), name
    # what the names say: the two bf16 makers differ (rounding carries into the kept half), normal_elems picks by width
    assert torch.equal(benchkit.normal_elems(torch, N, 2, SEED), benchkit.normal_bf16_truncated(torch, N, SEED))
    assert torch.equal(benchkit.normal_elems(torch, N, 8, SEED), benchkit.normal_fp(torch, N, 8, SEED))
    assert not torch.equal(benchkit.normal_bf16_rounded(torch, N, SEED), benchkit.normal_bf16_truncated(torch, N, SEED))
    nonzero = int(torch.count_nonzero(benchkit.sparse_bytes_1pct(torch, N, SEED)).item())
    assert 0 < nonzero < N // 25  # 1 in 100 expected: 655 of 65536


def test_pair_generators(env):
    _, _, torch = env
    for e in (2, 4, 8):
        new, base = benchkit.normal_pair(torch, N, e, None, SEED)
        assert new.dtype == base.dtype == torch.uint8 and new.numel() == base.numel() == N, e
        assert torch.equal(new, base) and new.data_ptr() != base.data_ptr(), e
        assert torch.equal(base, benchkit.normal_elems(torch, N, e, SEED)), e
        new1, base1 = benchkit.normal_pair(torch, N, e, 1e-3, SEED)
        new2, base2 = benchkit.normal_pair(torch, N, e, 1e-3, SEED)
        assert torch.equal(new1, new2) and torch.equal(base1, base2) and torch.equal(base1, base), e
        assert new1.numel() == N and not torch.equal(new1, base1), e
    for e in (2, 4):
        new1, base1 = benchkit.normal_pair_reseeded(torch, N, e, 1e-3, SEED)
        new2, base2 = benchkit.normal_pair_reseeded(torch, N, e, 1e-3, SEED)
        assert new1.dtype == torch.uint8 and new1.numel() == base1.numel() == N, e
        assert torch.equal(new1, new2) and torch.equal(base1, base2), e
        assert torch.equal(base1, benchkit.normal_elems(torch, N, e, SEED)) and not torch.equal(new1, base1), e
        assert not torch.equal(new1, benchkit.normal_pair(torch, N, e, 1e-3, SEED)[0]), e  # the two pairs draw other steps
