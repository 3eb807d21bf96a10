"""What the bench tools in this directory share: how a call is timed, the cache sweep, the seeded inputs and the record.
A tool imports it as `import benchkit` (a script's own directory is on sys.path) and keeps what is its own: what it compares,
its cases, its REQUIRED rule, its defaults and the keys of its document.  Nothing here touches the GPU on import; torch
comes in as an argument, as it does in golden_huffman_amd.synth."""
import json
import os
import statistics
import sys

SWEEP_BYTES = 256 << 20  # the Infinity Cache of the MI355X holds 256 MiB
CACHE_SWEEP = "plain 256 MiB copy in front of every timed call"  # the document's "cache_sweep" field of a tool that sweeps


def ok(rc):
    """the status check of one library call"""
    assert rc == 0, rc


def _timing_event():
    import torch

    return torch.cuda.Event(enable_timing=True)


def timed(variants, reps, warmup, sync, sweep=None, event=_timing_event):
    """Times every (name, fn) of `variants` -> ({name: median ms}, {name: [ms of every repeat]}).  The order of events:

      1. `warmup` rounds, each calling every variant in the given order
      2. one sync()
      3. `reps` rounds, each taking one sample of every variant in the given order (so the variants are interleaved, and
         a drift of the machine falls on all of them alike)
      4. per sample, sweep() first if there is one: it is queued in front of e0.record() and so stays outside the events
      5. e0.record(); fn(); e1.record(): nothing else between the two records
      6. e1.synchronize(), then e0.elapsed_time(e1)
      7. one sync() behind the last round

    Without a sweep a sample depends on what the call before it left in the caches.  `event` makes one timing event; a test
    passes a recording fake, the tools pass nothing."""
    variants = list(variants)
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    sync()
    times = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            e0, e1 = event(), event()
            if sweep is not None:
                sweep()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    sync()
    return {k: statistics.median(v) for k, v in times.items()}, times


def cache_sweep(ctx):
    """-> the sweep for timed(): a plain (not non-temporal) ghf_copy_d2d of 256 MiB between two buffers made here, on ctx's
    stream, so that no figure depends on which variant ran before it"""
    src, dst = ctx.empty_u8(SWEEP_BYTES), ctx.empty_u8(SWEEP_BYTES)
    src.zero_()

    def sweep():
        ok(ctx.L.ghf_copy_d2d(ctx.h, dst.data_ptr(), src.data_ptr(), SWEEP_BYTES, 0))

    return sweep


# ---- inputs: CUDA uint8 tensors.  Two functions that draw different bytes stay two functions: recorded documents depend on
# which one their tool called.


def _generator(torch, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _as_elems(torch, x, e):
    """float values as bytes: e == 2 keeps the upper half of fp32 (bf16 by truncation)"""
    if e == 2:
        return (x.view(torch.int32) >> 16).to(torch.int16).view(torch.uint8)
    return x.view(torch.uint8)


def normal_fp(torch, n_bytes, e, seed):
    """n_bytes of standard-normal fp32 (e == 4) or fp64 (e == 8)"""
    dt = torch.float64 if e == 8 else torch.float32
    return torch.randn(n_bytes // e, generator=_generator(torch, seed), device="cuda", dtype=dt).view(torch.uint8)


def normal_bf16_truncated(torch, n_bytes, seed):
    """n_bytes of bf16: the upper halves of n_bytes / 2 standard-normal fp32 values"""
    return _as_elems(torch, torch.randn(n_bytes // 2, generator=_generator(torch, seed), device="cuda", dtype=torch.float32), 2)


def normal_bf16_rounded(torch, n_bytes, seed):
    """n_bytes of bf16: n_bytes / 2 standard-normal fp32 values rounded by .to(torch.bfloat16)"""
    x = torch.randn(n_bytes // 2, generator=_generator(torch, seed), device="cuda", dtype=torch.float32)
    return x.to(torch.bfloat16).view(torch.uint8)


def normal_elems(torch, n_bytes, e, seed):
    """n_bytes of standard-normal elements of e bytes: bf16 by truncation / fp32 / fp64"""
    return normal_bf16_truncated(torch, n_bytes, seed) if e == 2 else normal_fp(torch, n_bytes, e, seed)


def uniform_bytes(torch, n, seed):
    """n uniform bytes from a seeded torch.randint (not synth.make's: that one draws other bytes)"""
    return torch.randint(0, 256, (n,), generator=_generator(torch, seed), device="cuda", dtype=torch.uint8)


def sparse_bytes_1pct(torch, n, seed):
    """n bytes, one in a hundred non-zero, its value 1 .. 255"""
    g = _generator(torch, seed)
    x = torch.randint(0, 256, (n,), generator=g, device="cuda", dtype=torch.uint8)
    keep = torch.randint(0, 100, (n,), generator=g, device="cuda", dtype=torch.uint8) == 0
    return x.clamp_(min=1) * keep


def zipf_bytes(torch, n, seed):
    """n bytes with P(value k) ~ 1 / (k + 1), by inversion of the cumulative distribution, a piece at a time"""
    g = _generator(torch, seed)
    w = 1.0 / torch.arange(1, 257, device="cuda", dtype=torch.float64)
    cdf = (torch.cumsum(w, 0) / w.sum()).to(torch.float32)
    out = torch.empty(n, device="cuda", dtype=torch.uint8)
    for at in range(0, n, 1 << 26):
        m = min(1 << 26, n - at)
        u = torch.rand(m, generator=g, device="cuda", dtype=torch.float32)
        out[at : at + m] = torch.searchsorted(cdf, u).clamp_(max=255).to(torch.uint8)
    return out


def normal_pair(torch, n_bytes, e, step, seed):
    """(new, base), n_bytes each: standard-normal values (fp64 for e == 8, else fp32) and the same after a step of relative
    size `step`, both drawn from ONE generator, the step behind the values; step None: new is base"""
    g = _generator(torch, seed)
    dt = torch.float64 if e == 8 else torch.float32
    w = torch.randn(n_bytes // e, generator=g, device="cuda", dtype=dt)
    base = _as_elems(torch, w, e)
    if step is None:
        return base.clone(), base
    return _as_elems(torch, w + step * torch.randn(n_bytes // e, generator=g, device="cuda", dtype=dt), e), base


def normal_pair_reseeded(torch, n_bytes, e, step, seed):
    """(new, base), n_bytes each, of fp32 (e == 4) or truncated bf16 (e == 2): as normal_pair, but the step is drawn after
    seeding the generator again with seed + 1, so `new` holds other bytes than normal_pair's"""
    n = n_bytes // e
    g = _generator(torch, seed)
    w = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    g.manual_seed(seed + 1)
    d = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    return _as_elems(torch, w + step * d, e).clone(), _as_elems(torch, w, e).clone()


# ---- the record


def add_args(ap, reps, warmup, out):
    """--reps, --warmup and --out with the tool's own defaults"""
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--out", default=out)


def envelope(torch, ghf, args, unit):
    """the fields every document opens with; the tool adds its own"""
    return {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "lib": ghf.lib_identity(), "unit": unit}


def stats(times):
    """{name: [ms]} -> the "median_ms", "min_ms" and "max_ms" dicts of a document, rounded to four places"""
    return {"median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
            "min_ms": {k: round(min(v), 4) for k, v in times.items()},
            "max_ms": {k: round(max(v), 4) for k, v in times.items()}}


def progress(obj):
    """one finished case as one JSON line on stderr, at once"""
    print(json.dumps(obj), file=sys.stderr, flush=True)


def save(doc, out):
    """the document into the file `out` (its directory is made), when `out` is set"""
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


def write(doc, out):
    """the closing step of a tool: the document on stdout, and into `out` when that is set"""
    print(json.dumps(doc, indent=1))
    save(doc, out)
