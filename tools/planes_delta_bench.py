#!/usr/bin/env python3
"""What the byte-plane calls against a base tensor cost, measured.  Not bench.py: this times typed
elements.  For every size in `--mib` (256 and 1024), every element width in `--widths` (2, 4, 8) and two kinds of data --
standard-normal values from a seeded generator (bf16 = the upper half of fp32, fp32, fp64) against the same values after a
step of relative size 1e-3, and uniform bytes against uniform bytes of another seed -- in one run:

  fused      each of ghf_histogram_planes_delta, ghf_planes_split_delta, ghf_planes_merge_delta,
             ghf_planes_merge_range_delta (first = 5, a skewed range), ghf_compress_planes_delta(GHF_PLANES_BUILD_CODES) and
             ghf_decode_planes_delta (side-cars)
  unfused    the pair it replaces: torch.bitwise_xor(..., out = a buffer allocated beforehand) plus the plain call (the XOR
             in front of a call that reads the interleaved side, behind one that writes it)
  plain      the plain parent of every kernel call on the same bytes, and ghf_copy_d2d(non_temporal = 1) of the bytes the
             call writes (of the bytes it reads, for the histogram, which writes next to nothing)
  stored     the bytes of the delta planes against the bytes of the planes of the new tensor

REQUIRED: every fused call is faster than its unfused pair in every row (it moves 3 N bytes where the pair moves 5 N).
Recorded, not required: the ratios to the plain parents and to the copy.

Every fused result is checked once against its unfused pair.  Recipe: tools/benchkit.py, with the cache sweep.  Prints one
JSON document and writes it to --out."""
import argparse
import ctypes as C
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

STEP = 1e-3
CALLS = ("hist", "split", "merge", "merge_range", "compress", "decode")


def make_pair(torch, synth, kind, n_bytes, e, seed):
    """(new, base): n_bytes each"""
    if kind == "uniform":
        return (synth.make(torch, "uniform", n_bytes, seed=seed, offset=0, device="cuda"),
                synth.make(torch, "uniform", n_bytes, seed=seed + 1, offset=0, device="cuda"))
    return benchkit.normal_pair(torch, n_bytes, e, STEP, seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    ap.add_argument("--widths", default="2,4,8")
    ap.add_argument("--kinds", default="normal,uniform")
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "delta_bench.json"))
    args = ap.parse_args()

    import importlib

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "planes_delta_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "step": STEP, "cache_sweep": benchkit.CACHE_SWEEP,
                "unfused": "torch.bitwise_xor(out = preallocated) + the plain call", "merge_range_first": 5,
                "required": ["fused < unfused for every call in every row"], "runs": []})
    ok = benchkit.ok
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    for mib in [int(x) for x in args.mib.split(",")]:
        nbytes = mib << 20
        for e in [int(x) for x in args.widths.split(",")]:
            n = nbytes // e
            first = res["merge_range_first"]
            count = n - 16
            for kind in args.kinds.split(","):
                d_new, d_base = make_pair(torch, synth, kind, nbytes, e, args.seed)
                p, b = d_new.data_ptr(), d_base.data_ptr()
                stride = (n + 255) & ~255
                d_xor = ctx.empty_u8(nbytes)      # the scratch of the unfused pairs
                d_planes = ctx.empty_u8(stride * e)
                d_planes2 = ctx.empty_u8(stride * e)
                d_out = ctx.empty_u8(nbytes)
                d_out2 = ctx.empty_u8(nbytes)
                h_f = torch.zeros((e, ghf.NSYM), dtype=torch.int64, device="cuda")
                h_u = torch.zeros((e, ghf.NSYM), dtype=torch.int64, device="cuda")
                x, pl, pl2, o, o2 = d_xor.data_ptr(), d_planes.data_ptr(), d_planes2.data_ptr(), d_out.data_ptr(), d_out2.data_ptr()

                def xor_in():
                    torch.bitwise_xor(d_new, d_base, out=d_xor)

                V = {}
                V["hist"] = {
                    "fused": lambda: ok(L.ghf_histogram_planes_delta(ctx.h, p, b, n, e, 0, h_f.data_ptr())),
                    "unfused": lambda: (xor_in(), ok(L.ghf_histogram_planes(ctx.h, x, n, e, 0, h_u.data_ptr()))),
                    "plain": lambda: ok(L.ghf_histogram_planes(ctx.h, p, n, e, 0, h_u.data_ptr())),
                    "copy_nt": lambda: ok(L.ghf_copy_d2d(ctx.h, o, p, nbytes, 1)),
                }
                V["split"] = {
                    "fused": lambda: ok(L.ghf_planes_split_delta(ctx.h, p, b, n, e, pl, stride)),
                    "unfused": lambda: (xor_in(), ok(L.ghf_planes_split(ctx.h, x, n, e, pl2, stride))),
                    "plain": lambda: ok(L.ghf_planes_split(ctx.h, p, n, e, pl2, stride)),
                    "copy_nt": lambda: ok(L.ghf_copy_d2d(ctx.h, o, p, nbytes, 1)),
                }
                # the merges read d_planes = the planes of new ^ base, as the split above leaves them
                V["merge"] = {
                    "fused": lambda: ok(L.ghf_planes_merge_delta(ctx.h, pl, stride, b, n, e, o)),
                    "unfused": lambda: (ok(L.ghf_planes_merge(ctx.h, pl, stride, n, e, o2)), torch.bitwise_xor(d_out2, d_base, out=d_out2)),
                    "plain": lambda: ok(L.ghf_planes_merge(ctx.h, pl, stride, n, e, o2)),
                    "copy_nt": lambda: ok(L.ghf_copy_d2d(ctx.h, o2, p, nbytes, 1)),
                }
                cb = count * e
                V["merge_range"] = {
                    "fused": lambda: ok(L.ghf_planes_merge_range_delta(ctx.h, pl, stride, b, first, count, e, o)),
                    "unfused": lambda: (ok(L.ghf_planes_merge_range(ctx.h, pl, stride, first, count, e, o2)),
                                        torch.bitwise_xor(d_out2[:cb], d_base[:cb], out=d_out2[:cb])),
                    "plain": lambda: ok(L.ghf_planes_merge_range(ctx.h, pl, stride, first, count, e, o2)),
                    "copy_nt": lambda: ok(L.ghf_copy_d2d(ctx.h, o2, p, cb, 1)),
                }

                # checked once: every fused result is its unfused pair's
                V["hist"]["fused"]()
                V["hist"]["unfused"]()
                ctx.sync()
                assert torch.equal(h_f, h_u) and int(h_f[:, :256].sum().item()) == nbytes, (mib, e, kind)
                V["split"]["fused"]()
                V["split"]["unfused"]()
                ctx.sync()
                for q in range(e):
                    assert torch.equal(d_planes[q * stride :][:n], d_planes2[q * stride :][:n]), (mib, e, kind, q)
                V["merge"]["fused"]()
                V["merge"]["unfused"]()
                ctx.sync()
                assert torch.equal(d_out, d_out2) and torch.equal(d_out, d_new), (mib, e, kind)
                V["merge_range"]["fused"]()
                V["merge_range"]["unfused"]()
                ctx.sync()
                assert torch.equal(d_out[:cb], d_out2[:cb]), (mib, e, kind)
                # (the planes hold new ^ base; the range call takes whatever base the caller gives for the range: here base[0 ..))
                assert torch.equal(d_out[:cb], d_new[first * e :][:cb] ^ d_base[first * e :][:cb] ^ d_base[:cb]), (mib, e, kind)

                # the composed calls
                slot = ghf.planes_slot_bytes(n)
                idx, idx2 = ctx.planes_index_alloc(n, e), ctx.planes_index_alloc(n, e)
                r_f = ctx.compress_planes_delta(d_new, d_base, e, n_elems=n, indexes=idx)
                xor_in()
                r_u = ctx.compress_planes_coded(d_xor, e, n_elems=n, indexes=idx2)
                r_plain = ctx.compress_planes_coded(d_new, e, n_elems=n)
                ctx.sync()
                sizes = [int(v) for v in r_f["out_bytes"].cpu().tolist()]
                assert sizes == [int(v) for v in r_u["out_bytes"].cpu().tolist()] and torch.equal(r_f["codes"], r_u["codes"]), (mib, e, kind)
                for q in range(e):
                    assert torch.equal(r_f["out"][q * slot :][: sizes[q]], r_u["out"][q * slot :][: sizes[q]]), (mib, e, kind, q)
                sizes_plain = [int(v) for v in r_plain["out_bytes"].cpu().tolist()]
                sptrs = (C.c_void_p * e)(*[r_f["out"].data_ptr() + q * slot for q in range(e)])
                ssizes = (C.c_size_t * e)(*sizes)
                codes = r_f["codes"].data_ptr()
                V["compress"] = {
                    "fused": lambda: ok(L.ghf_compress_planes_delta(ctx.h, p, b, n, e, codes, ghf.PLANES_BUILD_CODES, r_f["out"].data_ptr(),
                                                                    slot, r_f["out_bytes"].data_ptr(), idx)),
                    "unfused": lambda: (xor_in(), ok(L.ghf_compress_planes_coded(ctx.h, x, n, e, r_u["codes"].data_ptr(), ghf.PLANES_BUILD_CODES,
                                                                                 r_u["out"].data_ptr(), slot, r_u["out_bytes"].data_ptr(), idx2))),
                }
                V["decode"] = {
                    "fused": lambda: ok(L.ghf_decode_planes_delta(ctx.h, sptrs, ssizes, codes, idx, b, n, e, o, nbytes, None)),
                    "unfused": lambda: (ok(L.ghf_decode_planes(ctx.h, sptrs, ssizes, codes, idx, n, e, o2, nbytes, None)),
                                        torch.bitwise_xor(d_out2, d_base, out=d_out2)),
                }
                d_out.zero_()
                d_out2.zero_()
                V["decode"]["fused"]()
                V["decode"]["unfused"]()
                ctx.sync()
                assert torch.equal(d_out, d_new) and torch.equal(d_out2, d_new), (mib, e, kind)

                med, lo, hi = {}, {}, {}
                for call in CALLS:
                    _, times = timed(V[call].items())
                    med[call], lo[call], hi[call] = benchkit.stats(times).values()
                ctx.planes_index_free(idx)
                ctx.planes_index_free(idx2)
                run = {
                    "mib": mib, "elem_bytes": e, "kind": kind, "n_elems": n, "median_ms": med, "min_ms": lo, "max_ms": hi,
                    "fused_over_unfused": {c: round(med[c]["fused"] / med[c]["unfused"], 4) for c in CALLS},
                    "fused_over_plain": {c: round(med[c]["fused"] / med[c]["plain"], 4) for c in CALLS if "plain" in med[c]},
                    "fused_over_copy_nt": {c: round(med[c]["fused"] / med[c]["copy_nt"], 4) for c in CALLS if "copy_nt" in med[c]},
                    # 3 N bytes move through a fused kernel call (2 N through the histogram)
                    "fused_tb_per_s": {c: round((2 if c == "hist" else 3) * nbytes / med[c]["fused"] / 1e9, 3)
                                       for c in ("hist", "split", "merge", "merge_range")},
                    "stored_bytes": {"delta_planes": sum(sizes), "planes_of_new": sum(sizes_plain),
                                     "ratio": round(sum(sizes) / sum(sizes_plain), 4)},
                }
                run["meets_required"] = all(med[c]["fused"] < med[c]["unfused"] for c in CALLS)
                res["runs"].append(run)
                benchkit.progress(run)
                del V, d_new, d_base, d_xor, d_planes, d_planes2, d_out, d_out2, r_f, r_u, r_plain
                torch.cuda.empty_cache()
    res["meets_required"] = all(r["meets_required"] for r in res["runs"])
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
