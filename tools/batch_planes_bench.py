#!/usr/bin/env python3
"""What one shared code PER BYTE PLANE costs and buys over one flat shared code, measured.  Not
bench.py: this times many small items.  `--mib` MiB of bf16 and fp32 standard-normal values and of uniform bytes (taken
as 2-byte elements), cut into items of 4 KiB and 64 KiB:

  h    ghf_histogram_batch + ghf_build_code                        hp   ghf_histogram_batch_planes + ghf_build_codes
  c    ghf_compress_batch_shared                                   cp   ghf_compress_batch_planes_shared
  d    ghf_decode_batch_shared                                     dp   ghf_decode_batch_planes_shared
  s    ghf_decode_bodies_batch_shared                              sp   ghf_decode_bodies_batch_planes_shared

The flat calls run on the same interleaved bytes in the same run; their code paths are the parent commit's, so their times
are also the check that templating their bodies cost nothing.  Reported per item (call time / items) with the stored
bytes per item of both forms (bodies plus the headers' share).  No time ratio is required; the sizes are: the planes form
must store strictly less than the flat form on the bf16 and fp32 inputs.  Every variant is checked against the input
first.  Recipe: tools/benchkit.py, with the cache sweep.  Both codes come from GHF_HIST_COVER_ALL histograms.  Prints one
JSON document; --out also writes it.  Exit status 1 when a required row fails."""
import argparse
import ctypes as C
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

KINDS = {"bf16_normal": 2, "fp32_normal": 4, "uniform_bytes": 2}
SEED = 7


def make(torch, kind, n):
    if kind == "bf16_normal":
        return benchkit.normal_bf16_rounded(torch, n, SEED)
    if kind == "fp32_normal":
        return benchkit.normal_fp(torch, n, 4, SEED)
    return benchkit.uniform_bytes(torch, n, SEED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--item-kib", default="4,64")
    ap.add_argument("--kinds", default=",".join(KINDS))
    benchkit.add_args(ap, reps=10, warmup=2, out=None)
    args = ap.parse_args()

    import torch

    import pkgload

    ghf = pkgload.load().ghf
    assert torch.cuda.is_available(), "batch_planes_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    n = args.mib << 20
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"mib": args.mib, "cache_sweep": benchkit.CACHE_SWEEP, "kinds": {}})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    def clean(*results):
        return all(int(r["status"].abs().sum().item()) == 0 for r in results)

    ok = True
    for kind in args.kinds.split(","):
        e = KINDS[kind]
        d_in = make(torch, kind, n)
        kres = {"elem_bytes": e, "items": {}}
        for kib in [int(x) for x in args.item_kib.split(",")]:
            item = kib << 10
            count = n // item
            sizes = [item] * count
            # the flat form: one code over the interleaved bytes
            fidx = ctx.batch_index_alloc(count, item)
            f_hist = ctx.histogram_batch(d_in, sizes=sizes, max_item_bytes=item, flags=ghf.HIST_COVER_ALL)
            f_code = ctx.build_code(f_hist)
            f = ctx.compress_batch_shared(d_in, f_code, sizes=sizes, max_item_bytes=item, index=fidx)
            fd = ctx.decode_batch_shared(f["out_ptrs"], f["out_bytes"], f_code, fidx, f["in_bytes"], out_stride=item)
            fs = ctx.decode_bodies_batch_shared(f["out_ptrs"], f["out_bytes"], f_code, out=ctx.empty_u8(n), caps=f["in_bytes"])
            ctx.sync()
            assert clean(f, fd, fs) and torch.equal(fd["out"][:n], d_in) and torch.equal(fs["out"][:n], d_in), (kind, kib)
            # the planes form: one code per byte plane
            pidx = ctx.batch_index_alloc(count * e, item // e)
            p_hists = ctx.histogram_batch_planes(d_in, e, sizes=sizes, max_item_bytes=item, flags=ghf.HIST_COVER_ALL)
            p_codes = ctx.build_codes(p_hists)
            p = ctx.compress_batch_planes_shared(d_in, p_codes, e, sizes=sizes, max_item_bytes=item, index=pidx)
            pd = ctx.decode_batch_planes_shared(p["out_ptrs"], p["out_bytes"], p_codes, pidx, p["n_elems"], e, out_stride=item)
            ps = ctx.decode_bodies_batch_planes_shared(p["out_ptrs"], p["out_bytes"], p_codes, e, out=ctx.empty_u8(n), caps=p["in_bytes"])
            ctx.sync()
            assert clean(p, pd, ps) and torch.equal(pd["out"][:n], d_in) and torch.equal(ps["out"][:n], d_in), (kind, kib)
            f_hdr = int(L.ghf_header_bytes(ctx.code_to_host(f_code).max_len))
            p_hdr = sum(int(L.ghf_header_bytes(ctx.code_to_host(p_codes[k]).max_len)) for k in range(e))

            call = benchkit.ok
            P = lambda t: t.data_ptr()
            variants = [
                ("h", lambda: (call(L.ghf_histogram_batch(ctx.h, P(f["in_ptrs"]), P(f["in_bytes"]), item, count, 1, P(f_hist))),
                               call(L.ghf_build_code(ctx.h, P(f_hist), P(f_code))))),
                ("hp", lambda: (call(L.ghf_histogram_batch_planes(ctx.h, P(p["in_ptrs"]), P(p["in_bytes"]), item, count, e, 1, P(p_hists))),
                                call(L.ghf_build_codes(ctx.h, P(p_hists), e, P(p_codes), 0)))),
                ("c", lambda: call(L.ghf_compress_batch_shared(ctx.h, P(f["in_ptrs"]), P(f["in_bytes"]), item, count, P(f_code), P(f["out_ptrs"]),
                                                               P(f["out_caps"]), P(f["out_bytes"]), C.byref(fidx), P(f["status"])))),
                ("cp", lambda: call(L.ghf_compress_batch_planes_shared(ctx.h, P(p["in_ptrs"]), P(p["in_bytes"]), item, count, e, P(p_codes),
                                                                       P(p["out_ptrs"]), P(p["out_caps"]), P(p["out_bytes"]), C.byref(pidx),
                                                                       P(p["status"])))),
                ("d", lambda: call(L.ghf_decode_batch_shared(ctx.h, P(f["out_ptrs"]), P(f["out_bytes"]), P(f_code), C.byref(fidx), P(f["in_bytes"]),
                                                             count, P(fd["out_ptrs"]), P(fd["out_caps"]), P(fd["out_bytes"]), P(fd["status"])))),
                ("dp", lambda: call(L.ghf_decode_batch_planes_shared(ctx.h, P(p["out_ptrs"]), P(p["out_bytes"]), P(p_codes), C.byref(pidx),
                                                                     P(p["n_elems"]), count, e, P(pd["out_ptrs"]), P(pd["out_caps"]),
                                                                     P(pd["out_bytes"]), P(pd["status"])))),
                ("s", lambda: call(L.ghf_decode_bodies_batch_shared(ctx.h, P(f["out_ptrs"]), P(f["out_bytes"]), P(f_code), count, P(fs["out_ptrs"]),
                                                                    P(fs["out_caps"]), P(fs["out_bytes"]), P(fs["status"])))),
                ("sp", lambda: call(L.ghf_decode_bodies_batch_planes_shared(ctx.h, P(p["out_ptrs"]), P(p["out_bytes"]), P(p_codes), count, e,
                                                                            P(ps["out_ptrs"]), P(ps["out_caps"]), P(ps["out_bytes"]),
                                                                            P(ps["status"])))),
            ]
            med, times = timed(variants)
            assert clean(f, fd, fs, p, pd, ps), (kind, kib)
            flat_bytes = float(f["out_bytes"].sum().item()) / count + f_hdr / count
            planes_bytes = float(p["out_bytes"].sum().item()) / count + p_hdr / count
            row = {
                "count": count,
                **benchkit.stats(times),
                "per_item_us": {x: round(1e3 * v / count, 4) for x, v in med.items()},
                "gb_per_s": {x: round(n / v / 1e6, 2) for x, v in med.items()},
                "stored_bytes_per_item": {"input": item, "flat": round(flat_bytes, 1), "planes": round(planes_bytes, 1),
                                          "planes_over_flat": round(planes_bytes / flat_bytes, 4), "flat_header_bytes": f_hdr,
                                          "planes_header_bytes": p_hdr},
                "ratios": {x + "p_over_" + x: round(med[x + "p"] / med[x], 4) for x in "hcds"},
            }
            if kind != "uniform_bytes":
                row["planes_store_less"] = planes_bytes < flat_bytes
                ok = ok and row["planes_store_less"]
            kres["items"]["%dKiB" % kib] = row
            benchkit.progress({kind: {"%dKiB" % kib: row}})
            ctx.batch_index_free(fidx)
            ctx.batch_index_free(pidx)
            del f, fd, fs, p, pd, ps
        res["kinds"][kind] = kres
        del d_in
    res["required_planes_store_less_on_typed_inputs"] = ok
    ctx.close()
    benchkit.write(res, args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
