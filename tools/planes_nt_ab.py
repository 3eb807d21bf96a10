#!/usr/bin/env python3
"""A/B of the non-temporal hint in k_planes_split / k_planes_merge: the built library against
lib/libghf_planes_plain.so (`make -C golden-huffman_amd nt_ab`: the same objects with ghf_planes built with
-DGHF_PLANES_NT=0), alternating in one process at 256 MiB and 1 GiB for E = 2, 4, 8, on unseeded uniform bytes.  Recipe:
tools/benchkit.py, with the cache sweep.  Writes --out."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "nt_ab.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    ghf = pkgload.load().ghf
    plain = os.path.join(os.path.dirname(ghf.LIB_PATH), "libghf_planes_plain.so")
    if not os.path.exists(plain):
        subprocess.run(["make", "-s", "-C", os.path.dirname(os.path.dirname(ghf.LIB_PATH)), "nt_ab"], check=True)
    assert torch.cuda.is_available(), "planes_nt_ab needs the GPU: there is nothing to fall back to"
    LA, LB = ghf.lib(), C.CDLL(plain)
    vp, sz = C.c_void_p, C.c_size_t
    LB.ghf_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    LB.ghf_ctx_set_stream.argtypes = [vp, vp]
    LB.ghf_ctx_destroy.argtypes = [vp]
    LB.ghf_planes_split.argtypes = [vp, vp, sz, C.c_uint32, vp, sz]
    LB.ghf_planes_merge.argtypes = [vp, vp, sz, sz, C.c_uint32, vp]
    ctx = ghf.Context(0)
    hb = vp()
    assert LB.ghf_ctx_create(0, C.byref(hb)) == 0
    assert LB.ghf_ctx_set_stream(hb, vp(torch.cuda.current_stream().cuda_stream)) == 0
    sweep = benchkit.cache_sweep(ctx)
    # (no "lib" field: two libraries run here)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "unit": "ms (device events), medians",
           "cache_sweep": benchkit.CACHE_SWEEP, "runs": []}
    for mib in [int(x) for x in args.mib.split(",")]:
        nbytes = mib << 20
        d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        d_pl, d_out = torch.empty_like(d_in), torch.empty_like(d_in)
        for e in (2, 4, 8):
            n = nbytes // e
            variants = []
            for name, L, h in (("nt", LA, ctx.h), ("plain", LB, hb)):
                variants.append((name + "_split", lambda L=L, h=h: benchkit.ok(L.ghf_planes_split(h, d_in.data_ptr(), n, e, d_pl.data_ptr(), n))))
                variants.append((name + "_merge", lambda L=L, h=h: benchkit.ok(L.ghf_planes_merge(h, d_pl.data_ptr(), n, n, e, d_out.data_ptr()))))
            d_out.zero_()
            med, times = benchkit.timed(variants, args.reps, args.warmup, torch.cuda.synchronize, sweep)
            assert torch.equal(d_out, d_in), (mib, e)  # (behind the loop's closing sync: the last merge gave the input back)
            row = {"mib": mib, "elem_bytes": e, "median_ms": benchkit.stats(times)["median_ms"],
                   "plain_over_nt": {"split": round(med["plain_split"] / med["nt_split"], 3),
                                     "merge": round(med["plain_merge"] / med["nt_merge"], 3)}}
            res["runs"].append(row)
            benchkit.progress(row)
    LB.ghf_ctx_destroy(hb)
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
