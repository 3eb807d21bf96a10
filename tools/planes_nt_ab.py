#!/usr/bin/env python3
"""A/B of the non-temporal hint in k_planes_split / k_planes_merge: the built library against
lib/libghf_planes_plain.so (`make -C golden-huffman_amd nt_ab`: the same objects with ghf_planes built with
-DGHF_PLANES_NT=0), alternating in one process at 256 MiB and 1 GiB for E = 2, 4, 8.  Device events, medians; in front of
every timed call, outside its events, a plain 256 MiB copy sweeps the Infinity Cache.  Writes --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes", "nt_ab.json"))
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
    flush_src = torch.zeros(256 << 20, dtype=torch.uint8, device="cuda")
    flush_dst = torch.empty_like(flush_src)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "unit": "ms (device events), medians",
           "cache_sweep": "plain 256 MiB copy in front of every timed call", "runs": []}
    for mib in [int(x) for x in args.mib.split(",")]:
        nbytes = mib << 20
        d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        d_pl, d_out = torch.empty_like(d_in), torch.empty_like(d_in)
        for e in (2, 4, 8):
            n = nbytes // e
            variants = []
            for name, L, h in (("nt", LA, ctx.h), ("plain", LB, hb)):
                variants.append((name + "_split", lambda L=L, h=h: L.ghf_planes_split(h, d_in.data_ptr(), n, e, d_pl.data_ptr(), n)))
                variants.append((name + "_merge", lambda L=L, h=h: L.ghf_planes_merge(h, d_pl.data_ptr(), n, n, e, d_out.data_ptr())))
            for _ in range(args.warmup):
                for _, fn in variants:
                    assert fn() == 0
            torch.cuda.synchronize()
            assert torch.equal(d_out, d_in), (mib, e)
            times = {k: [] for k, _ in variants}
            for _ in range(args.reps):
                for k, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    assert LA.ghf_copy_d2d(ctx.h, flush_dst.data_ptr(), flush_src.data_ptr(), flush_src.numel(), 0) == 0
                    e0.record()
                    assert fn() == 0
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1))
            med = {k: statistics.median(v) for k, v in times.items()}
            row = {"mib": mib, "elem_bytes": e, "median_ms": {k: round(v, 4) for k, v in med.items()},
                   "plain_over_nt": {"split": round(med["plain_split"] / med["nt_split"], 3),
                                     "merge": round(med["plain_merge"] / med["nt_merge"], 3)}}
            res["runs"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    LB.ghf_ctx_destroy(hb)
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
