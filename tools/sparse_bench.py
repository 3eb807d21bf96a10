#!/usr/bin/env python3
"""What the zero-suppressed byte-plane calls cost, measured.  Not bench.py: this times the sparse
split / merge kernels and the plane calls built on them.  In one run:

  kernels     ghf_sparse_split and ghf_sparse_merge on byte strings of every size in `--mib` (256 and 1024) with 1 % non-zero
              bytes (the case the feature exists for) and on uniform bytes (255/256 non-zero: the compaction writes nearly
              everything, and the feature would not be chosen), beside ghf_copy_d2d(non_temporal = 1) of the same n bytes.
              Rates are counted on each call's own traffic over its three launches:
                split: 2 n read (count and move), n / 8 + n_vals written
                merge: the mask read twice (2 * n / 8), n_vals read, n written
                copy:  n read, n written
  end to end  ghf_compress_planes_sparse_delta(GHF_SPARSE_AUTO) and ghf_decode_planes_sparse_delta (side-cars) against
              ghf_compress_planes_delta(GHF_PLANES_BUILD_CODES) and ghf_decode_planes_delta (side-cars), `--e2e-mib` (256) of
              bf16 and fp32 pairs at steps 1e-3 and 1e-5 and of an identical pair; the stored bytes beside the times.  Both
              compress calls are timed without side-cars (the sparse call would allocate them inside the timed window).

REQUIRED: split and merge at 1 % non-zero reach at least 0.5 of the copy's rate at every size.
Recorded, not required: the uniform rows and everything end to end.

Every result is checked once.  Recipe: tools/benchkit.py, with the cache sweep.  Prints one JSON document and writes it to
--out."""
import argparse
import ctypes as C
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    ap.add_argument("--e2e-mib", type=int, default=256)
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "sparse_bench.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    assert torch.cuda.is_available(), "sparse_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "cache_sweep": benchkit.CACHE_SWEEP,
                "traffic": {"split": "2 n + n / 8 + n_vals", "merge": "2 * n / 8 + n_vals + n", "copy_nt": "2 n"},
                "required": ["split and merge at 1 % non-zero bytes: at least 0.5 of the rate of ghf_copy_d2d(non_temporal = 1)"],
                "kernels": [], "end_to_end": []})
    ok = benchkit.ok
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    # ---- the kernels
    for mib in [int(x) for x in args.mib.split(",")]:
        n = mib << 20
        mb = ghf.sparse_mask_bytes(n)
        # uniform: 255/256 non-zero; 1pct: one byte in a hundred non-zero
        for kind, make_bytes in (("1pct", benchkit.sparse_bytes_1pct), ("uniform", benchkit.uniform_bytes)):
            d_x = make_bytes(torch, n, args.seed)
            nv = int(torch.count_nonzero(d_x).item())
            d_mask, d_vals, d_out, d_copy = ctx.empty_u8(mb), ctx.empty_u8(nv), ctx.empty_u8(n), ctx.empty_u8(n)
            d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
            x, m, v, o, cp, cnt = d_x.data_ptr(), d_mask.data_ptr(), d_vals.data_ptr(), d_out.data_ptr(), d_copy.data_ptr(), d_count.data_ptr()
            V = [("split", lambda: ok(L.ghf_sparse_split(ctx.h, x, n, m, v, nv, cnt))),
                 ("merge", lambda: ok(L.ghf_sparse_merge(ctx.h, m, v, nv, n, o))),
                 ("copy_nt", lambda: ok(L.ghf_copy_d2d(ctx.h, cp, x, n, 1)))]
            d_out.zero_()
            V[0][1]()
            V[1][1]()
            ctx.sync()  # checked once: the count, the values and the round trip
            assert int(d_count.item()) == nv and torch.equal(d_vals[:nv], d_x[d_x != 0]) and torch.equal(d_out, d_x), (mib, kind)
            med, lo, hi = benchkit.stats(timed(V)[1]).values()
            traffic = {"split": 2 * n + mb + nv, "merge": 2 * mb + nv + n, "copy_nt": 2 * n}
            rate = {k: round(traffic[k] / med[k] / 1e9, 3) for k in med}  # bytes / ms / 1e9 = TB/s
            run = {"mib": mib, "kind": kind, "n": n, "n_vals": nv, "median_ms": med, "min_ms": lo, "max_ms": hi, "traffic_bytes": traffic,
                   "tb_per_s": rate, "rate_over_copy_nt": {k: round(rate[k] / rate["copy_nt"], 4) for k in ("split", "merge")}}
            if kind == "1pct":
                run["meets_required"] = all(r >= 0.5 for r in run["rate_over_copy_nt"].values())
            res["kernels"].append(run)
            benchkit.progress(run)
            del V, d_x, d_mask, d_vals, d_out, d_copy
            torch.cuda.empty_cache()

    # ---- end to end
    nbytes = args.e2e_mib << 20
    for e in (2, 4):
        n = nbytes // e
        for step in (1e-3, 1e-5, None):
            d_new, d_base = benchkit.normal_pair(torch, nbytes, e, step, args.seed)
            p, b = d_new.data_ptr(), d_base.data_ptr()
            slot = ghf.planes_slot_bytes(n)
            d_out, d_out2 = ctx.empty_u8(nbytes), ctx.empty_u8(nbytes)
            o, o2 = d_out.data_ptr(), d_out2.data_ptr()
            r_s = ctx.compress_planes_sparse_delta(d_new, d_base, e, n_elems=n, indexes=True)
            idx_d = ctx.planes_index_alloc(n, e)
            r_d = ctx.compress_planes_delta(d_new, d_base, e, n_elems=n, indexes=idx_d)
            ctx.sync()
            sizes_s = [int(v) for v in r_s["out_bytes"].cpu().tolist()]
            sizes_d = [int(v) for v in r_d["out_bytes"].cpu().tolist()]
            chosen, n_vals, idx_s = r_s["sparse_planes"], r_s["n_vals"], r_s["indexes"]
            sp_s = (C.c_void_p * (2 * e))(*[r_s["out"].data_ptr() + j * slot for j in range(2 * e)])
            ss_s = (C.c_size_t * (2 * e))(*sizes_s)
            nv_s = (C.c_size_t * e)(*n_vals)
            sp_d = (C.c_void_p * e)(*[r_d["out"].data_ptr() + j * slot for j in range(e)])
            ss_d = (C.c_size_t * e)(*sizes_d)
            h_chosen, h_nv = C.c_uint(0), (C.c_size_t * e)()
            V = [("compress_sparse", lambda: ok(L.ghf_compress_planes_sparse_delta(
                      ctx.h, p, b, n, e, ghf.SPARSE_AUTO, r_s["out"].data_ptr(), slot, r_s["out_bytes"].data_ptr(), r_s["codes"].data_ptr(),
                      None, C.byref(h_chosen), h_nv))),
                 ("compress_dense", lambda: ok(L.ghf_compress_planes_delta(
                      ctx.h, p, b, n, e, r_d["codes"].data_ptr(), ghf.PLANES_BUILD_CODES, r_d["out"].data_ptr(), slot,
                      r_d["out_bytes"].data_ptr(), None))),
                 ("decode_sparse", lambda: ok(L.ghf_decode_planes_sparse_delta(ctx.h, sp_s, ss_s, r_s["codes"].data_ptr(), idx_s, b, chosen,
                                                                               nv_s, n, e, o, nbytes, None))),
                 ("decode_dense", lambda: ok(L.ghf_decode_planes_delta(ctx.h, sp_d, ss_d, r_d["codes"].data_ptr(), idx_d, b, n, e, o2, nbytes,
                                                                       None)))]
            d_out.zero_()
            d_out2.zero_()
            V[2][1]()
            V[3][1]()
            ctx.sync()  # checked once: both decodes give the new tensor back
            assert torch.equal(d_out, d_new) and torch.equal(d_out2, d_new), (e, step)
            med, lo, hi = benchkit.stats(timed(V)[1]).values()
            assert h_chosen.value == chosen and list(h_nv) == n_vals
            run = {"mib": args.e2e_mib, "elem_bytes": e, "step": "identical" if step is None else step, "n_elems": n,
                   "sparse_planes": chosen, "n_vals": n_vals, "median_ms": med, "min_ms": lo, "max_ms": hi,
                   "stored_bytes": {"sparse": sum(sizes_s), "dense": sum(sizes_d), "ratio": round(sum(sizes_s) / sum(sizes_d), 4)},
                   "sparse_over_dense": {"compress": round(med["compress_sparse"] / med["compress_dense"], 4),
                                         "decode": round(med["decode_sparse"] / med["decode_dense"], 4)}}
            res["end_to_end"].append(run)
            benchkit.progress(run)
            ctx.planes_index_free(idx_s)
            ctx.planes_index_free(idx_d)
            del V, d_new, d_base, d_out, d_out2, r_s, r_d
            torch.cuda.empty_cache()
    res["meets_required"] = all(r["meets_required"] for r in res["kernels"] if "meets_required" in r)
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
