#!/usr/bin/env python3
"""What raw byte planes cost and save, measured.  Not bench.py: this times the pointer kernels and the
calls that take planes in three forms.  In one run, for every size in `--mib` (256 and 1024) and for standard-normal bf16 /
fp32 / fp64 values and uniform bytes (as 2-byte elements):

  kernels     ghf_planes_split_to and ghf_planes_merge_from on the parents' own addresses (planes + p * stride) beside
              ghf_planes_split, ghf_planes_merge and ghf_copy_d2d(non_temporal = 1) of the same bytes.  Every one of them reads
              n bytes and writes n bytes, so the ratio of the rates is the inverse ratio of the times.
  end to end  ghf_compress_planes_forms(GHF_RAW_AUTO, 0) against ghf_compress_planes_coded(GHF_PLANES_BUILD_CODES), the indexed
              ghf_decode_planes_forms against ghf_decode_planes, and the middle eighth through ghf_decode_planes_forms_range
              against ghf_decode_planes_range (side-cars), on the same tensor; also the compress with the masks GHF_RAW_AUTO
              chose given explicitly, which never waits for the device.  The compress calls are timed without side-cars (the
              forms call would allocate them inside the timed window).  The stored bytes of both forms beside the times.

REQUIRED: split_to and merge_from reach at least 0.5 of the copy's rate in every row; on the three float inputs each new call
(compress, decode, range) takes less time than its dense counterpart.
Recorded, not required: the ratio of the pointer kernels to their parents, the uniform rows end to end, the no-wait compress.

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

INPUTS = (("bf16", 2, "normal"), ("fp32", 4, "normal"), ("fp64", 8, "normal"), ("uniform", 2, "uniform"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "forms_bench.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    assert torch.cuda.is_available(), "planes_forms_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "cache_sweep": benchkit.CACHE_SWEEP,
                "required": ["split_to and merge_from: at least 0.5 of the rate of ghf_copy_d2d(non_temporal = 1)",
                             "bf16 / fp32 / fp64: compress_forms < compress_coded, decode_forms < decode_planes, range_forms < range_planes"],
                "rows": []})
    ok = benchkit.ok
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    for mib in [int(x) for x in args.mib.split(",")]:
        nbytes = mib << 20
        for name, e, kind in INPUTS:
            n = nbytes // e
            d_x = benchkit.uniform_bytes(torch, nbytes, args.seed) if kind == "uniform" else benchkit.normal_elems(torch, nbytes, e, args.seed)
            x = d_x.data_ptr()

            # ---- the kernels, on the parents' own addresses
            stride = (n + 255) & ~255
            d_planes, d_back, d_copy = ctx.empty_u8(e * stride), ctx.empty_u8(nbytes), ctx.empty_u8(nbytes)
            pl, bk, cp = d_planes.data_ptr(), d_back.data_ptr(), d_copy.data_ptr()
            ptrs = (C.c_void_p * e)(*[pl + p * stride for p in range(e)])
            K = [("split_to", lambda: ok(L.ghf_planes_split_to(ctx.h, x, None, n, e, ptrs))),
                 ("split", lambda: ok(L.ghf_planes_split(ctx.h, x, n, e, pl, stride))),
                 ("merge_from", lambda: ok(L.ghf_planes_merge_from(ctx.h, ptrs, None, n, e, bk))),
                 ("merge", lambda: ok(L.ghf_planes_merge(ctx.h, pl, stride, n, e, bk))),
                 ("copy_nt", lambda: ok(L.ghf_copy_d2d(ctx.h, cp, x, nbytes, 1)))]
            d_planes.zero_()
            K[0][1]()
            ctx.sync()
            want_planes = d_planes.clone()
            d_planes.zero_()
            K[1][1]()
            K[2][1]()
            ctx.sync()  # checked once: split_to writes what the parent writes, merge_from gives the tensor back
            assert torch.equal(d_planes, want_planes) and torch.equal(d_back, d_x), (mib, name)
            del want_planes
            k_med, k_lo, k_hi = benchkit.stats(timed(K)[1]).values()
            del K, d_planes, d_back, d_copy
            torch.cuda.empty_cache()

            # ---- end to end
            slot = ghf.planes_slot_bytes(n)
            r_f = ctx.compress_planes_forms(d_x, e, raw_planes=ghf.RAW_AUTO, sparse_planes=0, n_elems=n, indexes=True)
            idx_d = ctx.planes_index_alloc(n, e)
            r_d = ctx.compress_planes_coded(d_x, e, flags=ghf.PLANES_BUILD_CODES, n_elems=n, indexes=idx_d)
            ctx.sync()
            sizes_f = [int(v) for v in r_f["out_bytes"].cpu().tolist()]
            sizes_d = [int(v) for v in r_d["out_bytes"].cpu().tolist()]
            raw, idx_f = r_f["raw_planes"], r_f["indexes"]
            assert r_f["sparse_planes"] == 0
            first, count = n // 2 - n // 16, n // 8  # the middle eighth
            d_out, d_out2 = ctx.empty_u8(nbytes), ctx.empty_u8(nbytes)
            d_part, d_part2 = ctx.empty_u8(count * e), ctx.empty_u8(count * e)
            o, o2, pt, pt2 = d_out.data_ptr(), d_out2.data_ptr(), d_part.data_ptr(), d_part2.data_ptr()
            sp_f = (C.c_void_p * (2 * e))(*[r_f["out"].data_ptr() + j * slot for j in range(2 * e)])
            ss_f = (C.c_size_t * (2 * e))(*sizes_f)
            nv_f = (C.c_size_t * e)(*r_f["n_vals"])
            sp_d = (C.c_void_p * e)(*[r_d["out"].data_ptr() + j * slot for j in range(e)])
            ss_d = (C.c_size_t * e)(*sizes_d)
            h_raw, h_sparse, h_nv = C.c_uint(0), C.c_uint(0), (C.c_size_t * e)()
            fo, fb, fc = r_f["out"].data_ptr(), r_f["out_bytes"].data_ptr(), r_f["codes"].data_ptr()

            def compress_forms(mask):
                return lambda: ok(L.ghf_compress_planes_forms(ctx.h, x, None, n, e, mask, 0, fo, slot, fb, fc, None, None, 0, C.byref(h_raw),
                                                              C.byref(h_sparse), h_nv))

            V = [("compress_forms", compress_forms(ghf.RAW_AUTO)),
                 ("compress_coded", lambda: ok(L.ghf_compress_planes_coded(ctx.h, x, n, e, r_d["codes"].data_ptr(), ghf.PLANES_BUILD_CODES,
                                                                           r_d["out"].data_ptr(), slot, r_d["out_bytes"].data_ptr(), None))),
                 ("compress_forms_explicit", compress_forms(raw)),
                 ("decode_forms", lambda: ok(L.ghf_decode_planes_forms(ctx.h, sp_f, ss_f, fc, idx_f, None, raw, 0, nv_f, n, e, o, nbytes, None))),
                 ("decode_planes", lambda: ok(L.ghf_decode_planes(ctx.h, sp_d, ss_d, r_d["codes"].data_ptr(), idx_d, n, e, o2, nbytes, None))),
                 ("range_forms", lambda: ok(L.ghf_decode_planes_forms_range(ctx.h, sp_f, ss_f, fc, idx_f, None, None, None, None, None, None, raw,
                                                                            0, n, e, first, count, pt, count * e))),
                 ("range_planes", lambda: ok(L.ghf_decode_planes_range(ctx.h, sp_d, ss_d, r_d["codes"].data_ptr(), idx_d, None, None, None, e,
                                                                       first, count, pt2, count * e)))]
            for t in (d_out, d_out2, d_part, d_part2):
                t.zero_()
            for i in (3, 4, 5, 6):
                V[i][1]()
            ctx.sync()  # checked once: both decodes give the tensor back, both ranges its middle eighth
            want_part = d_x[first * e : (first + count) * e]
            assert torch.equal(d_out, d_x) and torch.equal(d_out2, d_x), (mib, name)
            assert torch.equal(d_part, want_part) and torch.equal(d_part2, want_part), (mib, name)
            med, lo, hi = benchkit.stats(timed(V)[1]).values()
            assert h_raw.value == raw and h_sparse.value == 0
            med.update(k_med), lo.update(k_lo), hi.update(k_hi)
            row = {"mib": mib, "input": name, "elem_bytes": e, "n_elems": n, "raw_planes": raw, "median_ms": med, "min_ms": lo, "max_ms": hi,
                   "rate_over_copy_nt": {k: round(med["copy_nt"] / med[k], 4) for k in ("split_to", "merge_from", "split", "merge")},
                   "over_parent": {"split_to": round(med["split_to"] / med["split"], 4), "merge_from": round(med["merge_from"] / med["merge"], 4)},
                   "forms_over_dense": {"compress": round(med["compress_forms"] / med["compress_coded"], 4),
                                        "compress_explicit": round(med["compress_forms_explicit"] / med["compress_coded"], 4),
                                        "decode": round(med["decode_forms"] / med["decode_planes"], 4),
                                        "range": round(med["range_forms"] / med["range_planes"], 4)},
                   "stored_bytes": {"forms": sum(sizes_f), "dense": sum(sizes_d), "raw_tensor": nbytes,
                                    "ratio": round(sum(sizes_f) / sum(sizes_d), 4)}}
            row["meets_required_kernels"] = row["rate_over_copy_nt"]["split_to"] >= 0.5 and row["rate_over_copy_nt"]["merge_from"] >= 0.5
            if kind == "normal":
                row["meets_required_end_to_end"] = all(row["forms_over_dense"][k] < 1.0 for k in ("compress", "decode", "range"))
            res["rows"].append(row)
            benchkit.progress(row)
            ctx.planes_index_free(idx_f)
            ctx.planes_index_free(idx_d)
            del V, d_x, d_out, d_out2, d_part, d_part2, r_f, r_d
            torch.cuda.empty_cache()
    res["meets_required"] = all(r["meets_required_kernels"] and r.get("meets_required_end_to_end", True) for r in res["rows"])
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
