#!/usr/bin/env python3
"""What an element range of a byte-plane compressed tensor costs, measured.  Not bench.py: this
times typed elements.  For every size in `--mib` (256 and 1024) and every element width in `--widths` (2, 4, 8), on seeded
standard-normal values (bf16 = the upper half of fp32, fp32, fp64):

  a  ghf_planes_merge_range of the whole buffer at skews 0, 5 and 15, against ghf_planes_merge and
     ghf_copy_d2d(non_temporal = 1) of the same byte count
  b  ghf_decode_planes_range of (0, n) from the side-cars, against ghf_decode_planes with the same side-cars
  c  the middle eighth at skew 0 and at skew 5, and a range of 1 MiB of output, from side-cars and from seek tables
  d  what the call replaces: ghf_decode_range per plane into 16-byte aligned planes (the byte path of the decoder at
     skew 5) followed by ghf_planes_merge, for the skew-5 eighth

Every variant is checked once against the input's slice.  Recipe: tools/benchkit.py, with the cache sweep.  Prints one JSON
document and writes it to --out."""
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
    ap.add_argument("--widths", default="2,4,8")
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "range_bench.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    assert torch.cuda.is_available(), "planes_range_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "data": "standard-normal", "cache_sweep": benchkit.CACHE_SWEEP, "required_fraction_of_copy": 0.5,
                "runs": []})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    for mib in [int(x) for x in args.mib.split(",")]:
        nbytes = mib << 20
        for e in [int(x) for x in args.widths.split(",")]:
            n = nbytes // e
            d_in = benchkit.normal_elems(torch, nbytes, e, args.seed)
            d_back = ctx.empty_u8(nbytes)
            d_copy = ctx.empty_u8(nbytes)

            # a: the merge alone.  The planes hold 16 elements more than the output so that every skew moves n elements.
            stride = (n + 16 + 255) & ~255
            d_planes = ctx.empty_u8(stride * e)
            m = n - 16  # elements moved by every merge variant
            ctx.planes_split(d_in, e, n_elems=n, d_planes=d_planes, plane_stride=stride)
            ctx.sync()

            def v_copy():
                assert L.ghf_copy_d2d(ctx.h, d_copy.data_ptr(), d_in.data_ptr(), m * e, 1) == 0

            def v_merge():
                assert L.ghf_planes_merge(ctx.h, d_planes.data_ptr(), stride, m, e, d_back.data_ptr()) == 0

            def v_merge_range(s):
                def fn():
                    assert L.ghf_planes_merge_range(ctx.h, d_planes.data_ptr(), stride, s, m, e, d_back.data_ptr()) == 0
                return fn

            for s in (0, 5, 15):
                d_back.zero_()
                v_merge_range(s)()
                ctx.sync()
                assert torch.equal(d_back[: m * e], d_in[s * e : (s + m) * e]), (mib, e, s)
            med_a, times_a = timed([("copy_nt", v_copy), ("merge", v_merge)] +
                                   [("merge_range_s%d" % s, v_merge_range(s)) for s in (0, 5, 15)])
            del d_copy

            # b, c, d: the codec.  Side-cars from the compression, seek tables through the host and back.
            idx = ctx.planes_index_alloc(n, e)
            r = ctx.compress_planes(d_in, e, n_elems=n, indexes=idx)
            ctx.sync()
            sizes = [int(v) for v in r["out_bytes"].cpu().tolist()]
            slot = r["slot_bytes"]
            codes = r["codes"]
            ptrs = (C.c_void_p * e)(*[r["out"].data_ptr() + p * slot for p in range(e)])
            szs = (C.c_size_t * e)(*sizes)
            h_tables = []
            for p in range(e):
                d_t = ctx.seek_pack(idx[p])
                ctx.sync()
                h_tables.append(d_t.cpu().numpy().copy())
            infos = (ghf.SeekInfo * e)(*[ghf.seek_parse(t) for t in h_tables])
            d_tables = [torch.from_numpy(t).cuda() for t in h_tables]
            tptrs = (C.c_void_p * e)(*[t.data_ptr() for t in d_tables])
            tbytes = (C.c_size_t * e)(*[t.size for t in h_tables])
            code_bytes = C.sizeof(ghf.Code)

            def v_whole_planes():
                assert L.ghf_decode_planes(ctx.h, ptrs, szs, codes.data_ptr(), idx, n, e, d_back.data_ptr(), nbytes, None) == 0

            def v_range(first, count, by_table):
                def fn():
                    assert L.ghf_decode_planes_range(ctx.h, ptrs, szs, codes.data_ptr(), None if by_table else idx,
                                                     infos if by_table else None, tptrs if by_table else None,
                                                     tbytes if by_table else None, e, first, count, d_back.data_ptr(), nbytes) == 0
                return fn

            def v_alternative(first, count, by_table):
                """per-plane ghf_decode_range into aligned planes, then ghf_planes_merge"""
                st = (count + 255) & ~255

                def fn():
                    for p in range(e):
                        assert L.ghf_decode_range(ctx.h, ptrs[p], szs[p], codes.data_ptr() + p * code_bytes,
                                                  None if by_table else C.byref(idx[p]), C.byref(infos[p]) if by_table else None,
                                                  tptrs[p] if by_table else None, tbytes[p] if by_table else 0, first, count,
                                                  d_planes.data_ptr() + p * st, st) == 0
                    assert L.ghf_planes_merge(ctx.h, d_planes.data_ptr(), st, count, e, d_back.data_ptr()) == 0
                return fn

            eighth = n // 8
            mid = ((7 * n // 16) & ~4095) + 1008  # a multiple of 16 that is no block edge
            small = (1 << 20) // e
            ranges = {"eighth_s0": (mid, eighth), "eighth_s5": (mid + 5, eighth), "mib1_s5": (n // 2 + 5, small)}
            variants = [("decode_planes", v_whole_planes), ("range_whole_idx", v_range(0, n, False))]
            for name, (first, count) in ranges.items():
                variants += [("range_%s_idx" % name, v_range(first, count, False)), ("range_%s_tab" % name, v_range(first, count, True))]
            f5, c5 = ranges["eighth_s5"]
            variants += [("alt_eighth_s5_idx", v_alternative(f5, c5, False)), ("alt_eighth_s5_tab", v_alternative(f5, c5, True))]
            where = {"decode_planes": (0, n), "range_whole_idx": (0, n), "alt_eighth_s5_idx": (f5, c5), "alt_eighth_s5_tab": (f5, c5)}
            for name, (first, count) in ranges.items():
                where["range_%s_idx" % name] = where["range_%s_tab" % name] = (first, count)
            for name, fn in variants:  # every variant gives the input's slice
                first, count = where[name]
                d_back[: count * e].zero_()
                fn()
                ctx.sync()
                assert torch.equal(d_back[: count * e], d_in[first * e : (first + count) * e]), (mib, e, name)
            med_b, times_b = timed(variants)

            med = dict(med_a, **med_b)
            times = dict(times_a, **times_b)
            whole = med["decode_planes"]
            spread = max(times["decode_planes"]) / min(times["decode_planes"])
            parts = [k for k in med_b if k.startswith("range_") and k != "range_whole_idx"]
            run = {
                "mib": mib, "elem_bytes": e, "n_elems": n, "merge_elems": m, "ranges": {k: list(v) for k, v in ranges.items()},
                **benchkit.stats(times),
                "tb_per_s": {k: round(2 * m * e / med[k] / 1e9, 3) for k in med_a},  # read + write
                "fraction_of_copy": {k: round(med["copy_nt"] / med[k], 4) for k in med_a if k != "copy_nt"},
                "whole_range_over_decode_planes": round(med["range_whole_idx"] / whole, 4),
                "decode_planes_max_over_min": round(spread, 4),
                "range_over_decode_planes": {k: round(med[k] / whole, 4) for k in parts},
                "eighth_s5_over_alternative": {s: round(med["range_eighth_s5_" + s] / med["alt_eighth_s5_" + s], 4) for s in ("idx", "tab")},
            }
            run["meets_a"] = min(v for k, v in run["fraction_of_copy"].items() if k.startswith("merge_range")) >= res["required_fraction_of_copy"]
            run["meets_b"] = run["whole_range_over_decode_planes"] <= run["decode_planes_max_over_min"]
            run["meets_c"] = all(med[k] < whole for k in parts) and all(v < 1 for v in run["eighth_s5_over_alternative"].values())
            res["runs"].append(run)
            benchkit.progress(run)
            ctx.planes_index_free(idx)
            del d_in, d_planes, d_back, r, d_tables
            torch.cuda.empty_cache()
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
