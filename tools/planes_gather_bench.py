#!/usr/bin/env python3
"""What a lookup of many rows of a byte-plane compressed tensor costs, measured.  Not bench.py: this
times typed elements.  256 MiB of seeded standard-normal values per type (bf16 = the upper half of fp32, and fp32), stored
by ghf_compress_planes_forms with GHF_RAW_AUTO; the seek tables of the dense planes through the host and back; random row
indices on the device.  For 64, 1024 and 16384 rows of 4096 elements and 1024 rows of 128 elements it times

  gather        ghf_decode_planes_gather: one launch
  range_loop    one ghf_decode_planes_forms_range from the tables per row, the only way there was
  whole_select  ghf_decode_planes_forms of the whole tensor (live side-cars) followed by torch.index_select

REQUIRED: at 1024 rows of 4096 elements the gather takes less time than the per-row loop in the same run, for both types.
Recorded, not required: the gather against whole decode + index_select, the row count at which the two cross (between
the measured row counts that bracket it), and the output rate in GB/s.

Every variant is checked once against index_select of the input.  Recipe: tools/benchkit.py, with the cache sweep.  Prints
one JSON document and writes it to --out."""
import argparse
import ctypes as C
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

CASES = [(64, 4096), (1024, 4096), (16384, 4096), (1024, 128)]  # (rows, elements per row)
REQUIRED = (1024, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--widths", default="2,4")
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "gather_bench.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    assert torch.cuda.is_available(), "planes_gather_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "data": "standard-normal, GHF_RAW_AUTO", "cache_sweep": benchkit.CACHE_SWEEP,
                "required": "gather < range_loop at %d rows of %d" % REQUIRED, "runs": []})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    nbytes = args.mib << 20
    for e in [int(x) for x in args.widths.split(",")]:
        n = nbytes // e
        d_in = benchkit.normal_elems(torch, nbytes, e, args.seed)
        r = ctx.compress_planes_forms(d_in, e, raw_planes=ghf.RAW_AUTO, sparse_planes=0, indexes=True)
        ctx.sync()
        raw = r["raw_planes"]
        slots = 2 * e
        sizes = [int(v) for v in r["out_bytes"].cpu().tolist()]
        ptrs = (C.c_void_p * slots)(*[r["out"].data_ptr() + j * r["slot_bytes"] for j in range(slots)])
        szs = (C.c_size_t * slots)(*sizes)
        infos, tptrs, tbytes, d_tables = (ghf.SeekInfo * slots)(), (C.c_void_p * slots)(), (C.c_size_t * slots)(), []
        for p in range(e):
            if raw >> p & 1:
                continue
            d_t = ctx.seek_pack(r["indexes"][p])
            ctx.sync()
            h_t = d_t.cpu().numpy().copy()
            infos[p] = ghf.seek_parse(h_t)
            d_tables.append(torch.from_numpy(h_t).cuda())
            tptrs[p], tbytes[p] = d_tables[-1].data_ptr(), h_t.size
        n_vals = (C.c_size_t * e)()
        d_whole = ctx.empty_u8(nbytes)
        d_nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
        codes = r["codes"]
        run = {"mib": args.mib, "elem_bytes": e, "n_elems": n, "raw_planes": raw, "stored_bytes": sum(sizes), "cases": []}

        for n_rows, row_elems in CASES:
            row_bytes = row_elems * e
            g = torch.Generator(device="cuda")
            g.manual_seed(args.seed + n_rows + row_elems)
            d_index = torch.randint(0, n // row_elems, (n_rows,), generator=g, device="cuda", dtype=torch.int64)
            h_index = [int(v) for v in d_index.cpu().tolist()]
            d_out = ctx.empty_u8(n_rows * row_bytes)
            d_status = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
            want = torch.index_select(d_in.view(-1, row_bytes), 0, d_index).view(-1)
            sel = [None]

            def v_gather():
                assert L.ghf_decode_planes_gather(ctx.h, ptrs, szs, codes.data_ptr(), infos, tptrs, tbytes, raw, n, e, d_index.data_ptr(),
                                                  row_elems, row_elems, n_rows, d_out.data_ptr(), row_bytes, d_status.data_ptr()) == 0

            def v_loop():
                for k, i in enumerate(h_index):
                    assert L.ghf_decode_planes_forms_range(ctx.h, ptrs, szs, codes.data_ptr(), None, infos, tptrs, tbytes, None, None, None,
                                                           raw, 0, n, e, i * row_elems, row_elems, d_out.data_ptr() + k * row_bytes,
                                                           row_bytes) == 0

            def v_whole():
                assert L.ghf_decode_planes_forms(ctx.h, ptrs, szs, codes.data_ptr(), r["indexes"], None, raw, 0, n_vals, n, e,
                                                 d_whole.data_ptr(), nbytes, d_nbytes.data_ptr()) == 0
                sel[0] = torch.index_select(d_whole.view(-1, row_bytes), 0, d_index)

            for name, fn in (("gather", v_gather), ("range_loop", v_loop)):
                d_out.zero_()
                fn()
                ctx.sync()
                assert torch.equal(d_out, want), (e, n_rows, row_elems, name)
            assert int(d_status.abs().sum().item()) == 0
            v_whole()
            ctx.sync()
            assert torch.equal(sel[0].view(-1), want), (e, n_rows, row_elems, "whole_select")
            med, times = timed([("gather", v_gather), ("range_loop", v_loop), ("whole_select", v_whole)])
            case = {"rows": n_rows, "row_elems": row_elems, "out_bytes": n_rows * row_bytes,
                    **benchkit.stats(times),
                    "loop_over_gather": round(med["range_loop"] / med["gather"], 2),
                    "whole_select_over_gather": round(med["whole_select"] / med["gather"], 3),
                    "gather_gb_per_s": round(n_rows * row_bytes / med["gather"] / 1e6, 3)}
            if (n_rows, row_elems) == REQUIRED:
                case["meets_required"] = med["gather"] < med["range_loop"]
            run["cases"].append(case)
            benchkit.progress(case)
            del d_out, want, d_index
        # where the gather stops being faster than whole decode + index_select: between the two measured row counts of 4096
        # elements that bracket it, both times taken as straight lines in the row count (null: no crossing in the measured span)
        rows4096 = sorted((c for c in run["cases"] if c["row_elems"] == 4096), key=lambda c: c["rows"])
        run["crossover_rows_of_4096"] = None
        for a, b in zip(rows4096, rows4096[1:]):
            da = a["median_ms"]["gather"] - a["median_ms"]["whole_select"]
            db = b["median_ms"]["gather"] - b["median_ms"]["whole_select"]
            if da < 0 <= db:
                run["crossover_rows_of_4096"] = int(a["rows"] + (b["rows"] - a["rows"]) * (-da) / (db - da))
        res["runs"].append(run)
        ctx.planes_index_free(r["indexes"])
        del d_in, d_whole, r, d_tables
        torch.cuda.empty_cache()
    res["meets_required"] = all(c.get("meets_required", True) for run in res["runs"] for c in run["cases"])
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
