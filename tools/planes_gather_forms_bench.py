#!/usr/bin/env python3
"""What a lookup of many rows costs when the tensor is stored sparse and against a base, measured.
Not bench.py: this times typed elements.  Per type (bf16 = the upper half of fp32, and fp32) and per step (1e-3, 1e-5):
256 MiB of seeded standard-normal values (the base) against the same values after the step (new), stored by
ghf_compress_planes_forms(d_base, GHF_RAW_AUTO, GHF_SPARSE_AUTO, d_ranks); seek tables through the host and back; the rank
tables on the host for the range calls and as device images for the gather; random row ids on the device.  For 64, 1024 and
16384 rows of 4096 elements and 1024 rows of 128 elements it times

  forms_gather    ghf_decode_planes_gather_forms: one launch
  range_loop      one ghf_decode_planes_forms_range from the tables per row, the only way there was (not at 16384 rows: the
                  loop's time is its per-call floor times the rows, and 16384 calls per repeat buy no further knowledge)
  whole_select    ghf_decode_planes_forms of the whole tensor (live side-cars) followed by torch.index_select
  self_gather     ghf_decode_planes_gather on `new` stored by itself (dense / raw, no base): what the rank walk and the XOR cost
  plain_forms     ghf_decode_planes_gather_forms with sparse_planes == 0 and no base on that same storage: against self_gather,
                  what the new kernel costs where the parent serves

REQUIRED: in every row of the table, 1024 rows of 4096 elements through forms_gather take less time than range_loop in the
same run.  Everything else is recorded.  Every variant is checked once against index_select of `new`.

Recipe: tools/benchkit.py, with the cache sweep.  Prints one JSON document and writes it to --out."""
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
LOOP_MAX_ROWS = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--widths", default="2,4")
    ap.add_argument("--steps", default="1e-3,1e-5")
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "gather_forms_bench.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    assert torch.cuda.is_available(), "planes_gather_forms_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "data": "standard-normal against itself after a step; GHF_RAW_AUTO | GHF_SPARSE_AUTO against the base",
                "cache_sweep": benchkit.CACHE_SWEEP, "required": "forms_gather < range_loop at %d rows of %d, in every run" % REQUIRED,
                "runs": []})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    def stored(r, e):
        """the arrays of a compress_planes_forms result as the decode calls take them; seek tables through the host and back"""
        slots = 2 * e
        sizes = [int(v) for v in r["out_bytes"].cpu().tolist()]
        ptrs = (C.c_void_p * slots)(*[r["out"].data_ptr() + j * r["slot_bytes"] if sizes[j] else None for j in range(slots)])
        szs = (C.c_size_t * slots)(*sizes)
        infos, tptrs, tbytes, keep = (ghf.SeekInfo * slots)(), (C.c_void_p * slots)(), (C.c_size_t * slots)(), []
        for j in range(slots):
            if not sizes[j] or r["raw_planes"] >> (j % e) & 1:
                continue
            d_t = ctx.seek_pack(r["indexes"][j])
            ctx.sync()
            h_t = d_t.cpu().numpy().copy()
            infos[j] = ghf.seek_parse(h_t)
            keep.append(torch.from_numpy(h_t).cuda())
            tptrs[j], tbytes[j] = keep[-1].data_ptr(), h_t.size
        return sizes, ptrs, szs, infos, tptrs, tbytes, keep

    nbytes = args.mib << 20
    for e in [int(x) for x in args.widths.split(",")]:
        for step in [float(x) for x in args.steps.split(",")]:
            n = nbytes // e
            d_new, d_base = benchkit.normal_pair_reseeded(torch, nbytes, e, step, args.seed)
            r = ctx.compress_planes_forms(d_new, e, raw_planes=ghf.RAW_AUTO, sparse_planes=ghf.SPARSE_AUTO, d_base=d_base, indexes=True,
                                          ranks=True)
            ctx.sync()
            raw, sparse = r["raw_planes"], r["sparse_planes"]
            sizes, ptrs, szs, infos, tptrs, tbytes, keep = stored(r, e)
            n_vals = (C.c_size_t * e)(*r["n_vals"])
            rbytes = ghf.sparse_rank_bytes(n)
            h_ranks = r["ranks"].cpu().numpy()
            rank_tables = [h_ranks[p * r["rank_slot_bytes"] :][:rbytes].copy() for p in range(e)]
            r_infos, r_host, r_dev, r_sizes = (ghf.SparseRankInfo * e)(), (C.c_void_p * e)(), (C.c_void_p * e)(), (C.c_size_t * e)()
            for p in range(e):
                if sparse >> p & 1:
                    r_infos[p] = ghf.sparse_rank_parse(rank_tables[p])
                    r_host[p] = rank_tables[p].ctypes.data
                    r_dev[p], r_sizes[p] = r["ranks"].data_ptr() + p * r["rank_slot_bytes"], rbytes
            codes = r["codes"]
            # `new` stored by itself: what ghf_decode_planes_gather serves
            rs = ctx.compress_planes_forms(d_new, e, raw_planes=ghf.RAW_AUTO, sparse_planes=0, indexes=True)
            ctx.sync()
            s_raw = rs["raw_planes"]
            s_sizes, s_ptrs, s_szs, s_infos, s_tptrs, s_tbytes, s_keep = stored(rs, e)
            d_whole = ctx.empty_u8(nbytes)
            d_nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
            run = {"mib": args.mib, "elem_bytes": e, "step": step, "n_elems": n, "raw_planes": raw, "sparse_planes": sparse,
                   "n_vals": list(r["n_vals"]), "stored_bytes": {"forms_against_base": sum(sizes), "self_dense_raw": sum(s_sizes),
                                                                 "plain": nbytes}, "cases": []}

            for n_rows, row_elems in CASES:
                row_bytes = row_elems * e
                g = torch.Generator(device="cuda")
                g.manual_seed(args.seed + n_rows + row_elems)
                d_index = torch.randint(0, n // row_elems, (n_rows,), generator=g, device="cuda", dtype=torch.int64)
                h_index = [int(v) for v in d_index.cpu().tolist()]
                d_out = ctx.empty_u8(n_rows * row_bytes)
                d_status = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
                want = torch.index_select(d_new.view(-1, row_bytes), 0, d_index).view(-1)
                sel = [None]

                def v_forms():
                    assert L.ghf_decode_planes_gather_forms(ctx.h, ptrs, szs, codes.data_ptr(), infos, tptrs, tbytes, r_infos, r_dev, r_sizes,
                                                            d_base.data_ptr(), raw, sparse, n, e, d_index.data_ptr(), row_elems, row_elems,
                                                            n_rows, d_out.data_ptr(), row_bytes, d_status.data_ptr()) == 0

                def v_loop():
                    for k, i in enumerate(h_index):
                        assert L.ghf_decode_planes_forms_range(ctx.h, ptrs, szs, codes.data_ptr(), None, infos, tptrs, tbytes, r_infos, r_host,
                                                               d_base.data_ptr() + i * row_bytes, raw, sparse, n, e, i * row_elems, row_elems,
                                                               d_out.data_ptr() + k * row_bytes, row_bytes) == 0

                def v_whole():
                    assert L.ghf_decode_planes_forms(ctx.h, ptrs, szs, codes.data_ptr(), r["indexes"], d_base.data_ptr(), raw, sparse, n_vals,
                                                     n, e, d_whole.data_ptr(), nbytes, d_nbytes.data_ptr()) == 0
                    sel[0] = torch.index_select(d_whole.view(-1, row_bytes), 0, d_index)

                def v_self():
                    assert L.ghf_decode_planes_gather(ctx.h, s_ptrs, s_szs, rs["codes"].data_ptr(), s_infos, s_tptrs, s_tbytes, s_raw, n, e,
                                                      d_index.data_ptr(), row_elems, row_elems, n_rows, d_out.data_ptr(), row_bytes,
                                                      d_status.data_ptr()) == 0

                def v_plain():
                    assert L.ghf_decode_planes_gather_forms(ctx.h, s_ptrs, s_szs, rs["codes"].data_ptr(), s_infos, s_tptrs, s_tbytes, None, None,
                                                            None, None, s_raw, 0, n, e, d_index.data_ptr(), row_elems, row_elems, n_rows,
                                                            d_out.data_ptr(), row_bytes, d_status.data_ptr()) == 0

                with_loop = n_rows <= LOOP_MAX_ROWS
                variants = [("forms_gather", v_forms)] + ([("range_loop", v_loop)] if with_loop else []) + \
                    [("self_gather", v_self), ("plain_forms", v_plain)]
                for name, fn in variants:
                    d_out.zero_()
                    d_status.fill_(-1)
                    fn()
                    ctx.sync()
                    assert torch.equal(d_out, want), (e, step, n_rows, row_elems, name)
                    assert name == "range_loop" or int(d_status.abs().sum().item()) == 0, name
                v_whole()
                ctx.sync()
                assert torch.equal(sel[0].view(-1), want), (e, step, n_rows, row_elems, "whole_select")
                med, times = timed(variants + [("whole_select", v_whole)])
                case = {"rows": n_rows, "row_elems": row_elems, "out_bytes": n_rows * row_bytes,
                        **benchkit.stats(times),
                        "loop_over_forms_gather": round(med["range_loop"] / med["forms_gather"], 2) if with_loop else None,
                        "whole_select_over_forms_gather": round(med["whole_select"] / med["forms_gather"], 3),
                        "forms_gather_over_self_gather": round(med["forms_gather"] / med["self_gather"], 3),
                        "plain_forms_over_self_gather": round(med["plain_forms"] / med["self_gather"], 3),
                        "forms_gather_gb_per_s": round(n_rows * row_bytes / med["forms_gather"] / 1e6, 3)}
                if (n_rows, row_elems) == REQUIRED:
                    case["meets_required"] = med["forms_gather"] < med["range_loop"]
                run["cases"].append(case)
                benchkit.progress(case)
                del d_out, want, d_index
            res["runs"].append(run)
            ctx.planes_index_free(r["indexes"])
            ctx.planes_index_free(rs["indexes"])
            del d_new, d_base, d_whole, r, rs, keep, s_keep
            torch.cuda.empty_cache()
    res["meets_required"] = all(c.get("meets_required", True) for run in res["runs"] for c in run["cases"])
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
