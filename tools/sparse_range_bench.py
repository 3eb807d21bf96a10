#!/usr/bin/env python3
"""What an element range of a tensor stored as zero-suppressed byte planes costs, measured.  Not
bench.py: this times typed elements against a base.  For every size in `--mib` (256 and 1024), every element width in
`--widths` (2 = bf16, 4 = fp32) and every step in `--steps` (1e-3, 1e-5): seeded standard-normal values against the same
values after the step, compressed by ghf_compress_planes_sparse_ranked_delta(GHF_SPARSE_AUTO), and

  a  ghf_decode_planes_sparse_delta of the whole tensor from side-cars: the call a shard costs without this feature
  b  ghf_decode_planes_sparse_range_delta of the whole range, the middle eighth and 1 MiB of output, from side-cars and
     from seek tables.  REQUIRED: the eighth takes less time than (a), from both sources, in every row
  c  recorded: the same ranges through ghf_decode_planes_range_delta on dense images of the same pair
  d  recorded: ghf_sparse_rank_pack of one plane's mask on its own, and the ranked compress against the plain sparse one

Every variant is checked once against the tensor's slice.  Recipe: tools/benchkit.py, with the cache sweep.  Prints one JSON
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
    ap.add_argument("--widths", default="2,4")
    ap.add_argument("--steps", default="1e-3,1e-5")
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "sparse_range_bench.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    assert torch.cuda.is_available(), "sparse_range_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "data": "standard-normal against itself after a step", "cache_sweep": benchkit.CACHE_SWEEP,
                "required": "range_eighth_idx and range_eighth_tab below decode_sparse_delta in every row", "runs": []})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    def tables_of(indexes, slots):
        """seek tables through the host and back, as a caller that stored them would have them"""
        h = []
        for j in range(slots):
            if not indexes[j].n_symbols:
                h.append(None)
                continue
            d_t = ctx.seek_pack(indexes[j])
            ctx.sync()
            h.append(d_t.cpu().numpy().copy())
        infos = (ghf.SeekInfo * slots)(*[ghf.SeekInfo() if t is None else ghf.seek_parse(t) for t in h])
        d_tables = [None if t is None else torch.from_numpy(t).cuda() for t in h]
        tptrs = (C.c_void_p * slots)(*[None if t is None else t.data_ptr() for t in d_tables])
        tbytes = (C.c_size_t * slots)(*[0 if t is None else t.size for t in h])
        return infos, d_tables, tptrs, tbytes

    for mib in [int(x) for x in args.mib.split(",")]:
        nbytes = mib << 20
        for e in [int(x) for x in args.widths.split(",")]:
            for step in [float(x) for x in args.steps.split(",")]:
                n = nbytes // e
                d_new, d_base = benchkit.normal_pair_reseeded(torch, nbytes, e, step, args.seed)
                d_back = ctx.empty_u8(nbytes)

                # the stored tensor: images, side-cars, rank tables (brought to the host and parsed), seek tables
                r = ctx.compress_planes_sparse_ranked_delta(d_new, d_base, e, n_elems=n, indexes=True)
                ctx.sync()
                slot, rslot, chosen, idx = r["slot_bytes"], r["rank_slot_bytes"], r["sparse_planes"], r["indexes"]
                sizes = [int(v) for v in r["out_bytes"].cpu().tolist()]
                ptrs = (C.c_void_p * (2 * e))(*[r["out"].data_ptr() + j * slot if sizes[j] else None for j in range(2 * e)])
                szs = (C.c_size_t * (2 * e))(*sizes)
                n_vals = (C.c_size_t * e)(*r["n_vals"])
                h_ranks = r["ranks"].cpu().numpy()
                rank_tables = [h_ranks[p * rslot : p * rslot + ghf.sparse_rank_bytes(n)].copy() for p in range(e)]
                r_infos, r_ptrs = (ghf.SparseRankInfo * e)(), (C.c_void_p * e)()
                for p in range(e):
                    if (chosen >> p) & 1:
                        r_infos[p] = ghf.sparse_rank_parse(rank_tables[p])
                        r_ptrs[p] = rank_tables[p].ctypes.data
                infos, d_tables, tptrs, tbytes = tables_of(idx, 2 * e)
                codes = r["codes"]

                # the dense images of the same pair
                pidx = ctx.planes_index_alloc(n, e)
                dr = ctx.compress_planes_delta(d_new, d_base, e, n_elems=n, flags=ghf.PLANES_BUILD_CODES, indexes=pidx)
                ctx.sync()
                d_sizes = [int(v) for v in dr["out_bytes"].cpu().tolist()]
                d_ptrs = (C.c_void_p * e)(*[dr["out"].data_ptr() + p * dr["slot_bytes"] for p in range(e)])
                d_szs = (C.c_size_t * e)(*d_sizes)
                d_infos, d_dtables, d_tptrs, d_tbytes = tables_of(pidx, e)

                eighth = n // 8
                mid = ((7 * n // 16) & ~4095) + 1008 + 5  # no block edge, no multiple of 16
                ranges = {"whole": (0, n), "eighth": (mid, eighth), "mib1": (n // 2 + 5, (1 << 20) // e)}
                shards = {k: d_base[f * e : (f + c) * e].clone() for k, (f, c) in ranges.items()}  # the caller's shard of the base

                def v_whole_sparse():
                    assert L.ghf_decode_planes_sparse_delta(ctx.h, ptrs, szs, codes.data_ptr(), idx, d_base.data_ptr(), chosen, n_vals, n, e,
                                                            d_back.data_ptr(), nbytes, None) == 0

                def v_range(name, by_table):
                    first, count = ranges[name]
                    base = shards[name].data_ptr()

                    def fn():
                        assert L.ghf_decode_planes_sparse_range_delta(
                            ctx.h, ptrs, szs, codes.data_ptr(), None if by_table else idx, infos if by_table else None,
                            tptrs if by_table else None, tbytes if by_table else None, r_infos, r_ptrs, base, chosen, n, e, first, count,
                            d_back.data_ptr(), nbytes) == 0
                    return fn

                def v_dense_range(name, by_table):
                    first, count = ranges[name]
                    base = shards[name].data_ptr()

                    def fn():
                        assert L.ghf_decode_planes_range_delta(
                            ctx.h, d_ptrs, d_szs, dr["codes"].data_ptr(), None if by_table else pidx, d_infos if by_table else None,
                            d_tptrs if by_table else None, d_tbytes if by_table else None, base, e, first, count, d_back.data_ptr(),
                            nbytes) == 0
                    return fn

                variants = [("decode_sparse_delta", v_whole_sparse)]
                where = {"decode_sparse_delta": (0, n)}
                for name in ranges:
                    for tag, by_table in (("idx", False), ("tab", True)):
                        variants += [("range_%s_%s" % (name, tag), v_range(name, by_table)),
                                     ("dense_range_%s_%s" % (name, tag), v_dense_range(name, by_table))]
                        where["range_%s_%s" % (name, tag)] = where["dense_range_%s_%s" % (name, tag)] = ranges[name]
                for name, fn in variants:  # every variant gives the tensor's slice
                    first, count = where[name]
                    d_back[: count * e].zero_()
                    fn()
                    ctx.sync()
                    assert torch.equal(d_back[: count * e], d_new[first * e : (first + count) * e]), (mib, e, step, name)
                med, times = timed(variants)

                # d: the rank table on its own (the mask of the highest plane), and the two compress calls without side-cars
                d_planes, stride = ctx.planes_split_delta(d_new, d_base, e, n_elems=n)
                d_mask, _, _ = ctx.sparse_split(d_planes[(e - 1) * stride : (e - 1) * stride + n], n=n)
                d_rank = ctx.empty_u8(ghf.sparse_rank_bytes(n))
                ctx.sync()
                d_out2 = ctx.empty_u8(2 * e * slot)
                d_ranks2 = ctx.empty_u8(e * rslot)

                def v_rank_pack():
                    assert L.ghf_sparse_rank_pack(ctx.h, d_mask.data_ptr(), n, d_rank.data_ptr(), d_rank.numel()) == 0

                def v_compress_sparse():
                    ctx.compress_planes_sparse_delta(d_new, d_base, e, n_elems=n, d_out=d_out2, slot_bytes=slot)

                def v_compress_ranked():
                    ctx.compress_planes_sparse_ranked_delta(d_new, d_base, e, n_elems=n, d_out=d_out2, slot_bytes=slot, d_ranks=d_ranks2,
                                                            rank_slot_bytes=rslot)

                med_d, times_d = timed([("rank_pack", v_rank_pack), ("compress_sparse_delta", v_compress_sparse),
                                        ("compress_sparse_ranked_delta", v_compress_ranked)])
                med.update(med_d)
                times.update(times_d)

                whole = med["decode_sparse_delta"]
                run = {
                    "mib": mib, "elem_bytes": e, "step": step, "n_elems": n, "sparse_planes": chosen, "n_vals": list(r["n_vals"]),
                    "stored_bytes": sum(sizes), "dense_stored_bytes": sum(d_sizes),
                    "rank_table_bytes": sum(ghf.sparse_rank_bytes(n) for p in range(e) if (chosen >> p) & 1),
                    "ranges": {k: list(v) for k, v in ranges.items()},
                    **benchkit.stats(times),
                    "range_over_decode_sparse_delta": {k: round(v / whole, 4) for k, v in med.items() if k.startswith("range_")},
                    "sparse_range_over_dense_range": {k: round(med[k] / med["dense_" + k], 4) for k in med if k.startswith("range_")},
                    "ranked_over_plain_compress": round(med["compress_sparse_ranked_delta"] / med["compress_sparse_delta"], 4),
                }
                run["meets_required"] = med["range_eighth_idx"] < whole and med["range_eighth_tab"] < whole
                res["runs"].append(run)
                benchkit.progress(run)
                ctx.planes_index_free(idx)
                ctx.planes_index_free(pidx)
                del d_new, d_base, d_back, r, dr, d_tables, d_dtables, shards, d_planes, d_mask, d_out2, d_ranks2
                torch.cuda.empty_cache()
                benchkit.save(res, args.out)  # kept current row by row: a run that is cut short leaves its finished rows
    ctx.close()
    res["meets_required"] = all(run["meets_required"] for run in res["runs"])
    benchkit.write(res, args.out)
    if not res["meets_required"]:  # the required comparison is the point of the tool: a miss is an error, not a field
        missed = [(r["mib"], r["elem_bytes"], r["step"]) for r in res["runs"] if not r["meets_required"]]
        print("REQUIRED ROW MISSED in %s: the middle eighth is not below decode_sparse_delta" % missed, file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
