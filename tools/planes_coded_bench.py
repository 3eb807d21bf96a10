#!/usr/bin/env python3
"""What the staged byte-plane calls cost, measured.  Not bench.py: this times typed elements.
For every size in `--mib` (256 and 1024), every element width in `--widths` (2, 4, 8) and two kinds of data -- standard-normal
values from a seeded generator (bf16 = the upper half of fp32, fp32, fp64) and uniform bytes:

  a  ghf_histogram_planes against the only way to these histograms before it (ghf_planes_split + E x ghf_histogram on the
     planes), against ghf_histogram of the flat buffer, and against ghf_copy_d2d(non_temporal = 1) of the same byte count
  b  ghf_compress_planes_coded with GHF_PLANES_BUILD_CODES and with ready codes (trained on the same tensor with
     GHF_HIST_COVER_ALL), against ghf_compress_planes and against ghf_compress of the interleaved buffer

all in one run.  REQUIRED: a is faster than split + E histograms in every row; coded(BUILD_CODES) is faster than
ghf_compress_planes at E = 4 and E = 8 at both sizes.

  c  with --parent-lib (a libghf.so built from the parent commit): ghf_compress_planes and ghf_compress of this tree and of
     the parent, alternating in one process, at the first size of --mib and E = 4: the existing calls keep their times.

Every variant is checked once (histograms against the split + E histograms, BUILD_CODES images against
ghf_compress_planes').  Recipe: tools/benchkit.py, with the cache sweep.  Prints one JSON document and writes it to --out."""
import argparse
import ctypes as C
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def make_elems(torch, synth, kind, n_bytes, e, seed):
    """n_bytes of `kind` as a CUDA uint8 tensor"""
    if kind == "uniform":
        return synth.make(torch, "uniform", n_bytes, offset=0, device="cuda")
    return benchkit.normal_elems(torch, n_bytes, e, seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    ap.add_argument("--widths", default="2,4,8")
    ap.add_argument("--kinds", default="normal,uniform")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parent-lib", default="", help="a libghf.so built from the parent commit, for part c")
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "coded_bench.json"))
    args = ap.parse_args()

    import importlib

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "planes_coded_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "cache_sweep": benchkit.CACHE_SWEEP,
                "required": ["hist_planes < split_plus_hists in every row", "coded_build < compress_planes at E = 4 and 8"], "runs": []})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    sizes_mib = [int(x) for x in args.mib.split(",")]
    for mib in sizes_mib:
        nbytes = mib << 20
        for e in [int(x) for x in args.widths.split(",")]:
            n = nbytes // e
            for kind in args.kinds.split(","):
                d_in = make_elems(torch, synth, kind, nbytes, e, args.seed)
                # a: the histograms
                stride = (n + 255) & ~255
                d_planes = ctx.empty_u8(stride * e)
                d_copy = ctx.empty_u8(nbytes)
                h_new = torch.zeros((e, ghf.NSYM), dtype=torch.int64, device="cuda")
                h_old = torch.zeros((e, ghf.NSYM), dtype=torch.int64, device="cuda")
                h_flat = torch.zeros(ghf.NSYM, dtype=torch.int64, device="cuda")

                def v_copy():
                    assert L.ghf_copy_d2d(ctx.h, d_copy.data_ptr(), d_in.data_ptr(), nbytes, 1) == 0

                def v_hist_planes():
                    assert L.ghf_histogram_planes(ctx.h, d_in.data_ptr(), n, e, 0, h_new.data_ptr()) == 0

                def v_split_hists():
                    assert L.ghf_planes_split(ctx.h, d_in.data_ptr(), n, e, d_planes.data_ptr(), stride) == 0
                    for p in range(e):
                        assert L.ghf_histogram(ctx.h, d_planes.data_ptr() + p * stride, n, h_old.data_ptr() + p * ghf.NSYM * 8) == 0

                def v_hist_flat():
                    assert L.ghf_histogram(ctx.h, d_in.data_ptr(), nbytes, h_flat.data_ptr()) == 0

                v_hist_planes()
                v_split_hists()
                v_hist_flat()
                ctx.sync()
                assert torch.equal(h_new, h_old), (mib, e, kind)
                assert int(h_new[:, :256].sum().item()) == nbytes and torch.equal(h_new[:, :256].sum(0), h_flat[:256])
                med_a, times_a = timed([("copy_nt", v_copy), ("hist_planes", v_hist_planes), ("split_plus_hists", v_split_hists),
                                        ("hist_flat", v_hist_flat)])
                del d_copy, d_planes

                # b: the composed calls
                slot = ghf.planes_slot_bytes(n)
                r_old = ctx.compress_planes(d_in, e, n_elems=n)
                r_new = ctx.compress_planes_coded(d_in, e, n_elems=n)
                codes_ready = ctx.build_codes(ctx.histogram_planes(d_in, e, n_elems=n, flags=ghf.HIST_COVER_ALL))
                r_ready = ctx.compress_planes_coded(d_in, e, d_codes=codes_ready, flags=0, n_elems=n)
                d_flat, nb_flat, d_code_flat = ctx.compress(d_in)
                ctx.sync()
                sizes = [int(v) for v in r_old["out_bytes"].cpu().tolist()]
                assert sizes == [int(v) for v in r_new["out_bytes"].cpu().tolist()], (mib, e, kind)
                assert torch.equal(r_old["codes"], r_new["codes"])
                for p in range(e):
                    assert torch.equal(r_old["out"][p * slot :][: sizes[p]], r_new["out"][p * slot :][: sizes[p]]), (mib, e, kind, p)
                sizes_ready = [int(v) for v in r_ready["out_bytes"].cpu().tolist()]

                def v_cp():
                    assert L.ghf_compress_planes(ctx.h, d_in.data_ptr(), n, e, r_old["out"].data_ptr(), slot, r_old["out_bytes"].data_ptr(),
                                                 r_old["codes"].data_ptr(), None) == 0

                def v_coded_build():
                    assert L.ghf_compress_planes_coded(ctx.h, d_in.data_ptr(), n, e, r_new["codes"].data_ptr(), ghf.PLANES_BUILD_CODES,
                                                       r_new["out"].data_ptr(), slot, r_new["out_bytes"].data_ptr(), None) == 0

                def v_coded_ready():
                    assert L.ghf_compress_planes_coded(ctx.h, d_in.data_ptr(), n, e, codes_ready.data_ptr(), 0, r_ready["out"].data_ptr(),
                                                       slot, r_ready["out_bytes"].data_ptr(), None) == 0

                def v_cf():
                    assert L.ghf_compress(ctx.h, d_in.data_ptr(), nbytes, d_flat.data_ptr(), d_flat.numel(), nb_flat.data_ptr(),
                                          d_code_flat.data_ptr(), None) == 0

                med_b, times_b = timed([("compress_planes", v_cp), ("coded_build", v_coded_build), ("coded_ready", v_coded_ready),
                                        ("compress", v_cf)])
                med = dict(med_a, **med_b)
                times = dict(times_a, **times_b)
                run = {
                    "mib": mib, "elem_bytes": e, "kind": kind, "n_elems": n,
                    **benchkit.stats(times),
                    "copy_tb_per_s_read_plus_write": round(2 * nbytes / med["copy_nt"] / 1e9, 3),
                    "hist_planes_read_tb_per_s": round(nbytes / med["hist_planes"] / 1e9, 3),
                    # the copy moves 2 N bytes, the histogram reads N: the fraction is of the copy's TIME
                    "hist_planes_time_over_copy_time": round(med["hist_planes"] / med["copy_nt"], 4),
                    "time_ratio": {
                        "hist_planes_over_split_plus_hists": round(med["hist_planes"] / med["split_plus_hists"], 4),
                        "hist_planes_over_hist_flat": round(med["hist_planes"] / med["hist_flat"], 4),
                        "coded_build_over_compress_planes": round(med["coded_build"] / med["compress_planes"], 4),
                        "coded_ready_over_compress_planes": round(med["coded_ready"] / med["compress_planes"], 4),
                        "coded_build_over_compress": round(med["coded_build"] / med["compress"], 3),
                        "coded_ready_over_compress": round(med["coded_ready"] / med["compress"], 3),
                        "compress_planes_over_compress": round(med["compress_planes"] / med["compress"], 3),
                    },
                    "stored_bytes": {"own_codes": sum(sizes), "ready_codes_cover_all": sum(sizes_ready), "interleaved": int(nb_flat.item())},
                }
                run["meets_required"] = bool(med["hist_planes"] < med["split_plus_hists"] and (e == 2 or med["coded_build"] < med["compress_planes"]))
                res["runs"].append(run)
                benchkit.progress(run)
                del d_in, d_flat, r_old, r_new, r_ready
                torch.cuda.empty_cache()
    res["meets_required"] = all(r["meets_required"] for r in res["runs"])

    # c: the existing calls, this tree against the parent commit's build
    if args.parent_lib:
        LB = C.CDLL(args.parent_lib)
        vp, sz = C.c_void_p, C.c_size_t
        LB.ghf_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        LB.ghf_ctx_set_stream.argtypes = [vp, vp]
        LB.ghf_ctx_destroy.argtypes = [vp]
        LB.ghf_compress_planes.argtypes = [vp, vp, sz, C.c_uint32, vp, sz, vp, vp, vp]
        LB.ghf_compress.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp]
        hb = vp()
        assert LB.ghf_ctx_create(0, C.byref(hb)) == 0
        assert LB.ghf_ctx_set_stream(hb, vp(torch.cuda.current_stream().cuda_stream)) == 0
        mib, e = sizes_mib[0], 4
        nbytes = mib << 20
        n = nbytes // e
        d_in = make_elems(torch, synth, "normal", nbytes, e, args.seed)
        slot = ghf.planes_slot_bytes(n)
        d_out = ctx.empty_u8(slot * e)
        d_flat = ctx.empty_u8(ghf.compress_bound(nbytes))
        nb = torch.zeros(e, dtype=torch.int64, device="cuda")
        variants = []
        for name, lib, h in (("this", L, ctx.h), ("parent", LB, hb)):
            variants.append((name + "_compress_planes", lambda lib=lib, h=h: lib.ghf_compress_planes(h, d_in.data_ptr(), n, e, d_out.data_ptr(), slot, nb.data_ptr(), None, None)))
            variants.append((name + "_compress", lambda lib=lib, h=h: lib.ghf_compress(h, d_in.data_ptr(), nbytes, d_flat.data_ptr(), d_flat.numel(), nb.data_ptr(), None, None)))
        checked = [(k, (lambda fn=fn: benchkit.ok(fn()))) for k, fn in variants]
        med, times = timed(checked)
        res["parent_ab"] = {"mib": mib, "elem_bytes": e, "kind": "normal", **benchkit.stats(times),
                            "this_over_parent": {"compress_planes": round(med["this_compress_planes"] / med["parent_compress_planes"], 4),
                                                 "compress": round(med["this_compress"] / med["parent_compress"], 4)}}
        benchkit.progress(res["parent_ab"])
        torch.cuda.synchronize()
        LB.ghf_ctx_destroy(hb)
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
