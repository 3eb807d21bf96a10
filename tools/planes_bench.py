#!/usr/bin/env python3
"""What the byte-plane calls cost and buy, measured.  Not bench.py: this times typed elements.
For every size in `--mib` (256 and 1024), every element width in `--widths` (2, 4, 8) and two kinds of data -- standard-normal
values from a seeded generator (bf16 = the upper half of fp32, fp32, fp64) and uniform bytes:

  a  ghf_planes_split and ghf_planes_merge alone, against ghf_copy_d2d(non_temporal = 1) of the same byte count in the same
     run: the yardstick every streaming kernel of the project is priced against
  b  ghf_compress_planes and the indexed ghf_decode_planes, against ghf_compress and the indexed ghf_decode of the
     interleaved buffer
  c  the stored bytes of both forms

Every variant is checked once (merge(split(x)) == x, both decodes against the input).  Recipe: tools/benchkit.py, with the
cache sweep.  Prints one JSON document and writes it to --out."""
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
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "planes_bench.json"))
    args = ap.parse_args()

    import importlib

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "planes_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "cache_sweep": benchkit.CACHE_SWEEP, "required_fraction_of_copy": 0.5, "runs": []})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    for mib in [int(x) for x in args.mib.split(",")]:
        nbytes = mib << 20
        for e in [int(x) for x in args.widths.split(",")]:
            n = nbytes // e
            for kind in args.kinds.split(","):
                d_in = make_elems(torch, synth, kind, nbytes, e, args.seed)
                # a: the two kernels alone, and the copy probe
                stride = (n + 255) & ~255
                d_planes = ctx.empty_u8(stride * e)
                d_copy = ctx.empty_u8(nbytes)
                d_back = ctx.empty_u8(nbytes)
                ctx.planes_split(d_in, e, n_elems=n, d_planes=d_planes, plane_stride=stride)
                ctx.planes_merge(d_planes, stride, n, e, d_out=d_back)
                ctx.sync()
                assert torch.equal(d_back, d_in), (mib, e, kind)
                assert torch.equal(d_planes[:n], d_in[0::e]) and torch.equal(d_planes[(e - 1) * stride :][:n], d_in[e - 1 :: e])

                def v_copy():
                    assert L.ghf_copy_d2d(ctx.h, d_copy.data_ptr(), d_in.data_ptr(), nbytes, 1) == 0

                def v_split():
                    assert L.ghf_planes_split(ctx.h, d_in.data_ptr(), n, e, d_planes.data_ptr(), stride) == 0

                def v_merge():
                    assert L.ghf_planes_merge(ctx.h, d_planes.data_ptr(), stride, n, e, d_back.data_ptr()) == 0

                med_a, times_a = timed([("copy_nt", v_copy), ("split", v_split), ("merge", v_merge)])
                del d_copy

                # b: the two forms of the codec, indexed decode on both sides
                idx_p = ctx.planes_index_alloc(n, e)
                r = ctx.compress_planes(d_in, e, n_elems=n, indexes=idx_p)
                idx_f = ctx.index_alloc(nbytes)
                d_flat, nb_flat, d_code_flat = ctx.compress(d_in, index=idx_f)
                ctx.sync()
                sizes = [int(v) for v in r["out_bytes"].cpu().tolist()]
                flat = int(nb_flat.item())
                slot = r["slot_bytes"]
                ptrs = (C.c_void_p * e)(*[r["out"].data_ptr() + p * slot for p in range(e)])
                szs = (C.c_size_t * e)(*sizes)
                nb_dev = torch.zeros(1, dtype=torch.int64, device="cuda")

                def v_cp():
                    assert L.ghf_compress_planes(ctx.h, d_in.data_ptr(), n, e, r["out"].data_ptr(), slot, r["out_bytes"].data_ptr(),
                                                 r["codes"].data_ptr(), idx_p) == 0

                def v_dp():
                    assert L.ghf_decode_planes(ctx.h, ptrs, szs, r["codes"].data_ptr(), idx_p, n, e, d_back.data_ptr(), nbytes,
                                               nb_dev.data_ptr()) == 0

                def v_cf():
                    assert L.ghf_compress(ctx.h, d_in.data_ptr(), nbytes, d_flat.data_ptr(), d_flat.numel(), nb_flat.data_ptr(),
                                          d_code_flat.data_ptr(), C.byref(idx_f)) == 0

                def v_df():
                    assert L.ghf_decode(ctx.h, d_flat.data_ptr(), flat, d_code_flat.data_ptr(), C.byref(idx_f), d_back.data_ptr(),
                                        nbytes, nb_dev.data_ptr()) == 0

                for v in (v_dp, v_df):  # both decodes give the input back
                    d_back.zero_()
                    v()
                    ctx.sync()
                    assert torch.equal(d_back, d_in), (mib, e, kind, v.__name__)
                med_b, times_b = timed([("compress_planes", v_cp), ("decode_planes", v_dp), ("compress", v_cf), ("decode", v_df)])
                med = dict(med_a, **med_b)
                times = dict(times_a, **times_b)
                run = {
                    "mib": mib, "elem_bytes": e, "kind": kind, "n_elems": n,
                    **benchkit.stats(times),
                    # read + write, as bench.py counts the copy probe
                    "tb_per_s": {k: round(2 * nbytes / med[k] / 1e9, 3) for k in ("copy_nt", "split", "merge")},
                    "fraction_of_copy": {"split": round(med["copy_nt"] / med["split"], 4), "merge": round(med["copy_nt"] / med["merge"], 4)},
                    "time_ratio": {"compress_planes_over_compress": round(med["compress_planes"] / med["compress"], 3),
                                   "decode_planes_over_decode": round(med["decode_planes"] / med["decode"], 3)},
                    "stored_bytes": {"planes": sizes, "planes_total": sum(sizes), "interleaved": flat,
                                     "planes_over_interleaved": round(sum(sizes) / flat, 4)},
                }
                run["meets_required"] = min(run["fraction_of_copy"].values()) >= res["required_fraction_of_copy"]
                res["runs"].append(run)
                benchkit.progress(run)
                ctx.planes_index_free(idx_p)
                ctx.index_free(idx_f)
                del d_in, d_planes, d_back, d_flat, r
                torch.cuda.empty_cache()
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
