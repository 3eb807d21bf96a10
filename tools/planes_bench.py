#!/usr/bin/env python3
"""What the byte-plane calls cost and buy, measured.  Not bench.py: this times typed elements.
For every size in `--mib` (256 and 1024), every element width in `--widths` (2, 4, 8) and two kinds of data -- standard-normal
values from a seeded generator (bf16 = the upper half of fp32, fp32, fp64) and uniform bytes:

  a  ghf_planes_split and ghf_planes_merge alone, against ghf_copy_d2d(non_temporal = 1) of the same byte count in the same
     run: the yardstick every streaming kernel of the project is priced against
  b  ghf_compress_planes and the indexed ghf_decode_planes, against ghf_compress and the indexed ghf_decode of the
     interleaved buffer
  c  the stored bytes of both forms

Device events around every call, variants interleaved within each repeat, every variant warmed up first and checked once
(merge(split(x)) == x, both decodes against the input).  In front of every timed call, outside its events, a plain copy of
256 MiB between two buffers of the tool's own sweeps the 256 MiB Infinity Cache, so that no figure depends on which variant
ran before it.  Prints one JSON document and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def make_elems(torch, synth, kind, n_bytes, e, seed):
    """n_bytes of `kind` as a CUDA uint8 tensor"""
    if kind == "uniform":
        return synth.make(torch, "uniform", n_bytes, offset=0, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n = n_bytes // e
    if e == 8:
        return torch.randn(n, generator=g, device="cuda", dtype=torch.float64).view(torch.uint8)
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    if e == 4:
        return x.view(torch.uint8)
    return (x.view(torch.int32) >> 16).to(torch.int16).view(torch.uint8)  # bf16 by truncation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    ap.add_argument("--widths", default="2,4,8")
    ap.add_argument("--kinds", default="normal,uniform")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes", "planes_bench.json"))
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
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "seed": args.seed,
           "lib": ghf.lib_identity(), "unit": "ms (device events), medians", "cache_sweep": "plain 256 MiB copy in front of every timed call", "required_fraction_of_copy": 0.5, "runs": []}

    flush_src, flush_dst = ctx.empty_u8(256 << 20), ctx.empty_u8(256 << 20)
    flush_src.zero_()

    def timed(variants):
        for _ in range(args.warmup):
            for _, fn in variants:
                fn()
        ctx.sync()
        times = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                assert L.ghf_copy_d2d(ctx.h, flush_dst.data_ptr(), flush_src.data_ptr(), flush_src.numel(), 0) == 0
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        ctx.sync()
        return {k: statistics.median(v) for k, v in times.items()}, times

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
                    "median_ms": {k: round(v, 4) for k, v in med.items()},
                    "min_ms": {k: round(min(v), 4) for k, v in times.items()},
                    "max_ms": {k: round(max(v), 4) for k, v in times.items()},
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
                print(json.dumps(run), file=sys.stderr, flush=True)
                ctx.planes_index_free(idx_p)
                ctx.index_free(idx_f)
                del d_in, d_planes, d_back, d_flat, r
                torch.cuda.empty_cache()
    ctx.close()
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
