#!/usr/bin/env python3
"""What the batch calls buy, measured.  Not bench.py: this times many small independent streams.
`--mib` MiB of uniform and of zipf bytes, cut into items of 4 KiB, 64 KiB and 1 MiB:

  a  ghf_compress_batch over all items                         (one launch)
  b  ghf_decode_batch over all items                           (one launch)
  c  the per-item loop of ghf_compress, and of ghf_decode with its side-car, over `--loop-items` of the same items:
     the unchanged single-stream path, the baseline
  d  ONE ghf_compress / ghf_decode of the concatenation: the ceiling

Reported per item (a, b: call time / items; c: loop time / looped items) with the ratios c / a and the fraction of d's
throughput that a and b reach.  Every variant is checked once (batch images against the looped single-stream images,
decodes against the input).  Recipe: tools/benchkit.py, without the cache sweep.  Prints one JSON document; --out also
writes it to a file."""
import argparse
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--item-kib", default="4,64,1024")
    ap.add_argument("--loop-items", type=int, default=256)
    ap.add_argument("--kinds", default="uniform,zipf")
    benchkit.add_args(ap, reps=10, warmup=2, out=None)
    args = ap.parse_args()

    import importlib

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "batch_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    n = args.mib << 20
    res = benchkit.envelope(torch, ghf, args, "ms (device events)")
    res.update({"mib": args.mib, "loop_items": args.loop_items, "kinds": {}})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync)

    for kind in args.kinds.split(","):
        d_in = synth.make(torch, kind, n, offset=0, device="cuda")
        # d: the ceiling, one stream
        idx_all = ctx.index_alloc(n)
        d_stream_all, nbytes_all, d_code_all = ctx.compress(d_in, index=idx_all)
        ctx.sync()
        nb_all = int(nbytes_all.item())
        d_back_all = ctx.empty_u8(n + 64)

        def v_d_comp():
            ctx.compress(d_in, d_out=d_stream_all, d_code=d_code_all, index=idx_all)

        def v_d_dec():
            ctx.decode(d_stream_all, nb_all, d_code_all, idx_all, d_out=d_back_all)

        v_d_dec()
        ctx.sync()
        assert torch.equal(d_back_all[:n], d_in), kind
        med_d, times_d = timed([("d_compress", v_d_comp), ("d_decode", v_d_dec)])
        kres = {"one_stream_ms": benchkit.stats(times_d)["median_ms"], "stream_bytes": nb_all, "items": {}}

        for kib in [int(x) for x in args.item_kib.split(",")]:
            item = kib << 10
            count = n // item
            sizes = [item] * count
            bidx = ctx.batch_index_alloc(count, item)
            r = ctx.compress_batch(d_in, sizes=sizes, max_item_bytes=item, index=bidx)
            ctx.sync()
            assert int(r["status"].abs().sum().item()) == 0, (kind, kib)
            stride = r["out_stride"]
            dec = ctx.decode_batch(r["out_ptrs"], r["out_bytes"], r["codes"], bidx, r["in_bytes"], out_stride=item)
            ctx.sync()
            assert int(dec["status"].abs().sum().item()) == 0, (kind, kib)
            assert torch.equal(dec["out"][:n], d_in), (kind, kib)
            L = ghf.lib()
            import ctypes as C

            status = r["status"]

            def v_a():
                rc = L.ghf_compress_batch(ctx.h, r["in_ptrs"].data_ptr(), r["in_bytes"].data_ptr(), item, count, r["out_ptrs"].data_ptr(),
                                          r["out_caps"].data_ptr(), r["out_bytes"].data_ptr(), r["codes"].data_ptr(), C.byref(bidx),
                                          status.data_ptr())
                assert rc == 0

            def v_b():
                rc = L.ghf_decode_batch(ctx.h, r["out_ptrs"].data_ptr(), r["out_bytes"].data_ptr(), r["codes"].data_ptr(), C.byref(bidx),
                                        r["in_bytes"].data_ptr(), count, dec["out_ptrs"].data_ptr(), dec["out_caps"].data_ptr(),
                                        dec["out_bytes"].data_ptr(), dec["status"].data_ptr())
                assert rc == 0

            # c: the loop over the first `loop_items` items, every item with buffers of its own
            k = min(args.loop_items, count)
            loop = []
            for i in range(k):
                src = d_in[i * item : (i + 1) * item]
                idx = ctx.index_alloc(item)
                out, nbytes, code = ctx.compress(src, index=idx)
                loop.append({"src": src, "idx": idx, "out": out, "nbytes": nbytes, "code": code, "back": ctx.empty_u8(item)})
            ctx.sync()
            nbs = r["out_bytes"].cpu().tolist()
            for i, it in enumerate(loop):  # both paths write the same images
                it["nb"] = int(it["nbytes"].item())
                assert it["nb"] == nbs[i], (kind, kib, i)
                assert torch.equal(it["out"][: it["nb"]], r["out"][i * stride : i * stride + it["nb"]]), (kind, kib, i)

            # (the C entry points themselves, with every buffer allocated beforehand: nothing but the library is timed)
            for it in loop:
                it["comp"] = (ctx.h, it["src"].data_ptr(), item, it["out"].data_ptr(), it["out"].numel(), it["nbytes"].data_ptr(),
                              it["code"].data_ptr(), C.byref(it["idx"]))
                it["dec"] = (ctx.h, it["out"].data_ptr(), it["nb"], it["code"].data_ptr(), C.byref(it["idx"]), it["back"].data_ptr(),
                             item, it["nbytes"].data_ptr())

            def v_c_comp():
                for it in loop:
                    L.ghf_compress(*it["comp"])

            def v_c_dec():
                for it in loop:
                    L.ghf_decode(*it["dec"])

            v_c_dec()
            ctx.sync()
            assert all(torch.equal(it["back"][:item], it["src"]) for it in loop), (kind, kib)
            med, times = timed([("a", v_a), ("b", v_b), ("c_compress", v_c_comp), ("c_decode", v_c_dec)])
            per_item_us = {"a": 1e3 * med["a"] / count, "b": 1e3 * med["b"] / count, "c_compress": 1e3 * med["c_compress"] / k,
                           "c_decode": 1e3 * med["c_decode"] / k}
            kres["items"]["%dKiB" % kib] = {
                "count": count,
                "looped_items": k,
                **benchkit.stats(times),
                "per_item_us": {x: round(v, 3) for x, v in per_item_us.items()},
                "gb_per_s": {"a": round(n / med["a"] / 1e6, 2), "b": round(n / med["b"] / 1e6, 2),
                             "c_compress": round(k * item / med["c_compress"] / 1e6, 3),
                             "c_decode": round(k * item / med["c_decode"] / 1e6, 3)},
                "ratios": {"loop_over_batch_compress": round(per_item_us["c_compress"] / per_item_us["a"], 2),
                           "loop_over_batch_decode": round(per_item_us["c_decode"] / per_item_us["b"], 2),
                           "fraction_of_one_stream_compress": round(med_d["d_compress"] / med["a"], 4),
                           "fraction_of_one_stream_decode": round(med_d["d_decode"] / med["b"], 4)},
                "a_lt_c": per_item_us["a"] < per_item_us["c_compress"],
                "b_lt_c": per_item_us["b"] < per_item_us["c_decode"],
            }
            for it in loop:
                ctx.index_free(it["idx"])
            ctx.batch_index_free(bidx)
            del loop, r, dec
        res["kinds"][kind] = kres
        ctx.index_free(idx_all)
        del d_in, d_stream_all, d_back_all
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
