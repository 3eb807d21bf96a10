#!/usr/bin/env python3
"""What one shared code buys over one code per item, measured.  Not bench.py: this times many small
items.  `--mib` MiB of uniform and of zipf bytes, cut into items of 4 KiB and 64 KiB:

  a    ghf_compress_batch over all items                                            (a code and a header per item)
  a1   ghf_histogram_batch + ghf_build_code + ghf_compress_batch_shared             (the code is made from the batch)
  a2   ghf_compress_batch_shared alone                                              (the caller has the code)
  b    ghf_decode_batch
  b1   ghf_decode_batch_shared

Reported per item (call time / items), with the stored bytes per item of both forms: the image of `a` against the body
of `a2` plus the one header divided by the item count.  REQUIRED: a2 < a per item at every size and input (the shared
kernel does a strict subset of a's work); a1 and b1 are reported against a and b without a requirement.  Every variant is
checked once (stored header || body through ghf_decode_images_batch on a sample, both decodes against the input).
Recipe: tools/benchkit.py, without the cache sweep.  Prints one JSON document; --out also writes it to a file.  Exit
status 1 when a required row fails."""
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
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--item-kib", default="4,64")
    ap.add_argument("--kinds", default="uniform,zipf")
    benchkit.add_args(ap, reps=10, warmup=2, out=None)
    args = ap.parse_args()

    import importlib

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "batch_shared_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    n = args.mib << 20
    res = benchkit.envelope(torch, ghf, args, "ms (device events)")
    res.update({"mib": args.mib, "kinds": {}})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync)

    ok = True
    for kind in args.kinds.split(","):
        d_in = synth.make(torch, kind, n, offset=0, device="cuda")
        kres = {"items": {}}
        for kib in [int(x) for x in args.item_kib.split(",")]:
            item = kib << 10
            count = n // item
            sizes = [item] * count
            # a / b: a code per item
            bidx = ctx.batch_index_alloc(count, item)
            r = ctx.compress_batch(d_in, sizes=sizes, max_item_bytes=item, index=bidx)
            dec = ctx.decode_batch(r["out_ptrs"], r["out_bytes"], r["codes"], bidx, r["in_bytes"], out_stride=item)
            ctx.sync()
            assert int(r["status"].abs().sum().item()) == 0 and int(dec["status"].abs().sum().item()) == 0, (kind, kib)
            assert torch.equal(dec["out"][:n], d_in), (kind, kib)
            # a1 / a2 / b1: one code for the batch
            sidx = ctx.batch_index_alloc(count, item)
            d_hist = ctx.histogram_batch(d_in, sizes=sizes, max_item_bytes=item)
            d_code = ctx.build_code(d_hist)
            s = ctx.compress_batch_shared(d_in, d_code, sizes=sizes, max_item_bytes=item, index=sidx)
            sdec = ctx.decode_batch_shared(s["out_ptrs"], s["out_bytes"], d_code, sidx, s["in_bytes"], out_stride=item)
            ctx.sync()
            assert int(s["status"].abs().sum().item()) == 0 and int(sdec["status"].abs().sum().item()) == 0, (kind, kib)
            assert torch.equal(sdec["out"][:n], d_in), (kind, kib)
            # the stored form: header || body of a few items through the decoder that takes nothing but images
            code = ctx.code_to_host(d_code)
            hdr_bytes = int(L.ghf_header_bytes(code.max_len))
            d_hdr = ctx.empty_u8(hdr_bytes)
            ctx.write_header(d_code, d_hdr)
            nbs = s["out_bytes"].cpu().tolist()
            sample = sorted({0, count // 3, count - 1})
            img_stride = (hdr_bytes + max(nbs[i] for i in sample) + 31) & ~15
            d_img = torch.zeros(len(sample) * img_stride, dtype=torch.uint8, device="cuda")
            for k, i in enumerate(sample):
                d_img[k * img_stride : k * img_stride + hdr_bytes] = d_hdr[:hdr_bytes]
                d_img[k * img_stride + hdr_bytes : k * img_stride + hdr_bytes + nbs[i]] = s["out"][i * s["out_stride"] :][: nbs[i]]
            iptr = d_img.data_ptr() + torch.arange(len(sample), dtype=torch.int64, device="cuda") * img_stride
            ilen = torch.tensor([hdr_bytes + nbs[i] for i in sample], dtype=torch.int64, device="cuda")
            icap = torch.full((len(sample),), item, dtype=torch.int64, device="cuda")
            im = ctx.decode_images_batch(iptr, ilen, out=True, caps=icap)
            ctx.sync()
            assert int(im["status"].abs().sum().item()) == 0, (kind, kib)
            for k, i in enumerate(sample):
                assert torch.equal(im["out"][k * im["out_stride"] :][:item], d_in[i * item : (i + 1) * item]), (kind, kib, i)

            def v_a():
                rc = L.ghf_compress_batch(ctx.h, r["in_ptrs"].data_ptr(), r["in_bytes"].data_ptr(), item, count, r["out_ptrs"].data_ptr(),
                                          r["out_caps"].data_ptr(), r["out_bytes"].data_ptr(), r["codes"].data_ptr(), C.byref(bidx),
                                          r["status"].data_ptr())
                assert rc == 0

            def v_a2():
                rc = L.ghf_compress_batch_shared(ctx.h, s["in_ptrs"].data_ptr(), s["in_bytes"].data_ptr(), item, count, d_code.data_ptr(),
                                                 s["out_ptrs"].data_ptr(), s["out_caps"].data_ptr(), s["out_bytes"].data_ptr(),
                                                 C.byref(sidx), s["status"].data_ptr())
                assert rc == 0

            def v_a1():
                rc = L.ghf_histogram_batch(ctx.h, s["in_ptrs"].data_ptr(), s["in_bytes"].data_ptr(), item, count, 0, d_hist.data_ptr())
                assert rc == 0
                rc = L.ghf_build_code(ctx.h, d_hist.data_ptr(), d_code.data_ptr())
                assert rc == 0
                v_a2()

            def v_b():
                rc = L.ghf_decode_batch(ctx.h, r["out_ptrs"].data_ptr(), r["out_bytes"].data_ptr(), r["codes"].data_ptr(), C.byref(bidx),
                                        r["in_bytes"].data_ptr(), count, dec["out_ptrs"].data_ptr(), dec["out_caps"].data_ptr(),
                                        dec["out_bytes"].data_ptr(), dec["status"].data_ptr())
                assert rc == 0

            def v_b1():
                rc = L.ghf_decode_batch_shared(ctx.h, s["out_ptrs"].data_ptr(), s["out_bytes"].data_ptr(), d_code.data_ptr(),
                                               C.byref(sidx), s["in_bytes"].data_ptr(), count, sdec["out_ptrs"].data_ptr(),
                                               sdec["out_caps"].data_ptr(), sdec["out_bytes"].data_ptr(), sdec["status"].data_ptr())
                assert rc == 0

            med, times = timed([("a", v_a), ("a1", v_a1), ("a2", v_a2), ("b", v_b), ("b1", v_b1)])
            ctx.sync()
            assert int(s["status"].abs().sum().item()) == 0 and int(sdec["status"].abs().sum().item()) == 0, (kind, kib)
            per_item_us = {x: 1e3 * v / count for x, v in med.items()}
            image_bytes = float(r["out_bytes"].sum().item()) / count
            body_bytes = float(s["out_bytes"].sum().item()) / count
            row = {
                "count": count,
                **benchkit.stats(times),
                "per_item_us": {x: round(v, 4) for x, v in per_item_us.items()},
                "gb_per_s": {x: round(n / v / 1e6, 2) for x, v in med.items()},
                "stored_bytes_per_item": {"image": round(image_bytes, 1), "body_plus_header_share": round(body_bytes + hdr_bytes / count, 1),
                                          "input": item, "shared_header_bytes": hdr_bytes},
                "ratios": {"a2_over_a": round(med["a2"] / med["a"], 4), "a1_over_a": round(med["a1"] / med["a"], 4),
                           "b1_over_b": round(med["b1"] / med["b"], 4)},
                "a2_lt_a": per_item_us["a2"] < per_item_us["a"],
            }
            ok = ok and row["a2_lt_a"]
            kres["items"]["%dKiB" % kib] = row
            ctx.batch_index_free(bidx)
            ctx.batch_index_free(sidx)
            del r, dec, s, sdec, d_img, im
        res["kinds"][kind] = kres
        del d_in
    res["required_a2_lt_a_everywhere"] = ok
    ctx.close()
    benchkit.write(res, args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
