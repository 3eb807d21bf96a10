#!/usr/bin/env python3
"""What decoding stored shared-code bodies costs, measured.  Not bench.py: this times many small
items.  `--mib` MiB of uniform and of zipf bytes, cut into items of 4 KiB and 64 KiB, compressed once with
ghf_histogram_batch(COVER_ALL) + ghf_build_code + ghf_compress_batch_shared.  Then, per item:

  g    ghf_decode_bodies_batch_shared                              (nothing but the bodies and the code)
  g0   the same call, sizes only
  e    ghf_decode_images_batch on pre-assembled header || body images     (the assembly is not timed)
  h    the assembly on the device + e                              (what a caller paid before this call existed)
  b1   ghf_decode_batch_shared with the live side-car              (b' of the issue: the floor, gone with the process)

REQUIRED: g < h at every size and input.  g / e, g / b1 and g0 / g are reported without a requirement, and so are the
passes per round of g (the words of ghf_decode_images_batch_stats).  Every variant is checked once against the input.
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

ASSEMBLY = ("two strided torch copy_ kernels into a [count, stride] uint8 tensor: img[:, :hdr] = header (broadcast), "
            "img[:, hdr:hdr + max_body] = bodies[:, :max_body]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--item-kib", default="4,64")
    ap.add_argument("--kinds", default="uniform,zipf")
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "batch", "bodies_bench.json"))
    args = ap.parse_args()

    import importlib

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "batch_bodies_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    n = args.mib << 20
    res = benchkit.envelope(torch, ghf, args, "ms (device events)")
    res.update({"mib": args.mib, "assembly": ASSEMBLY, "kinds": {}})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync)

    ok = True
    for kind in args.kinds.split(","):
        d_in = synth.make(torch, kind, n, offset=0, device="cuda")
        kres = {"items": {}}
        for kib in [int(x) for x in args.item_kib.split(",")]:
            item = kib << 10
            count = n // item
            sizes = [item] * count
            sidx = ctx.batch_index_alloc(count, item)
            d_hist = ctx.histogram_batch(d_in, sizes=sizes, max_item_bytes=item, flags=ghf.HIST_COVER_ALL)
            d_code = ctx.build_code(d_hist)
            s = ctx.compress_batch_shared(d_in, d_code, sizes=sizes, max_item_bytes=item, index=sidx)
            ctx.sync()
            assert int(s["status"].abs().sum().item()) == 0, (kind, kib)
            code = ctx.code_to_host(d_code)
            hdr_bytes = int(L.ghf_header_bytes(code.max_len))
            d_hdr = ctx.empty_u8(hdr_bytes)
            ctx.write_header(d_code, d_hdr)
            max_body = int(s["out_bytes"].max().item())
            bodies2d = s["out"][: count * s["out_stride"]].view(count, s["out_stride"])
            img_stride = (hdr_bytes + max_body + 15) & ~15
            d_img = torch.zeros((count, img_stride), dtype=torch.uint8, device="cuda")
            iptr = d_img.data_ptr() + torch.arange(count, dtype=torch.int64, device="cuda") * img_stride
            ilen = (s["out_bytes"] + hdr_bytes).contiguous()

            def assemble():
                d_img[:, :hdr_bytes] = d_hdr[:hdr_bytes]
                d_img[:, hdr_bytes : hdr_bytes + max_body] = bodies2d[:, :max_body]

            assemble()
            caps = torch.full((count,), item, dtype=torch.int64, device="cuda")
            # one checked run of every variant
            g0 = ctx.decode_bodies_batch_shared(s["out_ptrs"], s["out_bytes"], d_code)
            g = ctx.decode_bodies_batch_shared(s["out_ptrs"], s["out_bytes"], d_code, out=True, caps=caps)
            e = ctx.decode_images_batch(iptr, ilen, out=True, caps=caps)
            b1 = ctx.decode_batch_shared(s["out_ptrs"], s["out_bytes"], d_code, sidx, s["in_bytes"], out_stride=item)
            ctx.sync()
            for name, r in (("g0", g0), ("g", g), ("e", e), ("b1", b1)):
                assert int(r["status"].abs().sum().item()) == 0, (kind, kib, name)
                assert torch.equal(r["out_bytes"], s["in_bytes"][:count]), (kind, kib, name)
                if name != "g0":
                    assert r["out_stride"] == item and torch.equal(r["out"][:n], d_in), (kind, kib, name)

            def v_g():
                rc = L.ghf_decode_bodies_batch_shared(ctx.h, s["out_ptrs"].data_ptr(), s["out_bytes"].data_ptr(), d_code.data_ptr(), count,
                                                      g["out_ptrs"].data_ptr(), g["out_caps"].data_ptr(), g["out_bytes"].data_ptr(),
                                                      g["status"].data_ptr())
                assert rc == 0

            def v_g0():
                rc = L.ghf_decode_bodies_batch_shared(ctx.h, s["out_ptrs"].data_ptr(), s["out_bytes"].data_ptr(), d_code.data_ptr(), count,
                                                      None, None, g0["out_bytes"].data_ptr(), g0["status"].data_ptr())
                assert rc == 0

            def v_e():
                rc = L.ghf_decode_images_batch(ctx.h, iptr.data_ptr(), ilen.data_ptr(), count, e["out_ptrs"].data_ptr(),
                                               e["out_caps"].data_ptr(), e["out_bytes"].data_ptr(), None, e["status"].data_ptr())
                assert rc == 0

            def v_h():
                assemble()
                v_e()

            def v_b1():
                rc = L.ghf_decode_batch_shared(ctx.h, s["out_ptrs"].data_ptr(), s["out_bytes"].data_ptr(), d_code.data_ptr(),
                                               C.byref(sidx), s["in_bytes"].data_ptr(), count, b1["out_ptrs"].data_ptr(),
                                               b1["out_caps"].data_ptr(), b1["out_bytes"].data_ptr(), b1["status"].data_ptr())
                assert rc == 0

            med, times = timed([("g", v_g), ("g0", v_g0), ("e", v_e), ("h", v_h), ("b1", v_b1)])
            stats = torch.zeros(2, dtype=torch.int64, device="cuda")
            ctx.decode_images_batch_stats(stats)
            v_g0()
            ctx.sync()
            ctx.decode_images_batch_stats(None)
            rounds, passes = stats.cpu().tolist()
            for name, r in (("g0", g0), ("g", g), ("e", e), ("b1", b1)):
                assert int(r["status"].abs().sum().item()) == 0, (kind, kib, name)
            per_item_us = {x: 1e3 * v / count for x, v in med.items()}
            row = {
                "count": count,
                **benchkit.stats(times),
                "per_item_us": {x: round(v, 4) for x, v in per_item_us.items()},
                "gb_per_s": {x: round(n / v / 1e6, 2) for x, v in med.items()},
                "body_bytes_per_item": round(float(s["out_bytes"].sum().item()) / count, 1),
                "shared_header_bytes": hdr_bytes,
                "code_lengths": [code.min_len, code.max_len],
                "rounds_per_item": round(rounds / count, 3),
                "passes_per_round": round(passes / max(rounds, 1), 3),
                "ratios": {"g_over_h": round(med["g"] / med["h"], 4), "g_over_e": round(med["g"] / med["e"], 4),
                           "g_over_b1": round(med["g"] / med["b1"], 4), "g0_over_g": round(med["g0"] / med["g"], 4)},
                "g_lt_h": per_item_us["g"] < per_item_us["h"],
            }
            ok = ok and row["g_lt_h"]
            kres["items"]["%dKiB" % kib] = row
            ctx.batch_index_free(sidx)
            del s, g, g0, e, b1, d_img, bodies2d
        res["kinds"][kind] = kres
        del d_in
    res["required_g_lt_h_everywhere"] = ok
    ctx.close()
    benchkit.write(res, args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
