#!/usr/bin/env python3
"""What ghf_decode_images_batch costs and buys, measured.  Not bench.py: this times the decode of
many small standalone .crs2 images.  `--mib` MiB of uniform and of zipf bytes, cut into items of 4 KiB, 64 KiB and 1 MiB
and compressed once with ghf_compress_batch; then, per item:

  e   ghf_decode_images_batch, decode mode: the images alone                      (one launch)
  e0  the same, sizes only                                                        (one launch)
  b   ghf_decode_batch with the live tables and side-car                          (one launch)
  f   the existing route for images that come with nothing: a loop over `--loop-items` of the same items of host
      ghf_parse_header + table upload + ghf_decode(index = NULL)

Every variant is checked once against the input.  Recipe: tools/benchkit.py, without the cache sweep.  For e0 the kernel's
own counters (ghf_decode_images_batch_stats) give the observed passes per round, to hold against the bound of 256.

Every (kind, item size) is one GPU step: a child process of its own under `timeout -k 10`, started only if the one
before it ended well.  Prints one JSON document; --out (default profiles/batch/images_bench.json) also keeps it."""
import argparse
import json
import os
import subprocess
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def step(args, kind, kib):
    import ctypes as C
    import importlib

    import numpy as np
    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "batch_images_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    n = args.mib << 20
    item = kib << 10
    count = n // item
    d_in = synth.make(torch, kind, n, offset=0, device="cuda")
    bidx = ctx.batch_index_alloc(count, item)
    r = ctx.compress_batch(d_in, sizes=[item] * count, max_item_bytes=item, index=bidx)
    ctx.sync()
    assert int(r["status"].abs().sum().item()) == 0, (kind, kib)
    stride = r["out_stride"]
    caps = torch.full((count,), item, dtype=torch.int64, device="cuda")

    # e / e0 / b, every output buffer allocated beforehand
    e = ctx.decode_images_batch(r["out_ptrs"], r["out_bytes"], out=ctx.empty_u8(n), caps=caps)
    e0 = ctx.decode_images_batch(r["out_ptrs"], r["out_bytes"])
    b = ctx.decode_batch(r["out_ptrs"], r["out_bytes"], r["codes"], bidx, r["in_bytes"], out_stride=item)
    ctx.sync()
    for name, v in (("e", e), ("e0", e0), ("b", b)):
        assert int(v["status"].abs().sum().item()) == 0, (kind, kib, name)
        assert bool((v["out_bytes"] == item).all().item()), (kind, kib, name)
    assert torch.equal(e["out"][:n], d_in) and torch.equal(b["out"][:n], d_in), (kind, kib)

    def v_e():
        assert L.ghf_decode_images_batch(ctx.h, r["out_ptrs"].data_ptr(), r["out_bytes"].data_ptr(), count, e["out_ptrs"].data_ptr(),
                                         e["out_caps"].data_ptr(), e["out_bytes"].data_ptr(), None, e["status"].data_ptr()) == 0

    def v_e0():
        assert L.ghf_decode_images_batch(ctx.h, r["out_ptrs"].data_ptr(), r["out_bytes"].data_ptr(), count, None, None,
                                         e0["out_bytes"].data_ptr(), None, e0["status"].data_ptr()) == 0

    def v_b():
        assert L.ghf_decode_batch(ctx.h, r["out_ptrs"].data_ptr(), r["out_bytes"].data_ptr(), r["codes"].data_ptr(), C.byref(bidx),
                                  r["in_bytes"].data_ptr(), count, b["out_ptrs"].data_ptr(), b["out_caps"].data_ptr(),
                                  b["out_bytes"].data_ptr(), b["status"].data_ptr()) == 0

    # f: the images are on the host as well (they were stored, sent, or written by the reference); per item the host
    # parses the header, uploads the tables and calls the single-stream decoder, which rebuilds the side-car (K6)
    k = min(args.loop_items, count)
    nbs = r["out_bytes"][:k].cpu().tolist()
    h_images = r["out"][: k * stride].cpu().numpy()
    loop = []
    for i in range(k):
        img = np.ascontiguousarray(h_images[i * stride : i * stride + nbs[i]])
        loop.append({"img": img, "code": ghf.Code(), "d_code": ctx.new_code(), "back": ctx.empty_u8(item),
                     "nbytes": torch.zeros(1, dtype=torch.int64, device="cuda"), "d_stream": r["out_ptrs"][i].item(), "nb": nbs[i]})
    code_bytes = C.sizeof(ghf.Code)

    def v_f():
        for it in loop:
            assert L.ghf_parse_header(it["img"].ctypes.data, it["nb"], C.byref(it["code"]), None) == 0
            assert L.ghf_copy_h2d(ctx.h, it["d_code"].data_ptr(), C.byref(it["code"]), code_bytes) == 0
            assert L.ghf_decode(ctx.h, it["d_stream"], it["nb"], it["d_code"].data_ptr(), None, it["back"].data_ptr(), item,
                                it["nbytes"].data_ptr()) == 0

    v_f()
    ctx.sync()
    assert all(torch.equal(it["back"][:item], d_in[i * item : (i + 1) * item]) for i, it in enumerate(loop)), (kind, kib)

    med, times = benchkit.timed([("e", v_e), ("e0", v_e0), ("b", v_b), ("f", v_f)], args.reps, args.warmup, ctx.sync)

    # the kernel's own counters over one sizes-only call
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    ctx.decode_images_batch_stats(stats)
    v_e0()
    ctx.sync()
    ctx.decode_images_batch_stats(None)
    rounds, passes = stats.cpu().tolist()

    per_item_us = {"e": 1e3 * med["e"] / count, "e0": 1e3 * med["e0"] / count, "b": 1e3 * med["b"] / count, "f": 1e3 * med["f"] / k}
    res = {
        "device": torch.cuda.get_device_name(0),
        "lib": ghf.lib_identity(),
        "count": count,
        "looped_items": k,
        "image_bytes_mean": round(float(r["out_bytes"].double().mean().item()), 1),
        **benchkit.stats(times),
        "per_item_us": {x: round(v, 3) for x, v in per_item_us.items()},
        "gb_per_s": {"e": round(n / med["e"] / 1e6, 2), "e0": round(n / med["e0"] / 1e6, 2), "b": round(n / med["b"] / 1e6, 2),
                     "f": round(k * item / med["f"] / 1e6, 3)},
        "ratios": {"f_over_e": round(per_item_us["f"] / per_item_us["e"], 2), "e_over_b": round(per_item_us["e"] / per_item_us["b"], 2),
                   "e0_over_e": round(per_item_us["e0"] / per_item_us["e"], 3)},
        "e_lt_f": per_item_us["e"] < per_item_us["f"],
        "rounds_per_item": round(rounds / count, 3),
        "passes_per_round": round(passes / max(rounds, 1), 2),
        "passes_per_round_bound": 256,
    }
    ctx.batch_index_free(bidx)
    ctx.close()
    print("STEP " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--item-kib", default="4,64,1024")
    ap.add_argument("--loop-items", type=int, default=256)
    ap.add_argument("--kinds", default="uniform,zipf")
    ap.add_argument("--step-seconds", type=int, default=240, help="time limit of one (kind, item size) step")
    benchkit.add_args(ap, reps=10, warmup=2, out=os.path.join(ROOT, "profiles", "batch", "images_bench.json"))
    ap.add_argument("--step", nargs=2, metavar=("KIND", "KIB"), default=None, help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        return step(args, args.step[0], int(args.step[1]))

    res = {"mib": args.mib, "reps": args.reps, "warmup": args.warmup, "loop_items": args.loop_items,
           "unit": "ms (device events)", "kinds": {}}
    ok = True
    for kind in args.kinds.split(","):
        for kib in [int(x) for x in args.item_kib.split(",")]:
            cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--step", kind, str(kib),
                   "--mib", str(args.mib), "--loop-items", str(args.loop_items), "--reps", str(args.reps), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            line = [x for x in p.stdout.splitlines() if x.startswith("STEP ")]
            if p.returncode != 0 or not line:  # nothing more is started on the GPU after a step that failed
                res["failed"] = {"kind": kind, "kib": kib, "returncode": p.returncode, "stderr": p.stderr[-2000:]}
                ok = False
                break
            res["kinds"].setdefault(kind, {"items": {}})["items"]["%dKiB" % kib] = json.loads(line[0][5:])
            print("%s %d KiB done" % (kind, kib), file=sys.stderr, flush=True)
        if not ok:
            break
    benchkit.write(res, args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
