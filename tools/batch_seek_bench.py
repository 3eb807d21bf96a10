#!/usr/bin/env python3
"""What the run record of stored shared-code bodies costs and buys, measured.  Not bench.py: this
times many small items.  `--mib` MiB of uniform bytes and Zipf bytes (flat items, one code) and of standard-normal bf16 and
fp32 values (one code per byte plane), cut into items of 4 KiB and 64 KiB.  Timed in one run, on the same bodies:

  s    ghf_decode_bodies_batch_shared_seek / .._planes_shared_seek: body + run record     (the new call)
  g    ghf_decode_bodies_batch_shared / .._planes_shared: nothing but the bytes           (what a stored batch pays today)
  b'   ghf_decode_batch_shared / ghf_decode_batch_planes_shared: the live side-car        (what a stored batch cannot keep)
  pack ghf_batch_seek_pack on its own

and the stored bytes per item with a record against the stored bytes with the raw side-car.  REQUIRED: s < g on uniform
bytes and on both typed inputs, at both item sizes; the tool exits 1 otherwise.  g is existing code measured in the same
run; no margin beyond "faster" is fixed.  s / b' and everything about the Zipf input (its skewed code settles in few
passes, so g is already near b') are reported without a requirement.  Every variant is checked against the input first.
Recipe: tools/benchkit.py, with the cache sweep.  The codes come from GHF_HIST_COVER_ALL histograms.  Prints one JSON
document; --out also writes it."""
import argparse
import ctypes as C
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

KINDS = {"uniform_bytes": 1, "zipf_bytes": 1, "bf16_normal": 2, "fp32_normal": 4}
REQUIRED = ("uniform_bytes", "bf16_normal", "fp32_normal")
SEED = 7


def make(torch, kind, n):
    if kind == "bf16_normal":
        return benchkit.normal_bf16_rounded(torch, n, SEED)
    if kind == "fp32_normal":
        return benchkit.normal_fp(torch, n, 4, SEED)
    if kind == "uniform_bytes":
        return benchkit.uniform_bytes(torch, n, SEED)
    return benchkit.zipf_bytes(torch, n, SEED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--item-kib", default="4,64")
    ap.add_argument("--kinds", default=",".join(KINDS))
    benchkit.add_args(ap, reps=10, warmup=2, out=None)
    args = ap.parse_args()

    import torch

    import pkgload

    ghf = pkgload.load().ghf
    assert torch.cuda.is_available(), "batch_seek_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    n = args.mib << 20
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"mib": args.mib, "cache_sweep": benchkit.CACHE_SWEEP, "kinds": {}})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    def clean(*results):
        return all(int(r["status"].abs().sum().item()) == 0 for r in results)

    call = benchkit.ok
    P = lambda t: t.data_ptr()
    ok = True
    for kind in args.kinds.split(","):
        e = KINDS[kind]
        d_in = make(torch, kind, n)
        kres = {"elem_bytes": e, "items": {}}
        for kib in [int(x) for x in args.item_kib.split(",")]:
            item = kib << 10
            count = n // item
            sizes = [item] * count
            idx = ctx.batch_index_alloc(count * e, item // e)
            if e == 1:
                codes = ctx.build_code(ctx.histogram_batch(d_in, sizes=sizes, max_item_bytes=item, flags=ghf.HIST_COVER_ALL))
                c = ctx.compress_batch_shared(d_in, codes, sizes=sizes, max_item_bytes=item, index=idx)
                r = ctx.batch_seek_pack(idx, c["in_bytes"])
                live = ctx.decode_batch_shared(c["out_ptrs"], c["out_bytes"], codes, idx, c["in_bytes"], out_stride=item)
                bare = ctx.decode_bodies_batch_shared(c["out_ptrs"], c["out_bytes"], codes, out=ctx.empty_u8(n), caps=c["in_bytes"])
                seek = ctx.decode_bodies_batch_shared_seek(c["out_ptrs"], c["out_bytes"], r["rec_ptrs"], r["rec_bytes"], codes,
                                                           out=ctx.empty_u8(n), caps=c["in_bytes"])
                hdr = int(L.ghf_header_bytes(ctx.code_to_host(codes).max_len))
            else:
                codes = ctx.build_codes(ctx.histogram_batch_planes(d_in, e, sizes=sizes, max_item_bytes=item, flags=ghf.HIST_COVER_ALL))
                c = ctx.compress_batch_planes_shared(d_in, codes, e, sizes=sizes, max_item_bytes=item, index=idx)
                r = ctx.batch_seek_pack(idx, c["in_bytes"], elem_bytes=e)
                live = ctx.decode_batch_planes_shared(c["out_ptrs"], c["out_bytes"], codes, idx, c["n_elems"], e, out_stride=item)
                bare = ctx.decode_bodies_batch_planes_shared(c["out_ptrs"], c["out_bytes"], codes, e, out=ctx.empty_u8(n), caps=c["in_bytes"])
                seek = ctx.decode_bodies_batch_planes_shared_seek(c["out_ptrs"], c["out_bytes"], r["rec_ptrs"], r["rec_bytes"], codes, e,
                                                                  out=ctx.empty_u8(n), caps=c["in_bytes"])
                hdr = sum(int(L.ghf_header_bytes(ctx.code_to_host(codes[k]).max_len)) for k in range(e))
            ctx.sync()
            assert clean(c, r, live, bare, seek), (kind, kib)
            for name, d in (("b'", live), ("g", bare), ("s", seek)):
                assert torch.equal(d["out"][:n], d_in), (kind, kib, name)

            head = (ctx.h, P(c["out_ptrs"]), P(c["out_bytes"]))
            tail = lambda d: (P(d["out_ptrs"]), P(d["out_caps"]), P(d["out_bytes"]), P(d["status"]))
            recs = (P(r["rec_ptrs"]), P(r["rec_bytes"]))
            if e == 1:
                variants = [
                    ("s", lambda: call(L.ghf_decode_bodies_batch_shared_seek(*head, *recs, P(codes), count, *tail(seek)))),
                    ("g", lambda: call(L.ghf_decode_bodies_batch_shared(*head, P(codes), count, *tail(bare)))),
                    ("b'", lambda: call(L.ghf_decode_batch_shared(*head, P(codes), C.byref(idx), P(c["in_bytes"]), count, *tail(live)))),
                ]
            else:
                variants = [
                    ("s", lambda: call(L.ghf_decode_bodies_batch_planes_shared_seek(*head, *recs, P(codes), count, e, *tail(seek)))),
                    ("g", lambda: call(L.ghf_decode_bodies_batch_planes_shared(*head, P(codes), count, e, *tail(bare)))),
                    ("b'", lambda: call(L.ghf_decode_batch_planes_shared(*head, P(codes), C.byref(idx), P(c["n_elems"]), count, e, *tail(live)))),
                ]
            variants.append(("pack", lambda: call(L.ghf_batch_seek_pack(ctx.h, C.byref(idx), P(c["in_bytes"]), count, e, P(r["rec_ptrs"]),
                                                                       P(r["rec_caps"]), P(r["rec_bytes"]), P(r["status"])))))
            med, times = timed(variants)
            assert clean(c, r, live, bare, seek), (kind, kib)
            for name, d in (("b'", live), ("g", bare), ("s", seek)):
                assert torch.equal(d["out"][:n], d_in), (kind, kib, name)
            bodies = float(c["out_bytes"].sum().item()) / count + hdr / count
            records = float(r["rec_bytes"].sum().item()) / count
            side_car = e * (8.0 * int(idx.blocks_per_item) + 4.0 * int(idx.segs_per_item))
            row = {
                "count": count,
                **benchkit.stats(times),
                "per_item_us": {x: round(1e3 * v / count, 4) for x, v in med.items()},
                "gb_per_s": {x: round(n / v / 1e6, 2) for x, v in med.items()},
                "stored_bytes_per_item": {"input": item, "bodies": round(bodies, 1), "records": round(records, 1),
                                          "with_records": round(bodies + records, 1), "raw_side_car": side_car,
                                          "with_raw_side_car": round(bodies + side_car, 1),
                                          "records_over_input": round(records / item, 5), "side_car_over_input": round(side_car / item, 5)},
                "ratios": {"s_over_g": round(med["s"] / med["g"], 4), "s_over_b'": round(med["s"] / med["b'"], 4)},
                "s_faster_than_g": med["s"] < med["g"],
            }
            if kind in REQUIRED:
                ok = ok and row["s_faster_than_g"]
            kres["items"]["%dKiB" % kib] = row
            benchkit.progress({kind: {"%dKiB" % kib: row}})
            ctx.batch_index_free(idx)
            del c, r, live, bare, seek
        res["kinds"][kind] = kres
        del d_in
    res["required_s_faster_than_g_on"] = list(REQUIRED)
    res["required_met"] = ok
    ctx.close()
    benchkit.write(res, args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
