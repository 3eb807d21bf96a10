#!/usr/bin/env python3
"""What storing the incompressible byte planes of a batch RAW costs and buys, measured.  Not
bench.py: this times many small items.  `--mib` MiB of bf16 and fp32 standard-normal values and of uniform bytes (taken
as 2-byte elements), cut into items of 4 KiB and 64 KiB, under GHF_HIST_COVER_ALL codes; the mask comes from
ghf_batch_planes_raw_auto.  Each forms call is timed against its all-dense parent on the same items in the same run:

  cp   ghf_compress_batch_planes_shared             cf   ghf_compress_batch_planes_forms            c0   .. with raw_planes == 0
  dp   ghf_decode_batch_planes_shared               df   ghf_decode_batch_planes_forms              d0
  sp   ghf_decode_bodies_batch_planes_shared        sf   ghf_decode_bodies_batch_planes_forms       s0
  kp   ghf_decode_bodies_batch_planes_shared_seek   kf   ghf_decode_bodies_batch_planes_forms_seek  k0
  auto ghf_batch_planes_raw_auto on its own

Required: on bf16 and fp32 at both item sizes sf takes less time than sp (no margin: the call drops the planes that
dominate the parent's time).  Recorded, not required: the other three pairs and the raw_planes == 0 calls against their
parents; the stored bytes of both forms.  Every variant is checked against the input first.  Recipe: tools/benchkit.py,
with the cache sweep.  Prints one JSON document; --out also writes it.  Exit status 1 when a required row fails."""
import argparse
import ctypes as C
import functools
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

KINDS = {"bf16_normal": 2, "fp32_normal": 4, "uniform_bytes": 2}
PAIRS = {"c": "compress", "d": "decode with the live side-car", "s": "decode from the bodies alone", "k": "decode with run records"}
SEED = 7


def make(torch, kind, n):
    if kind == "bf16_normal":
        return benchkit.normal_bf16_rounded(torch, n, SEED)
    if kind == "fp32_normal":
        return benchkit.normal_fp(torch, n, 4, SEED)
    return benchkit.uniform_bytes(torch, n, SEED)


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
    assert torch.cuda.is_available(), "batch_forms_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    L = ghf.lib()
    n = args.mib << 20
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"mib": args.mib, "cache_sweep": benchkit.CACHE_SWEEP, "kinds": {}})
    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=benchkit.cache_sweep(ctx))

    def clean(*results):
        return all(int(r["status"].abs().sum().item()) == 0 for r in results)

    ok = True
    for kind in args.kinds.split(","):
        e = KINDS[kind]
        d_in = make(torch, kind, n)
        kres = {"elem_bytes": e, "items": {}}
        for kib in [int(x) for x in args.item_kib.split(",")]:
            item = kib << 10
            count = n // item
            sizes = [item] * count
            hists = ctx.histogram_batch_planes(d_in, e, sizes=sizes, max_item_bytes=item, flags=ghf.HIST_COVER_ALL)
            codes = ctx.build_codes(hists)
            d_mask = ctx.batch_planes_raw_auto(hists, codes)
            ctx.sync()
            mask = int(d_mask.item())

            def whole(raw):
                """one form of the batch, compressed and decoded through every decoder, checked against the input"""
                idx = ctx.batch_index_alloc(count * e, item // e)
                c = ctx.compress_batch_planes_shared(d_in, codes, e, sizes=sizes, max_item_bytes=item, index=idx, raw_planes=raw)
                rec = ctx.batch_seek_pack(idx, c["in_bytes"], elem_bytes=e)
                d = ctx.decode_batch_planes_shared(c["out_ptrs"], c["out_bytes"], codes, idx, c["n_elems"], e, out_stride=item, raw_planes=raw)
                s = ctx.decode_bodies_batch_planes_shared(c["out_ptrs"], c["out_bytes"], codes, e, out=ctx.empty_u8(n), caps=c["in_bytes"],
                                                          raw_planes=raw)
                k = ctx.decode_bodies_batch_planes_shared_seek(c["out_ptrs"], c["out_bytes"], rec["rec_ptrs"], rec["rec_bytes"], codes, e,
                                                               out=ctx.empty_u8(n), caps=c["in_bytes"], raw_planes=raw)
                ctx.sync()
                assert clean(c, d, s, k), (kind, kib, raw)
                assert torch.equal(d["out"][:n], d_in) and torch.equal(s["out"][:n], d_in) and torch.equal(k["out"][:n], d_in), (kind, kib, raw)
                return {"idx": idx, "c": c, "rec": rec, "d": d, "s": s, "k": k}

            par, frm = whole(None), whole(mask)

            call = benchkit.ok
            P = lambda t: t.data_ptr()

            def four(tag, w, raw):
                """the four calls over the buffers of `w`; raw None: the parents"""
                c, d, s, k, rec, idx = w["c"], w["d"], w["s"], w["k"], w["rec"], w["idx"]
                r = () if raw is None else (raw,)
                comp = L.ghf_compress_batch_planes_shared if raw is None else L.ghf_compress_batch_planes_forms
                live = L.ghf_decode_batch_planes_shared if raw is None else L.ghf_decode_batch_planes_forms
                bod = L.ghf_decode_bodies_batch_planes_shared if raw is None else L.ghf_decode_bodies_batch_planes_forms
                seek = L.ghf_decode_bodies_batch_planes_shared_seek if raw is None else L.ghf_decode_bodies_batch_planes_forms_seek
                return [
                    ("c" + tag, lambda: call(comp(ctx.h, P(c["in_ptrs"]), P(c["in_bytes"]), item, count, e, P(codes), *r, P(c["out_ptrs"]),
                                                  P(c["out_caps"]), P(c["out_bytes"]), C.byref(idx), P(c["status"])))),
                    ("d" + tag, lambda: call(live(ctx.h, P(c["out_ptrs"]), P(c["out_bytes"]), P(codes), C.byref(idx), P(c["n_elems"]), count, e,
                                                  *r, P(d["out_ptrs"]), P(d["out_caps"]), P(d["out_bytes"]), P(d["status"])))),
                    ("s" + tag, lambda: call(bod(ctx.h, P(c["out_ptrs"]), P(c["out_bytes"]), P(codes), count, e, *r, P(s["out_ptrs"]),
                                                 P(s["out_caps"]), P(s["out_bytes"]), P(s["status"])))),
                    ("k" + tag, lambda: call(seek(ctx.h, P(c["out_ptrs"]), P(c["out_bytes"]), P(rec["rec_ptrs"]), P(rec["rec_bytes"]), P(codes),
                                                  count, e, *r, P(k["out_ptrs"]), P(k["out_caps"]), P(k["out_bytes"]), P(k["status"])))),
                ]

            # the raw_planes == 0 calls work on the parent's buffers: they write the same bytes
            variants = four("p", par, None) + four("f", frm, mask) + four("0", par, 0)
            variants.append(("auto", lambda: call(L.ghf_batch_planes_raw_auto(ctx.h, P(hists), P(codes), e, P(d_mask)))))
            med, times = timed(variants)
            for w in (par, frm):
                assert clean(w["c"], w["d"], w["s"], w["k"]), (kind, kib)
                assert torch.equal(w["d"]["out"][:n], d_in) and torch.equal(w["s"]["out"][:n], d_in) and torch.equal(w["k"]["out"][:n], d_in)
            dense_bytes, forms_bytes = int(par["c"]["out_bytes"].sum().item()), int(frm["c"]["out_bytes"].sum().item())
            row = {
                "count": count,
                "raw_planes": mask,
                **benchkit.stats(times),
                "stored_bytes": {"input": n, "all_dense": dense_bytes, "forms": forms_bytes, "forms_over_dense": round(forms_bytes / dense_bytes, 6)},
                "forms_over_parent": {x: round(med[x + "f"] / med[x + "p"], 4) for x in PAIRS},
                "mask0_over_parent": {x: round(med[x + "0"] / med[x + "p"], 4) for x in PAIRS},
            }
            if kind != "uniform_bytes":
                row["bodies_decode_faster_than_parent"] = med["sf"] < med["sp"]
                ok = ok and row["bodies_decode_faster_than_parent"]
            kres["items"]["%dKiB" % kib] = row
            benchkit.progress({kind: {"%dKiB" % kib: row}})
            ctx.batch_index_free(par["idx"])
            ctx.batch_index_free(frm["idx"])
            del par, frm, variants
        res["kinds"][kind] = kres
        del d_in
    res["pairs"] = PAIRS
    res["required_bodies_decode_faster_on_typed_inputs"] = ok
    ctx.close()
    benchkit.write(res, args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
