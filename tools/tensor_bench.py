#!/usr/bin/env python3
"""What one stored object per typed tensor costs, measured.  Not bench.py: this times typed elements.
Data: --mib (256 and 1024) MiB of seeded standard-normal bf16 and fp32 stored by themselves with GHF_RAW_AUTO, and fp32
against itself after a step of 1e-5 with GHF_RAW_AUTO | GHF_SPARSE_AUTO.  Per data set it times

  copy_nt          ghf_copy_d2d(non_temporal = 1) of as many bytes as the container's stream region: the yardstick
  pack             ghf_tensor_pack on the outputs of ghf_compress_planes_forms: the seek tables, the rank copies, k_tensor_pack
  compress_tensor  ghf_compress_tensor: the one call
  today_route      the only route there was: ghf_compress_planes_forms with side-cars and rank tables, one ghf_seek_pack per
                   stream, the copy of the sizes to the host and the wait for it, one ghf_copy_d2d per section
  forms_alone      ghf_compress_planes_forms with side-cars and rank tables, nothing behind it
  open             ghf_tensor_open from the 768 head bytes (the close is outside the events)
  tensor_decode    ghf_tensor_decode                     | forms_decode   ghf_decode_planes_forms with live side-cars
  tensor_gather    ghf_tensor_gather, 1024 rows of 4096  | forms_gather   ghf_decode_planes_gather_forms on the same container

REQUIRED, in every run: (1) the bytes k_tensor_pack reads plus writes (twice the stream region), over the time of the WHOLE
pack call -- which also holds the table launches, so the kernel alone is no slower -- reach 0.5 of the rate of copy_nt;
(2) compress_tensor takes less time than today_route.  Everything else is recorded.  The container is checked once: it
parses, and a decode of it gives the tensor back.

Recipe: tools/benchkit.py, with the cache sweep.  Prints one JSON document and writes it to --out."""
import argparse
import ctypes as C
import functools
import importlib
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

DATA = [("bf16", 2, None), ("fp32", 4, None), ("fp32_step_1e-5", 4, 1e-5)]
ROWS, ROW_ELEMS = 1024, 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="256,1024")
    ap.add_argument("--seed", type=int, default=7)
    benchkit.add_args(ap, reps=9, warmup=2, out=os.path.join(ROOT, "profiles", "planes", "tensor_bench.json"))
    args = ap.parse_args()

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    gt = importlib.import_module("golden_huffman_amd.ghf_tensor")
    assert torch.cuda.is_available(), "tensor_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    res = benchkit.envelope(torch, ghf, args, "ms (device events), medians")
    res.update({"seed": args.seed, "cache_sweep": benchkit.CACHE_SWEEP,
                "required": ["2 * stream region / pack >= 0.5 * the rate of copy_nt", "compress_tensor < today_route"], "runs": []})
    sweep = benchkit.cache_sweep(ctx)
    opened = []  # what the `open` variant opened and nobody has closed yet

    def close_opened():
        while opened:
            ctx.sync()
            opened.pop().close()

    def close_then_sweep():
        """the close of an opened container stays outside every pair of events: it runs in front of the next sample's sweep"""
        close_opened()
        sweep()

    timed = functools.partial(benchkit.timed, reps=args.reps, warmup=args.warmup, sync=ctx.sync, sweep=close_then_sweep)

    for mib in [int(x) for x in args.mib.split(",")]:
        for name, e, step in DATA:
            nbytes = mib << 20
            n = nbytes // e
            if step is None:
                d_new, d_base = benchkit.normal_elems(torch, nbytes, e, args.seed), None
            else:
                d_new, d_base = benchkit.normal_pair_reseeded(torch, nbytes, e, step, args.seed)
            raw_ask, sparse_ask = ghf.RAW_AUTO, (ghf.SPARSE_AUTO if step is not None else 0)
            flags = gt.DELTA if d_base is not None else 0
            cap = gt.bound(n, e)
            d_cont, d_cbytes = ctx.empty_u8(cap), torch.zeros(1, dtype=torch.int64, device="cuda")
            d_cont2 = ctx.empty_u8(cap)

            # the outputs of ghf_compress_planes_forms, kept for pack, forms_decode and forms_gather
            r = ctx.compress_planes_forms(d_new, e, raw_planes=raw_ask, sparse_planes=sparse_ask, d_base=d_base, indexes=True, ranks=True)
            ctx.sync()
            raw, sparse, slot, rsb = r["raw_planes"], r["sparse_planes"], r["slot_bytes"], r["rank_slot_bytes"]
            sizes = [int(v) for v in r["out_bytes"].cpu().tolist()]
            streams = [r["out"][j * slot : (j + 1) * slot] for j in range(2 * e)]
            ranks = [r["ranks"][p * rsb : (p + 1) * rsb] for p in range(e)]

            def v_pack():
                gt.pack(ctx, streams, r["out_bytes"], r["indexes"], ranks, raw, sparse, r["n_vals"], n, e, flags=flags, d_container=d_cont,
                        cap=cap, nbytes=d_cbytes)

            def v_compress():
                gt.compress_tensor(ctx, d_new, e, raw_planes=raw_ask, sparse_planes=sparse_ask, d_base=d_base, n_elems=n, d_container=d_cont2,
                                   cap=cap, nbytes=d_cbytes)

            v_compress()
            ctx.sync()
            total = int(d_cbytes.item())
            info = gt.parse(d_cont2[: gt.HEAD_BYTES].cpu().numpy(), total)
            assert (info.raw_planes, info.sparse_planes, info.n_elems) == (raw, sparse, n)
            secs = info.sections()
            streams_off = min(o for o, b in secs[gt.STREAMS : gt.TABLES] if b)
            region = total - streams_off
            v_pack()
            ctx.sync()
            assert int(d_cbytes.item()) == total and torch.equal(d_cont[:total], d_cont2[:total]), "pack and compress_tensor differ"

            # today's route: forms + a seek_pack per stream + the sizes to the host + a copy per section
            rt = {"out": ctx.empty_u8(slot * 2 * e), "codes": torch.zeros((2 * e, C.sizeof(ghf.Code)), dtype=torch.uint8, device="cuda"),
                  "out_bytes": torch.zeros(2 * e, dtype=torch.int64, device="cuda"), "ranks": ctx.empty_u8(rsb * e)}
            d_tabs = [ctx.empty_u8(ghf.seek_bytes(n) + 16) for _ in range(2 * e)]
            d_cont3 = ctx.empty_u8(cap)
            h_sizes = torch.zeros(2 * e, dtype=torch.int64).pin_memory()

            def v_today():
                q = ctx.compress_planes_forms(d_new, e, raw_planes=raw_ask, sparse_planes=sparse_ask, d_base=d_base, d_out=rt["out"],
                                              slot_bytes=slot, d_codes=rt["codes"], indexes=True, d_ranks=rt["ranks"], rank_slot_bytes=rsb,
                                              out_bytes=rt["out_bytes"])
                coded = [j for j in range(2 * e) if q["indexes"][j].d_chunk_bit]
                for j in coded:
                    ctx.seek_pack(q["indexes"][j], d_table=d_tabs[j])
                h_sizes.copy_(rt["out_bytes"], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                at = gt.HEAD_BYTES
                for j in coded:
                    tb = ghf.seek_bytes(q["indexes"][j].n_symbols)
                    ctx.copy_d2d(d_cont3[at : at + tb], d_tabs[j], tb)
                    at += (tb + 15) & ~15
                for p in range(e):
                    if q["sparse_planes"] >> p & 1:
                        rb = ghf.sparse_rank_bytes(n)
                        ctx.copy_d2d(d_cont3[at : at + rb], rt["ranks"][p * rsb : p * rsb + rb], rb)
                        at += (rb + 15) & ~15
                for j in range(2 * e):
                    sz = int(h_sizes[j])
                    if sz:
                        ctx.copy_d2d(d_cont3[at : at + sz], rt["out"][j * slot : j * slot + sz], sz)
                        at += (sz + 15) & ~15
                ctx.planes_index_free(q["indexes"])

            def v_forms():
                q = ctx.compress_planes_forms(d_new, e, raw_planes=raw_ask, sparse_planes=sparse_ask, d_base=d_base, d_out=rt["out"],
                                              slot_bytes=slot, d_codes=rt["codes"], indexes=True, d_ranks=rt["ranks"], rank_slot_bytes=rsb,
                                              out_bytes=rt["out_bytes"])
                ctx.planes_index_free(q["indexes"])

            d_copy_src, d_copy_dst = ctx.empty_u8(region), ctx.empty_u8(region)

            def v_copy():
                ctx.copy_d2d(d_copy_dst, d_copy_src, region, non_temporal=True)

            # the decode side, on the container compress_tensor wrote
            head = d_cont2[: gt.HEAD_BYTES].cpu().numpy()

            def v_open():
                opened.append(gt.open(ctx, d_cont2, total, head=head))

            t = gt.open(ctx, d_cont2, total, head=head)
            ctx.sync()
            d_out, d_nbytes = ctx.empty_u8(nbytes), torch.zeros(1, dtype=torch.int64, device="cuda")
            gi = torch.Generator(device="cuda")
            gi.manual_seed(args.seed + 2)
            d_index = torch.randint(0, n // ROW_ELEMS, (ROWS,), generator=gi, device="cuda", dtype=torch.int64)
            d_rows, d_status = ctx.empty_u8(ROWS * ROW_ELEMS * e), torch.zeros(ROWS, dtype=torch.int32, device="cuda")

            def v_tdecode():
                t.decode(d_base=d_base, d_out=d_out, nbytes=d_nbytes)

            def v_fdecode():
                ctx.decode_planes_forms(streams, sizes, r["codes"], raw, sparse, r["n_vals"], n, e, indexes=r["indexes"], d_base=d_base,
                                        d_out=d_out, nbytes=d_nbytes)

            def v_tgather():
                t.gather(d_index, ROW_ELEMS, d_base=d_base, d_out=d_rows, d_row_status=d_status)

            c_streams = [d_cont2[o : o + b] if b else None for o, b in secs[gt.STREAMS : gt.TABLES]][: 2 * e]
            c_tables = [d_cont2[o : o + b] if b else None for o, b in secs[gt.TABLES : gt.RANKS]][: 2 * e]
            c_infos = [ghf.seek_parse(x.cpu().numpy()) if x is not None else None for x in c_tables]
            c_ranks = [None] * e
            for p in range(e):
                o, b = secs[gt.RANKS + p]
                if b:
                    c_ranks[p] = (ghf.sparse_rank_parse(d_cont2[o : o + b].cpu().numpy()), d_cont2[o : o + b])

            def v_fgather():
                ctx.decode_planes_gather_forms(c_streams, [b for _, b in secs[: 2 * e]], r["codes"], raw, sparse, c_ranks, n, e, d_index,
                                               ROW_ELEMS, infos=c_infos, d_tables=c_tables, d_base=d_base, d_out=d_rows, d_row_status=d_status)

            for fn, what in ((v_tdecode, "tensor_decode"), (v_fdecode, "forms_decode")):
                d_out.zero_()
                fn()
                ctx.sync()
                assert torch.equal(d_out, d_new), what
            want = torch.index_select(d_new.view(-1, ROW_ELEMS * e), 0, d_index).view(-1)
            for fn, what in ((v_tgather, "tensor_gather"), (v_fgather, "forms_gather")):
                d_rows.zero_()
                fn()
                ctx.sync()
                assert torch.equal(d_rows, want) and int(d_status.abs().sum().item()) == 0, what

            med, times = timed([("copy_nt", v_copy), ("pack", v_pack), ("compress_tensor", v_compress), ("today_route", v_today),
                                ("forms_alone", v_forms), ("open", v_open), ("tensor_decode", v_tdecode), ("forms_decode", v_fdecode),
                                ("tensor_gather", v_tgather), ("forms_gather", v_fgather)])
            close_opened()
            copy_rate = 2 * region / med["copy_nt"] / 1e6
            pack_rate = 2 * region / med["pack"] / 1e6
            run = {"data": name, "mib": mib, "elem_bytes": e, "n_elems": n, "raw_planes": raw, "sparse_planes": sparse,
                   "bytes": {"tensor": nbytes, "container": total, "stream_region": region, "slots_2E": 2 * e * slot},
                   "container_over_tensor": round(total / nbytes, 4), "container_over_slots": round(total / (2 * e * slot), 4),
                   **benchkit.stats(times),
                   "copy_nt_gb_per_s": round(copy_rate, 1), "pack_gb_per_s": round(pack_rate, 1), "pack_over_copy_rate": round(pack_rate / copy_rate, 3),
                   "compress_tensor_over_today_route": round(med["compress_tensor"] / med["today_route"], 3),
                   "compress_tensor_over_forms_alone": round(med["compress_tensor"] / med["forms_alone"], 3),
                   "tensor_decode_over_forms_decode": round(med["tensor_decode"] / med["forms_decode"], 3),
                   "tensor_gather_over_forms_gather": round(med["tensor_gather"] / med["forms_gather"], 3),
                   "meets_required": {"pack_rate": pack_rate >= 0.5 * copy_rate, "one_call": med["compress_tensor"] < med["today_route"]}}
            res["runs"].append(run)
            benchkit.progress(run)
            t.close()
            ctx.planes_index_free(r["indexes"])
            del d_new, d_base, d_cont, d_cont2, d_cont3, r, rt, d_tabs, d_out, d_rows, streams, ranks, c_streams, c_tables, c_ranks, t
            del d_copy_src, d_copy_dst, want
            torch.cuda.empty_cache()
    res["meets_required"] = all(all(run["meets_required"].values()) for run in res["runs"])
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
