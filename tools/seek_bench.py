#!/usr/bin/env python3
"""What the seek table buys, measured (DESIGN.md "Seekable .crs2").  Not bench.py: this times only the decode-side
paths a persisted .crs2 can take.  On `--mib` MiB of uniform and of zipf bytes:

  a  ghf_decode with a live side-car                          (what a stream decodes at while its writer still holds the index)
  b  ghf_seek_expand + ghf_decode                             (a stream opened with its .crs2.seek table)
  c  ghf_decode(index = NULL)                                 (the K6 path a persisted stream takes without a table)
  d  ghf_decode_range of 1 MiB, table-driven, at an unaligned offset in the middle, 16-byte aligned output
  plus  b_expand (ghf_seek_expand alone), d_live (the same range from a live side-car) and d_coaligned (output pointer
        congruent to `first` modulo 16, so that K7 stores 16 bytes at a time).

Every variant is checked against the input once.  Recipe: tools/benchkit.py, without the cache sweep.  Prints one JSON
document; --out also writes it to a file."""
import argparse
import os
import sys

import benchkit

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--kinds", default="uniform,zipf")
    benchkit.add_args(ap, reps=30, warmup=3, out=None)
    args = ap.parse_args()

    import importlib

    import torch

    import pkgload

    pkg = pkgload.load()
    ghf = pkg.ghf
    synth = importlib.import_module("golden_huffman_amd.synth")
    assert torch.cuda.is_available(), "seek_bench needs the GPU: there is nothing to fall back to"
    ctx = ghf.Context(0)
    n = args.mib << 20
    res = benchkit.envelope(torch, ghf, args, "ms (device events)")
    res.update({"mib": args.mib, "kinds": {}})
    for kind in args.kinds.split(","):
        d_in = synth.make(torch, kind, n, offset=0, device="cuda")
        idx = ctx.index_alloc(n)
        d_stream, nbytes, d_code = ctx.compress(d_in, index=idx)
        ctx.sync()
        nb = int(nbytes.item())
        d_table = ctx.seek_pack(idx)
        ctx.sync()
        info = ghf.seek_parse(d_table.cpu().numpy())
        idx2 = ctx.index_alloc(n)
        d_out = ctx.empty_u8(n + 64)
        first, count = n // 2 + 1234 + 7, 1 << 20
        r_buf = ctx.empty_u8(count + 64)
        r_out = r_buf[:count]
        r_co = r_buf[first % 16 : first % 16 + count]
        assert first % 4096 and first % 16 and r_out.data_ptr() % 16 == 0 and (r_co.data_ptr() - first) % 16 == 0

        def v_a():
            ctx.decode(d_stream, nb, d_code, idx, d_out=d_out)

        def v_b():
            ctx.seek_expand(info, d_table, d_stream, nb, d_code, index=idx2)
            ctx.decode(d_stream, nb, d_code, idx2, d_out=d_out)

        def v_b_expand():
            ctx.seek_expand(info, d_table, d_stream, nb, d_code, index=idx2)

        def v_c():
            ctx.decode(d_stream, nb, d_code, None, d_out=d_out)

        def v_d():
            ctx.decode_range(d_stream, nb, d_code, first, count, info=info, d_table=d_table, d_out=r_out)

        def v_d_live():
            ctx.decode_range(d_stream, nb, d_code, first, count, index=idx, d_out=r_out)

        def v_d_co():
            ctx.decode_range(d_stream, nb, d_code, first, count, info=info, d_table=d_table, d_out=r_co)

        variants = [("a", v_a), ("b", v_b), ("b_expand", v_b_expand), ("c", v_c), ("d", v_d), ("d_live", v_d_live), ("d_coaligned", v_d_co)]
        # correctness, once each (and the first warm-up)
        for name, fn in variants:
            d_out.zero_()
            r_buf.zero_()
            fn()
            ctx.sync()
            if name in ("a", "b", "c"):
                assert torch.equal(d_out[:n], d_in), (kind, name)
            elif name == "d_coaligned":
                assert torch.equal(r_co, d_in[first : first + count]), (kind, name)
            elif name != "b_expand":
                assert torch.equal(r_out, d_in[first : first + count]), (kind, name)
        med, times = benchkit.timed(variants, args.reps, args.warmup, ctx.sync)
        res["kinds"][kind] = {
            "stream_bytes": nb,
            "table_bytes": int(d_table.numel()),
            "range": {"first": first, "count": count},
            **benchkit.stats(times),
            "ratios": {"b_over_a": round(med["b"] / med["a"], 3), "c_over_b": round(med["c"] / med["b"], 3),
                       "d_over_a": round(med["d"] / med["a"], 3)},
            "b_lt_c": med["b"] < med["c"],
            "d_lt_a": med["d"] < med["a"],
        }
        ctx.index_free(idx)
        ctx.index_free(idx2)
        del d_in, d_stream, d_out, r_buf
    ctx.close()
    benchkit.write(res, args.out)


if __name__ == "__main__":
    main()
