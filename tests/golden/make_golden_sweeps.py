#!/usr/bin/env python3
"""Generate tests/golden/golden_sweeps.json by running the COMPILED REFERENCE (oracle/_ref/ref_glzip, `make -C oracle
ref`) on the random sweeps of tests/golden/cases.py (needs the reference tree).  Committed: data only -- per input its
SHA-256, and the size / SHA-256 of what the reference wrote:
  crs2 : `c` (Compressor<CanonicalHuffEncoder<>>) and `d` of that file (Decompressor<CanonicalHuffDecoder<>>)
  crs  : `nc` (Compressor<NormalHuffEncoder<>>) and `nd` of that file (Decompressor<NormalHuffDecoder<>>)
  limited : `d` of the oracle's 32-bit length-limited .crs2 of a 33-deep input (the reference's decoder reads it)

    python tests/golden/make_golden_sweeps.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import oracle as orc  # noqa: E402
from cases import limited_stream_input, sweep_crs2_inputs, sweep_crs_inputs  # noqa: E402


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def run(td, data, enc, dec):
    fin, fenc, fde = (os.path.join(td, "x." + e) for e in ("bin", "enc", "de"))
    data.tofile(fin)
    orc.ref_run([enc, fin, fenc])
    e = np.fromfile(fenc, dtype=np.uint8)
    orc.ref_run([dec, fenc, fde])
    d = np.fromfile(fde, dtype=np.uint8)
    return {"n": int(data.size), "input_sha256": sha(data), "ref_bytes": int(e.size), "ref_sha256": sha(e),
            "ref_decoded_sha256": sha(d)}


def main():
    orc.build()
    assert orc.have_ref(), "oracle/_ref/ref_glzip missing: run `make -C oracle ref` where the reference tree exists"
    out = {"_generator": "tests/golden/make_golden_sweeps.py", "_reference": "chenghuige/golden-huffman",
           "_compiler": os.popen("g++ --version").read().splitlines()[0]}
    with tempfile.TemporaryDirectory() as td:
        out["crs2"] = [dict(run(td, data, "c", "d"), label=label) for label, data in sweep_crs2_inputs()]
        out["crs"] = [dict(run(td, data, "nc", "nd"), label=label) for label, data in sweep_crs_inputs()]
        data = limited_stream_input()
        crs = orc.compress_limited(data, 32)
        f = os.path.join(td, "lim.crs2")
        crs.tofile(f)
        orc.ref_run(["d", f, f + ".de"], timeout=300)
        out["limited"] = {"n": int(data.size), "input_sha256": sha(data), "stream_bytes": int(crs.size), "stream_sha256": sha(crs),
                          "ref_decoded_sha256": sha(np.fromfile(f + ".de", dtype=np.uint8))}
    with open(os.path.join(HERE, "golden_sweeps.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
