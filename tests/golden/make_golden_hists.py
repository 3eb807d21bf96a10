#!/usr/bin/env python3
"""Generate tests/golden/golden_hists.json by running the COMPILED REFERENCE (oracle/_ref/ref_glzip, `make -C oracle
ref`) on the synthesised histograms of tests/hist_families.py that are small enough to exist as a byte stream (needs the
reference tree).  Committed: data only.  Every family entry whose 257 counts sum to at most 65 536 is materialised with
datagen.counts_to_bytes(h[:256], seed=<entry number>) and recorded with its label, the SHA-256 of those bytes, and the
size / SHA-256 of what the reference wrote:
  crs2 : `c`  (Compressor<CanonicalHuffEncoder<>>)
  crs  : `nc` (Compressor<NormalHuffEncoder<>>), where at least two byte values are live
plus one SHA-256 over the whole family's packed int64 counts, so that a drifting generator fails before anything else.

    python tests/golden/make_golden_hists.py
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hist_families as hf  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def run(td, data, enc):
    fin, fenc = os.path.join(td, "x.bin"), os.path.join(td, "x.enc")
    data.tofile(fin)
    orc.ref_run([enc, fin, fenc])
    e = np.fromfile(fenc, dtype=np.uint8)
    return {"ref_bytes": int(e.size), "ref_sha256": sha(e)}


def main():
    orc.build()
    assert orc.have_ref(), "oracle/_ref/ref_glzip missing: run `make -C oracle ref` where the reference tree exists"
    out = {"_generator": "tests/golden/make_golden_hists.py", "_reference": "chenghuige/golden-huffman",
           "_compiler": os.popen("g++ --version").read().splitlines()[0],
           "family_entries": len(hf.family()), "family_sha256": hf.family_sha256(), "pin_total": hf.PIN_TOTAL, "entries": []}
    with tempfile.TemporaryDirectory() as td:
        for i, label, h in hf.pinned():
            data = hf.materialise(i, h)
            e = {"entry": i, "label": label, "n": int(data.size), "input_sha256": sha(data), "crs2": run(td, data, "c")}
            if hf.n_live(h) >= 2:
                e["crs"] = run(td, data, "nc")
            out["entries"].append(e)
    with open(os.path.join(HERE, "golden_hists.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
