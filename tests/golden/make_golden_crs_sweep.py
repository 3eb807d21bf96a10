#!/usr/bin/env python3
"""Generate tests/golden/golden_crs_sweep.json: the pins of tests/crs_sweep.py (its digest, the depths of its pool, the trees
per depth and per kind, the item and piece counts, the parts of the pieces ids, what it leaves out) and -- where the
COMPILED REFERENCE is present (oracle/_ref/ref_glzip, `make -C oracle ref`; needs the reference tree) -- what the reference's own NormalHuffDecoder reads out of a sample
of the sweep's files (`ref_glzip nd`): per file the SHA-256 of the decoded bytes, or "failed: ..." with what the reference
did instead.  The sample: the first and the last item of the first tree of every depth, of every hand-built tree and of every
mirror of depth 33 or more.  Committed: recorded results only.

    python tests/golden/make_golden_crs_sweep.py
"""
import collections
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import crs_sweep as zs  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def sample():
    seen, out = set(), []
    for t in zs.pool():
        if t.max_len not in seen or t.kind == "hand" or (t.kind == "mirror" and t.max_len >= 33):
            seen.add(t.max_len)
            its = zs.items(t)
            out += [its[0], its[-1]]
    return out


def ref_decode(td, it):
    fin, fout = os.path.join(td, "x.crs"), os.path.join(td, "x.out")
    it.file.tofile(fin)
    if os.path.exists(fout):
        os.remove(fout)
    try:
        orc.ref_run(["nd", fin, fout])
    except subprocess.TimeoutExpired:
        return "failed: timeout"
    except subprocess.CalledProcessError as e:
        return "failed: exit status %d" % e.returncode
    if not os.path.exists(fout):
        return "failed: no output"
    return sha(np.fromfile(fout, dtype=np.uint8))


def main():
    orc.build()
    pool = zs.pool()
    per_depth = collections.Counter(t.max_len for t in pool)
    out = {"_generator": "tests/golden/make_golden_crs_sweep.py", "_reference": "chenghuige/golden-huffman",
           "per_group": zs.PER_GROUP, "sha256": zs.sha256(), "pool_size": len(pool),
           "items": sum(len(zs.items(t)) for t in pool), "groups": zs.groups(),
           "group_sizes": [per_depth[d] for d in zs.groups()],
           "pieces": sum(it.n_pieces() for t in pool for it in zs.items(t)),
           "piece_parts": [zs.piece_parts(d) for d in zs.groups()],
           "kinds": dict(sorted(collections.Counter(t.kind for t in pool).items())), "left_out": zs.left_out()}
    if orc.have_ref():
        out["_compiler"] = os.popen("g++ --version").read().splitlines()[0]
        with tempfile.TemporaryDirectory() as td:
            out["ref_nd"] = {repr(it): ref_decode(td, it) for it in sample()}
    else:  # keep what an earlier run with the reference recorded
        with open(os.path.join(HERE, "golden_crs_sweep.json")) as f:
            out["ref_nd"] = json.load(f)["ref_nd"]
    with open(os.path.join(HERE, "golden_crs_sweep.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
