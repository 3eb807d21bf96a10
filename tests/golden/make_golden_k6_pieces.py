#!/usr/bin/env python3
"""Generate tests/golden/golden_k6_pieces.json: the pins of tests/k6_pieces.py -- one digest over every expected
(landing, n_symbols, has_end_mark) and every image, its codes, and the census of its tiers.  Recorded results only.

    python tests/golden/make_golden_k6_pieces.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import k6_pieces as kp  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def main():
    orc.build()
    census = kp.census()
    out = {"_generator": "tests/golden/make_golden_k6_pieces.py", "sha256": kp.sha256(), "codes": [c.label for c in kp.codes()],
           "census": census, "cases": sum(census.values())}
    with open(os.path.join(HERE, "golden_k6_pieces.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
