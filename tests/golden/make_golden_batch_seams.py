#!/usr/bin/env python3
"""Generate tests/golden/golden_batch_seams.json: the pins of tests/batch_seams.py -- its digest, its codes, the census of
its tiers, what cannot exist by name, the shapes and carries of the items with codes of their own, and the two mutant tables
of tests/test_batch_seams_cpu.py (per code: the carries of the `ones` fill at which each packer mutant changes a byte; the
items at which each decoder mutant does, of those that could show it).  Recorded results only.

    python tests/golden/make_golden_batch_seams.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import batch_seams as bs  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def own_codes():
    seen, shapes = {}, {}
    for it in bs.own_items():
        key = it.base.label
        shapes[key] = [int(it.code.min_len), int(it.code.max_len), it.lead % 128]
        a, b = it.carries()
        seen.setdefault(key, [set(), set()])
        seen[key][0].add(a)
        seen[key][1].add(b)
    return {k: shapes[k] + [len(v[0]), len(v[1])] for k, v in seen.items()}


def main():
    orc.build()
    out = {"_generator": "tests/golden/make_golden_batch_seams.py", "sha256": bs.sha256(),
           "codes": [bs.label(c) for c in bs.codes()], "census": {k: list(v) for k, v in bs.census().items()},
           "unreachable": bs.unreachable(), "own_codes": own_codes(), "pack_mutants": bs.pack_mutant_table(),
           "decode_mutants": bs.decode_mutant_table()}
    with open(os.path.join(HERE, "golden_batch_seams.json"), "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
