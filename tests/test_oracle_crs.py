"""CPU: the `.crs` restatement (NormalHuffEncoder/Decoder, oracle/huff_oracle.c) against the golden
vectors the compiled reference produced (tests/golden/golden_crs.json, generator tests/golden/make_golden_crs.py)."""
import base64
import hashlib
import json
import os

import numpy as np
import pytest

from cases import CRS_CASES as CASES, sweep_crs_inputs
from oracle import oracle as orc
import datagen as dg


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _sweeps():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_sweeps.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_crs_oracle_matches_reference_fixture(golden_crs, name):
    g = golden_crs[name]
    data = CASES[name]()
    assert data.size == g["n"] and sha(data) == g["input_sha256"], "input generator drifted"
    if "undefined" in g:
        with pytest.raises(ValueError):
            orc.crs_compress(data)
        return
    tree = orc.crs_tree(np.bincount(data, minlength=256))
    assert orc.crs_code_strings(tree) == g["codes"]
    tb = orc.crs_tree_bytes(tree)
    assert tb.size == g["tree_bytes"] and bytes(tb) == base64.b64decode(g["tree_b64"])
    crs = orc.crs_compress(data)
    assert crs.size == g["crs_bytes"] and sha(crs) == g["crs_sha256"]
    assert [int(crs[tb.size]), int(crs[tb.size + 1])] == g["prefix"]
    if "crs_b64" in g:
        assert bytes(crs) == base64.b64decode(g["crs_b64"])
    back = orc.crs_decompress(crs, cap=data.size + 8)
    assert sha(back) == g["decoded_sha256"] and np.array_equal(back, data)


def test_crs_worked_example():
    # aaaabbc: c(1)+b(2) -> 3, then a(4) is popped first (3 > ... no: 3 < 4), so the parent is (3-node, a):
    # a = "1", c = "00", b = "01"; 4*1 + 2*2 + 1*2 = 10 bits -> one whole byte + 2 bits, left_bits = 6
    data = np.frombuffer(b"aaaabbc", dtype=np.uint8)
    crs = orc.crs_compress(data)
    codes = orc.crs_code_strings(orc.crs_tree(np.bincount(data, minlength=256)))
    assert (codes[ord("a")], codes[ord("b")], codes[ord("c")]) == ("1", "01", "00")
    assert bytes(crs[:10]) == bytes([255, 255, 255, 255, 0, ord("c"), 0, ord("b"), 0, ord("a")])
    assert bytes(crs[10:]) == bytes([6, 0b00000000, 0b11110101])  # 1111 01 01 | 00 + six zero bits


def test_crs_oracle_rejects_what_the_reference_leaves_undefined():
    with pytest.raises(ValueError):
        orc.crs_compress(np.zeros(0, dtype=np.uint8))
    with pytest.raises(ValueError):
        orc.crs_compress(np.full(100, 7, dtype=np.uint8))
    good = orc.crs_compress(np.frombuffer(b"hello world", dtype=np.uint8))
    with pytest.raises(ValueError):
        orc.crs_decompress(good[:5])  # truncated tree
    bad = good.copy()
    bad[0] = 0  # root claims to be a leaf
    with pytest.raises(ValueError):
        orc.crs_decompress(bad)


def test_crs_random_inputs_against_the_compiled_reference():
    """fresh random inputs: the oracle's .crs == what the compiled reference wrote (tests/golden/golden_sweeps.json,
    generator tests/golden/make_golden_sweeps.py); the reference's decoder read those same bytes back to the input"""
    recs = _sweeps()["crs"]
    inputs = sweep_crs_inputs()
    assert len(recs) == len(inputs) > 20
    for (label, data), g in zip(inputs, recs):
        assert g["label"] == label and data.size == g["n"] and sha(data) == g["input_sha256"], "input generator drifted"
        mine = orc.crs_compress(data)
        assert mine.size == g["ref_bytes"] and sha(mine) == g["ref_sha256"], label
        assert g["ref_decoded_sha256"] == sha(data), label  # the reference reads what the oracle wrote
        assert np.array_equal(orc.crs_decompress(mine), data), label
