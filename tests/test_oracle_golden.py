"""CPU: the oracle (oracle/huff_oracle.c) against the golden vectors the compiled reference produced
(tests/golden/golden.json, generator tests/golden/make_golden.py) -- every stage, bit-exact."""
import base64
import hashlib
import json
import os

import numpy as np
import pytest

from cases import CASES, sweep_crs2_inputs
from oracle import oracle as orc
import datagen as dg


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _sweeps():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_sweeps.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_matches_reference_fixture(golden, name):
    g = golden[name]
    data = CASES[name]()
    assert data.size == g["n"] and sha(data) == g["input_sha256"], "input generator drifted"
    hist = orc.histogram(data)
    assert hist.tolist() == g["hist"]
    code = orc.build_code(hist)
    d = code.as_dict()
    for k in ("length", "codeword", "symbol", "first_code", "start_pos", "min_len", "max_len"):
        assert d[k] == g[k], k
    hdr = orc.header_bytes(code)
    assert hdr.size == g["header_bytes"]
    assert bytes(hdr) == base64.b64decode(g["header_b64"])
    crs = orc.compress(data)
    assert crs.size == g["crs2_bytes"]
    assert sha(crs) == g["crs2_sha256"]
    assert sha(crs[hdr.size:]) == g["body_sha256"]
    assert bytes(crs[-8:]).hex() == g["body_tail_hex"]
    assert (orc.body_bits(hist, code) + 7) // 8 == crs.size - hdr.size
    if "crs2_b64" in g:
        assert bytes(crs) == base64.b64decode(g["crs2_b64"])
    back = orc.decompress(crs, cap=data.size + 8)
    assert sha(back) == g["decoded_sha256"] and np.array_equal(back, data)


def test_worked_example_from_survey():
    # SURVEY 8 "wire format": aaaabbc -> a=1,b=2,c=3,EOF=3; codes 1,01,000,001; header 1064 B; body F5 07
    data = np.frombuffer(b"aaaabbc", dtype=np.uint8)
    crs = orc.compress(data)
    dcode, hs = orc.parse_header(crs)
    assert hs == 1064 and bytes(crs[hs:]) == b"\xF5\x07"
    assert (dcode.min_len, dcode.max_len) == (1, 3)
    assert list(dcode.start_pos)[1:4] == [0, 1, 2] and list(dcode.first_code)[1:4] == [1, 1, 0]
    code = orc.build_code(orc.histogram(data))
    assert [code.length[ord(c)] for c in "abc"] + [code.length[256]] == [1, 2, 3, 3]
    assert [code.codeword[ord(c)] for c in "abc"] + [code.codeword[256]] == [1, 1, 0, 1]


def test_oracle_rejects_what_the_reference_leaves_undefined():
    with pytest.raises(ValueError):  # empty input: SURVEY 5.2
        orc.compress(np.zeros(0, dtype=np.uint8))
    with pytest.raises(ValueError):  # 33-bit codes: include/canonical_huff_encoder.h:43-44
        h = np.zeros(257, dtype=np.int64)
        h[:33] = dg.fib_counts(33)
        h[256] = 1
        orc.build_code(h)


def test_oracle_vs_compiled_reference_random_sweep():
    """fresh random inputs (not in the named cases): restatement == what the compiled reference wrote, byte for byte
    (tests/golden/golden_sweeps.json, generator tests/golden/make_golden_sweeps.py), and both decoders agree."""
    recs = _sweeps()["crs2"]
    inputs = sweep_crs2_inputs()
    assert len(recs) == len(inputs) == 40
    for (label, data), g in zip(inputs, recs):
        assert g["label"] == label and data.size == g["n"] and sha(data) == g["input_sha256"], "input generator drifted"
        mine = orc.compress(data)
        assert mine.size == g["ref_bytes"] and sha(mine) == g["ref_sha256"], label
        assert sha(orc.decompress(mine, cap=data.size + 8)) == g["ref_decoded_sha256"] == sha(data), label
