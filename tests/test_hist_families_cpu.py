"""CPU: the synthesised histograms of tests/hist_families.py and the oracle on them.  No GPU, no reference binary.

The oracle (oracle/huff_oracle.c) is the yardstick tests/test_gpu_code_builders.py holds every code builder to, so it is
itself held here (a) to what the COMPILED REFERENCE wrote for every family entry small enough to exist as a byte stream
(tests/golden/golden_hists.json, written by tests/golden/make_golden_hists.py) and (b), on every entry, to plain
references on Python integers: a heapq Huffman for the cost of the unlimited code, a package-merge for the cost of the
32-bit-limited one (PARITY UNPINNED for the limited tables: the reference has no such code), Kraft's sum, monotonicity."""
import hashlib
import heapq
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import hist_families as hf
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


@pytest.fixture(scope="module")
def golden_hists():
    with open(os.path.join(HERE, "golden", "golden_hists.json")) as f:
        return json.load(f)


def test_the_family_has_not_drifted(golden_hists):
    fam = hf.family()
    assert len(fam) == golden_hists["family_entries"] <= 1500
    assert hf.family_sha256() == golden_hists["family_sha256"]
    assert len({label for label, _, _ in fam}) == len(fam)
    for label, h, kind in fam:
        assert h.dtype == np.int64 and h.shape == (257,) and h[256] == 1, label
        assert (kind == "out_of_domain") == (hf.total(h) >= 1 << 55), label
    # large and small heaps alternate (hist_families: launch order)
    live = [hf.n_live(h) for _, h, _ in fam]
    assert all(live[i] >= live[i + 1] for i in range(0, len(live) - 1, 2))
    assert all(live[i] <= live[i + 1] for i in range(1, len(live) - 1, 2))


def test_oracle_equals_the_compiled_reference_on_every_small_entry(golden_hists):
    fam = hf.family()
    want = sum(1 for _, h, kind in fam if hf.total(h) <= hf.PIN_TOTAL)
    assert want >= 512 + 156  # all of ties at c = 1, near-ties over {1, 2, 3}
    visited = with_crs = 0
    for g in golden_hists["entries"]:
        label, h, kind = fam[g["entry"]]
        assert label == g["label"] and kind == "fits" and hf.total(h) <= hf.PIN_TOTAL
        data = hf.materialise(g["entry"], h)
        assert data.size == g["n"] == hf.total(h) - 1 and sha(data) == g["input_sha256"], label
        crs2 = orc.compress(data)
        assert (crs2.size, sha(crs2)) == (g["crs2"]["ref_bytes"], g["crs2"]["ref_sha256"]), label
        assert ("crs" in g) == (hf.n_live(h) >= 2), label
        if "crs" in g:
            crs = orc.crs_compress(data)
            assert (crs.size, sha(crs)) == (g["crs"]["ref_bytes"], g["crs"]["ref_sha256"]), label
            with_crs += 1
        visited += 1
    assert visited == want == len(hf.pinned()) == len({g["entry"] for g in golden_hists["entries"]})
    assert with_crs == sum(1 for _, _, h in hf.pinned() if hf.n_live(h) >= 2)


# ---- plain references on Python integers ----
def huffman_cost(counts):
    """sum of count * length of an optimal prefix code = the sum of all merged weights"""
    q = [int(c) for c in counts if c]
    heapq.heapify(q)
    cost = 0
    while len(q) > 1:
        w = heapq.heappop(q) + heapq.heappop(q)
        cost += w
        heapq.heappush(q, w)
    return cost


def package_merge_cost(counts, limit):
    """cost of an optimal prefix code with no length above `limit` (Larmore & Hirschberg): `limit` rounds of "pair the
    list up into packages and merge them with the leaves"; the 2n - 2 lightest items of the last list weigh the cost"""
    leaves = sorted(int(c) for c in counts if c)
    items = []
    for _ in range(limit):
        items = sorted(leaves + [items[2 * i] + items[2 * i + 1] for i in range(len(items) // 2)])
    return sum(items[: 2 * len(leaves) - 2])


def check_code(label, h, code):
    counts = [int(c) for c in h]
    length = list(code.length)
    assert all((c != 0) == (l != 0) for c, l in zip(counts, length)), label
    num = {}
    for l in length:
        if l:
            num[l] = num.get(l, 0) + 1
    assert sum(Fraction(n, 1 << l) for l, n in num.items()) == 1, label
    assert code.max_len == max(length) and code.min_len == min(l for l in length if l), label
    longest_above = 0  # a larger count never has a longer code
    by_count = {}
    for c, l in zip(counts, length):
        if c:
            by_count.setdefault(c, []).append(l)
    for c in sorted(by_count, reverse=True):
        assert min(by_count[c]) >= longest_above, label
        longest_above = max(longest_above, max(by_count[c]))
    return sum(c * l for c, l in zip(counts, length))


def test_oracle_against_integer_references_on_every_entry():
    n_fits = n_deep = 0
    for label, h, kind in hf.family():
        if kind == "fits":
            code = orc.build_code(h)  # (raises if the entry is not what its kind says)
            assert code.max_len <= 32, label
            assert check_code(label, h, code) == huffman_cost(h), label
            n_fits += 1
        elif kind == "deep":
            with pytest.raises(ValueError, match="rc=-2"):
                orc.build_code(h)
            code = orc.build_code_limited(h, 32)
            assert code.max_len == 32, label
            cost = check_code(label, h, code)
            assert cost == package_merge_cost(h, 32), label
            assert cost >= huffman_cost(h), label
            n_deep += 1
    assert n_fits > 1300 and n_deep >= 13
    by_label = {label: (h, kind) for label, h, kind in hf.family()}
    # the two entries that guard the classification: exactly 32 bits, and a long chain that 216 ones lift to 24
    assert orc.build_code(by_label["chain/fib2x/k45/first"][0]).max_len == 32
    assert by_label["deep/fib40+216ones"][1] == "fits" and orc.build_code(by_label["deep/fib40+216ones"][0]).max_len == 24
    assert hf.total(by_label["wide/total-2^55-555"][0]) == (1 << 55) - 555
    assert hf.total(by_label["wide/total-2^55-1"][0]) == (1 << 55) - 1
    assert hf.total(by_label["ood/total-2^55"][0]) == 1 << 55


def test_crs_extras_have_the_stated_depth():
    for label, h, expect in hf.crs_extras():
        assert h.shape == (256,)
        if expect in ("empty", "single"):
            assert np.count_nonzero(h) == (0 if expect == "empty" else 1)
            with pytest.raises(ValueError):
                orc.crs_tree(h)
            continue
        codes = [c for c in orc.crs_code_strings(orc.crs_tree(h)) if c]
        assert len(codes) == np.count_nonzero(h) and max(len(c) for c in codes) == expect, label
        assert sum(Fraction(1, 1 << len(c)) for c in codes) == 1, label  # complete ..
        s = sorted(codes)
        assert not any(b.startswith(a) for a, b in zip(s, s[1:])), label  # .. and prefix-free
