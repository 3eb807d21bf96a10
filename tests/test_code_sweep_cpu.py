"""CPU: what tests/code_sweep.py covers, pinned before any kernel runs, and its expectations held against the oracle's own
decoder and plain numpy.  No GPU.  The pins (tests/golden/golden_code_sweep.json) are those of the default draw of
code_sweep.PER_GROUP codes per group."""
import json
import os

import numpy as np
import pytest

import code_sweep as cs
import hist_families as hf
import range_worlds as rw
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "golden_code_sweep.json")) as f:
        return json.load(f)


def all_items():
    return [it for e in cs.pool() for it in cs.items(e)]


def test_the_sweep_has_not_drifted(pins):
    assert cs.PER_GROUP == 4 == pins["per_group"]
    assert cs.sha256() == pins["sha256"]
    assert len(cs.pool()) == pins["pool_size"]
    assert len(all_items()) == pins["items"]
    assert [len(cs.typed_cases(e)) for e in cs.WIDTHS] == [cs.TYPED_CASES] * 3 == [40] * 3


def test_the_pool_covers_every_code_shape(pins):
    pool = cs.pool()
    cand, _ = cs.candidates()
    assert len({e.label for e in pool}) == len(pool)
    pairs = sorted({(e.min_len, e.max_len) for e in pool})
    assert pairs == [tuple(p) for p in pins["min_max_pairs"]]
    assert pairs == sorted({(e.min_len, e.max_len) for e in cand})  # the draw loses no pair that the family has
    max_lens = {e.max_len for e in pool}
    assert max_lens == {e.max_len for e in cand} and max_lens >= set(cs.REQUIRED_MAX_LEN)
    assert cs.REQUIRED_MAX_LEN == (1, 2, 5, 6, 8, 9, 10, 11, 12, 13, 16, 17, 24, 32)
    assert sorted({e.variant for e in pool}) == [0, 1, 2, 3, 4, 5] == pins["decoder_classes"]
    assert {str(v): sum(1 for e in pool if e.variant == v) for v in range(6)} == pins["codes_per_class"]
    assert {e.bucket for e in pool} == {0, 1, 2, 3}
    groups = {}
    for e in cand:
        groups.setdefault(e.group, []).append(e)
    drawn = {}
    for e in pool:
        assert e.group == (e.min_len, e.max_len, rw.decoder_class(e.min_len, e.max_len)[0], cs.bucket_of(e.live.size))
        drawn[e.group] = drawn.get(e.group, 0) + 1
    assert drawn == {g: min(len(m), cs.PER_GROUP) for g, m in groups.items()}  # up to 4 of every group, no group lost
    assert sorted(groups) == [tuple(g) for g in pins["groups"]]  # the ids of tests/test_gpu_code_sweep.py
    assert [drawn[g] for g in sorted(groups)] == pins["group_sizes"]


def test_only_entries_without_a_live_byte_symbol_are_left_out(pins):
    fits = [(label, h) for label, h, kind in hf.family() if kind == "fits"]
    want = [label for label, h in fits if hf.n_live(h) == 0]
    assert cs.left_out() == want == pins["left_out"]
    assert len(cs.candidates()[0]) == len(fits) - len(want) + len(cs.EXTRA_HISTS)


def test_every_code_has_the_stated_items():
    seen_modes, seen_sizes = set(), set()
    for ci, e in enumerate(cs.pool()):
        its = cs.items(e)
        sizes = [it.n for it in its[: cs.N_EDGE + cs.N_DRAWN]]
        assert len(set(sizes[: cs.N_EDGE])) == cs.N_EDGE and set(sizes[: cs.N_EDGE]) <= set(cs.EDGE_SIZES), e.label
        assert all(1 <= n <= cs.DRAWN_MAX for n in sizes[cs.N_EDGE :]), e.label
        assert {it.mode for it in its[:7]} == set(cs.MODES), e.label
        assert len(its) == 7 + (e.max_len == 32), e.label
        live = set(e.live.tolist())
        top2 = sorted(set(e.length[e.live].tolist()))[-2:]
        for it in its:
            assert it.n >= 1 and set(np.unique(it.data).tolist()) <= live, it
            lens = e.length[it.data]
            if it.mode == "deep":
                assert lens.min() >= top2[0], it
            if it.mode == "tail":
                assert np.all(lens[-cs.TAIL_RUN :] == e.length[e.live].max()), it
            seen_modes.add(it.mode)
            seen_sizes.add(it.n)
    assert seen_modes == set(cs.MODES) | {"deepest"} and seen_sizes >= set(cs.EDGE_SIZES)


def test_every_32_bit_code_has_the_item_that_fills_the_bound():
    """only the deepest byte symbol: a body of 4 n + 4 bytes, which is ghf_compress_batch_shared_bound(n) = (4 n + 4 + 15) & ~15
    to the byte, and runs of 128 * 32 and 512 * 32 bits, the widest a u16 of a run record and of a seek table holds"""
    deep = [e for e in cs.pool() if e.max_len == 32]
    assert len(deep) >= 4
    n = cs.BOUND_EXACT_N
    assert (4 * n + 4) % 16 == 0 and n > cs.DRAWN_MAX
    for e in deep:
        it = cs.items(e)[-1]
        assert it.mode == "deepest" and it.n == n and e.length[e.deepest] == 32 and np.all(it.data == e.deepest), e.label
        assert it.body.size == 4 * n + 4 == (4 * n + 4 + 15) & ~15, e.label
        assert it.n == max(x.n for x in cs.items(e)), e.label  # it sets the batch's max_item_bytes
        rec = np.frombuffer(it.record[8 : 8 + 2 * (-(-n // 128))].tobytes(), dtype="<u2")
        assert rec.max() == 128 * 32, e.label
        tab = np.frombuffer(it.table[64:].tobytes(), dtype=rw.REC)
        assert tab["run"].max() == 512 * 32, e.label


def test_the_ranges_cover_every_residue_and_edge():
    for what, cases in (("flat", all_items()), ("typed", [t for e in cs.WIDTHS for t in cs.typed_cases(e)])):
        lo, hi, ones, aligned = set(), set(), 0, 0
        for c in cases:
            assert len(c.ranges) == 3, c
            for first, count in c.ranges:
                assert 0 <= first and 1 <= count and first + count <= c.n, c
                lo.add(first % 16)
                hi.add((first + count) % 16)
                ones += count == 1
                aligned += first % 4096 == 0 and (first + count) % 4096 == 0 and first > 0
        assert lo == set(range(16)) == hi, what
        assert ones >= len(cases) and aligned >= 3, what


def test_header_and_body_decompress_to_the_item():
    for it in all_items():
        back = orc.decompress(it.image, cap=it.n + 8)
        assert back.size == it.n and np.array_equal(back, it.data), it
        code, hs = orc.parse_header(it.image)
        got, want = code.as_dict(), it.entry.code.as_dict()  # (the header holds the decoder's tables, not the lengths)
        assert hs == it.entry.header.size, it
        assert all(got[k] == want[k] for k in ("symbol", "first_code", "start_pos", "min_len", "max_len")), it


def test_records_and_tables_add_up_to_the_body():
    for it in all_items():
        bits = int(it.entry.length[it.data].sum())
        assert it.body.size == -(-(bits + int(it.entry.length[256])) // 8), it
        rec = it.record
        magic, n = np.frombuffer(rec[:8].tobytes(), dtype="<u4")
        runs = np.frombuffer(rec[8 : 8 + 2 * (-(-it.n // cs.RUN))].tobytes(), dtype="<u2")
        assert (int(magic), int(n), int(runs.astype(np.int64).sum())) == (cs.MAGIC, it.n, bits) and rec.size % 8 == 0, it
        tab = np.frombuffer(it.table[64:].tobytes(), dtype=rw.REC)
        assert int(tab["start"][0]) == it.entry.first_bit and int(tab["run"].astype(np.int64).sum()) == bits, it


@pytest.mark.parametrize("e", cs.WIDTHS)
def test_typed_cases_split_xor_and_merge(e):
    cases = cs.typed_cases(e)
    classes = set()
    for t in cases:
        assert t.tensor.size == t.base.size == t.new.size == t.n * e, t
        x = t.new ^ t.base                                   # the XOR the delta forms compress
        out = np.empty(t.n * e, dtype=np.uint8)
        for p in range(e):
            plane = np.ascontiguousarray(x[p::e])            # the split
            assert np.array_equal(plane, t.planes[p]), (t, p)
            back = orc.decompress(t.image(p), cap=t.n + 8)
            assert np.array_equal(back, plane), (t, p)
            out[p::e] = back                                 # the merge
        assert np.array_equal(out, t.tensor) and np.array_equal(out ^ t.base, t.new), t
        assert all(a != b for a, b in zip(t.variants, t.variants[1:])), t  # neighbouring planes run different hot loops
        assert len(set(t.variants)) == min(e, 6), t
        classes |= set(t.variants)
    assert classes == set(range(6))
    assert {t.n for t in cases} >= set(cs.EDGE_SIZES)


def _forget():
    for f in (cs._pool, cs._items, cs._typed_cases):
        f.cache_clear()


@pytest.mark.parametrize("name", ["SEED_POOL", "SEED_SIZES", "SEED_ITEM", "SEED_RANGE", "SEED_TYPED", "SEED_BASE", "TAIL_RUN",
                                  "DEEP_RUN_ODDS", "DRAWN_MAX", "BOUND_EXACT_N", "PER_GROUP"])
def test_a_changed_generator_constant_changes_the_digest(monkeypatch, pins, name):
    before = getattr(cs, name)
    monkeypatch.setattr(cs, name, before + 1)
    _forget()
    try:
        assert cs.sha256() != pins["sha256"]
    finally:
        monkeypatch.undo()
        _forget()
    assert getattr(cs, name) == before
