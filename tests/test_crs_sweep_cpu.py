"""CPU: what tests/crs_sweep.py covers, pinned before any kernel runs, and its expectations held against the oracle's own
.crs encoder and decoder and against what the compiled reference's NormalHuffDecoder read out of a sample of the files
(tests/golden/golden_crs_sweep.json).  No GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import crs_sweep as zs
import hist_families as hf
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "golden_crs_sweep.json")) as f:
        return json.load(f)


def all_items():
    return [it for t in zs.pool() for it in zs.items(t)]


def test_the_sweep_has_not_drifted(pins):
    pool = zs.pool()
    assert zs.PER_GROUP == 2 == pins["per_group"]
    assert zs.sha256() == pins["sha256"]
    assert len(pool) == pins["pool_size"] and len(all_items()) == pins["items"]
    assert zs.groups() == pins["groups"]
    assert [len(zs.trees_of(d)) for d in zs.groups()] == pins["group_sizes"]
    assert {k: sum(1 for t in pool if t.kind == k) for k in ("hand", "mirror", "ref")} == pins["kinds"]


def test_the_pool_covers_every_depth_and_both_orientations(pins):
    pool = zs.pool()
    assert zs.groups() == list(range(1, 65))
    ref = [t for t in pool if t.kind == "ref"]
    assert {t.max_len for t in ref} == set(range(1, 65))  # a reference-built tree at every depth, 33..64 included
    for edge in (12, 16, 32):
        for side in ([t for t in pool if t.max_len <= edge], [t for t in pool if t.max_len > edge]):
            assert any(t.deepest_zeros for t in side) and any(t.deepest_ones for t in side), edge
    # the draw: PER_GROUP of every depth up to 32 (or all there are), every deeper tree; every one of them mirrored
    cand, left = zs.candidates()
    by_depth = {}
    for t in cand:
        by_depth.setdefault(t.max_len, []).append(t)
    for d, members in by_depth.items():
        assert sum(1 for t in ref if t.max_len == d) == (min(len(members), zs.PER_GROUP) if d <= 32 else len(members)), d
    assert [t.label for t in pool if t.kind == "mirror"] == [t.label + "~mirror" for t in ref]
    # only what is deeper than 64 is left out, by name
    assert left == zs.left_out() == pins["left_out"] == ["deep/fib75", "crs/fib66"]
    hists = dict([(label, h[:256]) for label, h, _ in hf.family()] + [(label, h) for label, h, _ in hf.crs_extras()])
    for label in left:
        assert max(len(c) for c in orc.crs_code_strings(orc.crs_tree(hists[label]))) > 64
    n_usable = sum(1 for h in hists.values() if np.count_nonzero(h) >= 2) + len(zs.EXTRA_HISTS)
    assert len(cand) + len(left) == n_usable
    for _, h in zs.EXTRA_HISTS:
        assert 0 < int(h.sum()) < 1 << 55


def test_hand_built_shapes():
    hand = {t.label: t for t in zs.pool() if t.kind == "hand"}
    assert len(hand) == 2 * len(zs.COMB_DEPTHS) + 8 + len(zs.HYBRIDS) == 40
    assert zs.COMB_DEPTHS == (1, 2, 8, 9, 10, 11, 12, 13, 16, 17, 32, 33, 63, 64)
    for d in zs.COMB_DEPTHS:
        r, l = hand["hand/comb-right/d%d" % d], hand["hand/comb-left/d%d" % d]
        for t, bit in ((r, "1"), (l, "0")):
            assert t.max_len == d and t.n_leaves == d + 1 and sorted(t.length[t.live].tolist()) == list(range(1, d + 1)) + [d]
            assert t.codes[t.rightmost if bit == "1" else t.leftmost] == bit * d
            order = sorted(t.live.tolist(), key=lambda k: t.codes[k])
            assert order != sorted(order) or d < 2, t  # leaf order is not key order
    for j in range(1, 9):
        t = hand["hand/balanced/%d" % (1 << j)]
        assert t.n_leaves == 1 << j and t.min_len == t.max_len == j
    assert zs.HYBRIDS == ((7, 13), (7, 17), (7, 33), (4, 64))
    for j, d in zs.HYBRIDS:
        t = hand["hand/balanced%d+comb/d%d" % (1 << j, d)]
        lens = t.length[t.live]
        assert t.max_len == d and t.min_len == j and int((lens == j).sum()) == (1 << j) - 1 and t.n_leaves == (1 << j) + d - j


def test_headers_and_numbering_are_the_reference_decoders():
    """the model's preorder header is the oracle's serialisation of the tree it built; parsed back (the restatement of
    DecodeHuffTree), it gives the model's codes and the numbering the model states for ghf_tree"""
    L = orc.lib()
    hists = dict([(label, h[:256]) for label, h, _ in hf.family()] + [(label, h) for label, h, _ in hf.crs_extras()] +
                 [("sweep/" + label, h) for label, h in zs.EXTRA_HISTS])
    for t in zs.pool():
        if t.kind == "ref":
            assert np.array_equal(t.header, orc.crs_tree_bytes(orc.crs_tree(hists[t.label]))), t
        assert t.tree_bytes == 2 * (2 * t.n_leaves - 1)
        parsed = orc.OrcTree()
        assert L.orc_crs_parse_tree(t.header.ctypes.data, t.header.size, C.byref(parsed)) == t.header.size, t
        assert orc.crs_code_strings(parsed) == t.codes, t
        assert parsed.root == t.root == 256 and parsed.n_leaves == t.n_leaves
        n_par = t.n_leaves - 1
        assert list(parsed.left[256 : 256 + n_par]) == t.left[:n_par] and list(parsed.right[256 : 256 + n_par]) == t.right[:n_par], t
        assert t.codes[t.leftmost] == "0" * t.length[t.leftmost] and t.codes[t.rightmost] == "1" * t.length[t.rightmost]


def test_every_tree_has_the_stated_items():
    seen_sizes, seen_modes = set(), set()
    for ti, t in enumerate(zs.pool()):
        its = zs.items(t)
        live = set(t.live.tolist())
        sizes = [it.n for it in its[:7]]
        assert len(set(sizes[:5])) == 5 and set(sizes[:5]) <= set(zs.EDGE_SIZES) and all(1 <= n <= zs.DRAWN_MAX for n in sizes[5:]), t
        assert {it.mode for it in its[:7]} == set(zs.MODES), t
        top2 = sorted(set(t.length[t.live].tolist()))[-2:]
        for it in its:
            assert set(np.unique(it.data).tolist()) <= live and it.n <= 48 * 1024, it
            lens = t.length[it.data]
            assert it.total_bits == int(lens.sum()) and it.body.size == -(-it.total_bits // 8), it
            if it.left_bits:
                assert int(it.body[-1]) & ((1 << it.left_bits) - 1) == 0, it  # zero-filled
            if it.mode == "deep":
                assert lens.min() >= top2[0], it
            if it.mode == "tail":
                assert np.all(lens[-zs.TAIL_RUN :] == t.max_len), it
            if it.mode == "block":
                assert it.n == 4097 and lens.min() >= 33, it
            seen_modes.add(it.mode)
            seen_sizes.add(it.n)
        assert sum(it.mode == "block" for it in its) == (t.max_len >= 33), t
        # ends: every left_bits the lengths can reach, in items of at most 200 symbols
        ends = [it for it in its if it.mode == "ends"]
        reach = {int(-sum(c) % 8) for c in _sums_mod8(t)}
        assert sorted(reach) == zs.reachable_left_bits(t), t
        assert sorted(it.left_bits for it in ends) == sorted(reach) and all(it.n <= 200 for it in ends), t
        k = int(t.length[t.leftmost])
        if k <= 7:  # the zero padding can be a whole code of the leftmost leaf: an item where it is
            assert any(it.left_bits >= k for it in ends), t
    assert seen_modes == set(zs.MODES) | {"ends", "run0", "run1", "block"} and seen_sizes >= set(zs.EDGE_SIZES)


def _sums_mod8(t):
    """the residues mod 8 that sums of one or more of the tree's lengths take, by closure"""
    steps = {int(l) % 8 for l in t.length[t.live]}
    seen = set(steps)
    while True:
        more = {(a + b) % 8 for a in seen for b in steps} - seen
        if not more:
            return [(r,) for r in seen]
        seen |= more


def test_the_run_items_cannot_settle_by_themselves():
    runs = zs.run_items()
    assert sorted(s for s, _ in runs) == [16, 16, 32, 32, 64, 64]
    assert {it.mode for _, it in runs} == {"run0", "run1"}
    for stride, it in runs:
        t = it.tree
        assert stride == (16 if t.max_len <= 16 else 64 if t.max_len > 32 else 32)
        key = t.leftmost if it.mode == "run0" else t.rightmost
        k = int(t.length[key])
        run = int(np.flatnonzero(it.data != key)[-1]) + 1
        prefix_bits = int(it.cum[run])
        assert prefix_bits % 2 == 1 and k % 2 == 0 and 512 % k == 0, it  # no subsequence starts on a boundary of the run
        first_sub, last_sub = -(-prefix_bits // 512), it.total_bits // 512
        assert last_sub - first_sub >= 80, it
        # every shifted parse of the run is valid: from any bit of it the walk returns the run's leaf
        bits = np.unpackbits(it.body)[: it.total_bits]
        for shift in range(1, k):
            got, _, _ = zs.decode_bits(t, bits, prefix_bits + shift, prefix_bits + shift + 8 * k, limit=4)
            assert got == [key] * 4, (it, shift)


def test_materialised_histograms_pack_to_the_oracles_file():
    """header || prefix || body from the model == orc.crs_compress(data), for the family entries that exist as bytes"""
    n = 0
    for i, label, h in hf.pinned():
        if hf.n_live(h) < 2:
            continue
        data = hf.materialise(i, h)
        t = zs.Tree(label, "ref", orc.crs_code_strings(orc.crs_tree(h[:256])))
        assert np.array_equal(zs.Item(t, "materialised", "materialised", data).file, orc.crs_compress(data)), label
        n += 1
    assert n >= 300


def test_every_file_decompresses_to_its_item():
    for it in all_items():
        f = it.file
        tb = it.tree.tree_bytes
        assert f.size == tb + 2 + it.total_bits // 8 and int(f[tb]) == it.left_bits, it
        back = orc.crs_decompress(f, cap=it.n + 8)
        assert back.size == it.n and np.array_equal(back, it.data), it
        d = it.decoder_input
        assert d.size == tb + 2 + it.body.size and np.array_equal(d[tb + 2 :], it.body), it
        chunk, seg = it.index()
        assert int(chunk[0]) == it.tree.first_bit and seg.size == -(-it.n // 64), it


def test_the_pieces_add_up(pins):
    """(landing, n_symbols) of every piece of every item at every cut, held to the oracle's plain walk of the body (decode
    under the tree that its restatement of DecodeHuffTree parses from the model's header) from the landing of the piece
    before; the walks' symbols concatenate to the item"""
    assert zs.PIECE_SIZES == (64, 1000, 4096)
    total, over = 0, []
    for t in zs.pool():
        tree = orc.crs_parse_tree(t.header)
        for it in zs.items(t):
            assert it.cuts() == (list(zs.PIECE_SIZES) if it.total_bits >= 8 else []), it
            out = np.empty(it.n, dtype=np.uint8)
            for own in it.cuts():
                cuts, at = it.pieces(own), 0
                assert len(cuts) == -(-(it.total_bits // 8) // own) >= 1, (it, own)
                for k, (lo, hi, first, end_bit, landing, nsym) in enumerate(cuts):
                    assert (lo, hi) == (k * own, min((k + 1) * own, it.total_bits // 8)), (it, own, lo)
                    n, pos = orc.crs_walk(tree, it.body, it.total_bits, 8 * lo + first, 8 * lo + end_bit, out[at:])
                    assert n == nsym, (it, own, lo)
                    if k == len(cuts) - 1:
                        assert landing == 0 and pos == it.total_bits == 8 * lo + end_bit, (it, own, lo)
                    else:
                        assert end_bit == 8 * own and pos - 8 * hi == landing >= 0, (it, own, lo)
                    at += n
                    if t.max_len >= 33:
                        over.append(landing)
                assert at == it.n and np.array_equal(out, it.data), (it, own)
                total += len(cuts)
            assert it.n_pieces() == sum(len(it.pieces(own)) for own in it.cuts()), it
    # codes of more than 32 bits that begin in a piece's last bits, a 64-bit code in its very last bit included
    assert sum(1 for x in over if x >= 32) >= 1000 and max(over) == 63
    assert total == pins["pieces"]


def test_the_pieces_ids_are_pinned(pins):
    """the ids of tests/test_gpu_crs_sweep.py::test_pieces: a depth's (tree, item) pairs in ceil(pieces / PIECES_PER_ID) parts"""
    assert zs.PIECES_PER_ID == 5000
    parts = [zs.piece_parts(d) for d in zs.groups()]
    assert parts == pins["piece_parts"] and min(parts) == 1
    for d, k in zip(zs.groups(), parts):
        want = sorted(repr(it) for t in zs.trees_of(d) for it in zs.items(t))
        got = [repr(it) for j in range(k) for t, its in zs.piece_part(d, j) for it in its]
        assert sorted(got) == want and len(got) == len(want), d  # every item in exactly one part
        for j in range(k):
            assert sum(it.n_pieces() for t, its in zs.piece_part(d, j) for it in its) <= 2 * zs.PIECES_PER_ID, (d, j)


def test_the_references_own_decoder_read_the_sample(pins):
    ref = pins["ref_nd"]
    by_name = {repr(it): it for it in all_items()}
    assert set(ref) <= set(by_name)
    trees = {by_name[name].tree.label for name in ref}
    assert {by_name[name].tree.max_len for name in ref} == set(range(1, 65))
    assert trees >= {t.label for t in zs.pool() if t.kind == "hand" or (t.kind == "mirror" and t.max_len >= 33)}
    failed = {name: r for name, r in ref.items() if r.startswith("failed")}
    assert failed == {}, failed
    for name, digest in ref.items():
        assert hashlib.sha256(by_name[name].data.tobytes()).hexdigest() == digest, name


@pytest.mark.parametrize("name", ["SEED_POOL", "SEED_SIZES", "SEED_ITEM", "SEED_ENDS", "SEED_RUN", "SEED_BLOCK", "SEED_KEYS", "PER_GROUP"])
def test_a_changed_generator_constant_changes_the_digest(monkeypatch, pins, name):
    before = getattr(zs, name)
    monkeypatch.setattr(zs, name, before + 1)
    for f in (zs.pool, zs._items):
        f.cache_clear()
    try:
        assert zs.sha256() != pins["sha256"]
    finally:
        monkeypatch.undo()
        for f in (zs.pool, zs._items):
            f.cache_clear()
    assert getattr(zs, name) == before
