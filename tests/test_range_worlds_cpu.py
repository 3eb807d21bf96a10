"""CPU (-m "not gpu"): the preconditions of tests/test_gpu_range_variants.py, checked with the oracle before anything runs
on a GPU.  Every world must land in the decoder class it was chosen for, its hot-eligible ranges must really be
hot-eligible, and the blocks that are meant to take the miss path or the unstaged path must be where the ranges look."""
import numpy as np
import pytest

import range_worlds as rw
from oracle import oracle as orc


@pytest.mark.parametrize("name", rw.WORLDS)
def test_world_lands_in_its_class(name):
    w = rw.world(name)
    min_len, max_len, largest, variant, pair_bits = rw.EXPECTED[name]
    assert (w.min_len, w.max_len) == (min_len, max_len)
    assert int(w.block_bits.max()) == largest
    assert int(np.round(largest / 8)) == rw.LARGEST_BLOCK_BYTES[name]
    assert rw.decoder_class(w.min_len, w.max_len) == (variant, pair_bits) == (w.variant, w.pair_bits)
    lens = np.asarray(w.length)
    assert lens[256] >= 1 and lens[lens > 0].min() == min_len and lens.max() == max_len
    assert w.stream_bytes == w.first_bit // 8 + (int(w.block_bits.sum()) + w.length[256] + 7) // 8


def test_the_classes_are_all_there():
    assert sorted({rw.EXPECTED[name][3] for name in rw.WORLDS}) == [0, 1, 2, 3, 4, 5]
    assert {rw.EXPECTED[name][4] for name in rw.WORLDS} == {0, 4, 10}
    # the thresholds of the choice itself
    assert [rw.decoder_class(1, m)[0] for m in (5, 6, 8, 9, 10, 11, 12, 13, 16, 17, 32)] == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


@pytest.mark.parametrize("name", rw.WORLDS)
def test_pairs(name):
    w = rw.world(name)
    pairs = w.pairs()
    assert len(w.random_pairs()) == 40 and max(c for _, c in w.random_pairs()) <= 20000
    assert len(set(w.random_pairs())) == 40
    for p in w.fixed_pairs() + w.hot_pairs() + w.extra_pairs():
        assert p in pairs
    # the last, partial block alone, from its start and from three bytes in
    assert w.n % rw.BLOCK != 0
    assert (4096 * (w.nb - 1), w.n - 4096 * (w.nb - 1)) in pairs and (4096 * (w.nb - 1) + 3, w.n - 4096 * (w.nb - 1) - 3) in pairs
    assert (4096 * 3 + 5, 4096 * 4) in pairs


def test_fixed_pairs_are_those_of_test_gpu_seek():
    import test_gpu_seek

    for name in rw.WORLDS:
        w = rw.world(name)
        fixed = w.fixed_pairs()
        assert len(fixed) == 23 and test_gpu_seek.range_pairs(w.n)[: len(fixed)] == fixed


@pytest.mark.parametrize("name", rw.WORLDS)
def test_hot_pairs_are_hot_eligible(name):
    w = rw.world(name)
    assert len(w.hot_pairs()) == 5
    for first, count in w.hot_pairs():
        gI, groups = rw.k7_view(first, count)
        assert (gI * 4096 - first) % 16 == 0, (first, count)  # the view's output pointer is as aligned as d_out
        assert groups - 1 >= 2, (first, count)                # whole blocks in front of the view's last group
        assert (gI + groups - 1) * 4096 < first + count <= (gI + groups) * 4096
    assert rw.k7_view(4096 * 2 + 16 * 9, 4096 * 5 + 1000)[0] == 3  # ... behind a head
    gI, groups = rw.k7_view(4096 * 3 + 5, 4096 * 4)                 # the cold twin: never aligned
    assert groups >= 2 and (gI * 4096 - (4096 * 3 + 5)) % 16 != 0


@pytest.mark.parametrize("name", rw.WORLDS)
def test_blocks_fit_the_staged_span_or_not(name):
    """4576 = 4608 less the 16 bytes of alignment slack in front of a span, the 12 bytes of look-ahead behind it and the
    partial bytes at either end"""
    w = rw.world(name)
    if name != "nonstat":
        assert int(w.block_bytes.max()) <= 4576
        return
    big = [int(b) for b in np.nonzero(w.block_bits // 8 > rw.STAGED_MAX)[0]]
    assert len(big) == 5
    a, k = rw.NONSTAT_RUN
    assert big == list(range(a // 4096 + 1, (a + k) // 4096 + 1))
    # every one of them is decoded by K7 (not only by the head) in a range made for it, one of them as a head too
    by_k7, by_head = set(), set()
    for first, count in w.unstaged_pairs():
        assert (first, count) in w.pairs()
        gI, groups = rw.k7_view(first, count)
        by_k7.update(range(gI, gI + groups))
        if first % 4096:
            by_head.add(first // 4096)
    assert set(big) <= by_k7 and by_head & set(big)
    firsts = [f for f, c in w.unstaged_pairs() if a <= f < a + k]
    assert any(f % 16 for f in firsts)                                            # begins inside the stretch, unaligned
    assert any(f < a and a < f + c < a + k for f, c in w.unstaged_pairs())        # ends inside it
    assert (4096 * 8, 4096 * 9) in w.unstaged_pairs()


def _hot_blocks(w, pairs):
    """blocks that a hot pass of K7 decodes in one of these ranges (16-byte aligned output)"""
    out = set()
    for first, count in pairs:
        gI, groups = rw.k7_view(first, count)
        if (gI * 4096 - first) % 16 == 0:
            out.update(g for g in range(gI, gI + groups - 1) if w.block_bytes[g] <= 4576)
    return out


def test_the_miss_path_is_reached():
    w14, w22, wns = rw.world("len14"), rw.world("len22"), rw.world("nonstat")
    full14, full22 = w14.n // 4096, w22.n // 4096
    assert (full14, full22) == (48, 18)
    a12 = w14.block_count_above(12)
    assert int((a12[:full14] > 0).sum()) == 40
    b12, b16 = w22.block_count_above(12), w22.block_count_above(16)
    assert int((b12[:full22] > 0).sum()) == 18 and int((b16[:full22] > 0).sum()) == 14
    hot14, hot22 = _hot_blocks(w14, w14.hot_pairs()), _hot_blocks(w22, w22.hot_pairs())
    assert any(a12[g] > 0 for g in hot14)      # variant 4's miss path inside a hot pass
    assert any(b16[g] > 0 for g in hot22)      # variant 5, a code beyond 16 bits inside a hot pass
    assert any(a12[g] > 1 for g in hot14) and any(b12[g] > 1 for g in hot22)  # more than one miss in a block
    # the head (k_decode_head) meets codes beyond the 12-bit table too
    for w in (w14, w22):
        heads = [(f, min(f + c, (f // 4096 + 1) * 4096)) for f, c in w.pairs() if f % 4096]
        assert any(int((w.sym_len[lo:hi] > 12).sum()) > 0 for lo, hi in heads)
    # nonstat: the unstaged path meets them as well (13-bit codes in the stretch the code does not fit)
    assert wns.max_len == 13 and all(wns.block_count_above(12)[g] > 1 for g in (10, 11, 12, 13))
    # no other world has a code beyond the table
    for name in ("pair5", "pair2", "len8", "len9", "len12"):
        assert rw.world(name).max_len <= rw.LUT_BITS_MAX


@pytest.mark.parametrize("kind", sorted(rw.TAIL_KINDS))
def test_tail_sizes_give_every_remainder(kind):
    sizes = rw.tail_sizes(kind)
    assert sorted(sizes) == list(range(16)), "widen TAIL_WINDOW: all 16 remainders are required"
    data = rw.tail_data(kind)
    for r, n in sizes.items():
        assert rw.TAIL_N0 <= n < rw.TAIL_N0 + rw.TAIL_WINDOW
        assert int(orc.compress(data[:n]).size) % 16 == r
        assert n - 5000 > 0 and n > 2 * 4096  # the tail ranges: two whole blocks and a short third


def test_expected_table_on_a_hand_made_input():
    """expected_table moved here from test_gpu_seek.py: two blocks of a two-symbol code, by hand"""
    data = np.zeros(4096 + 600, dtype=np.uint8)
    data[5] = 1
    data[4096 + 513] = 1
    length = [1, 2] + [0] * 254 + [2]
    t = rw.expected_table(data, length, 100, flags=1)
    assert t.size == 64 + 2 * 24 and bytes(t[:8]) == b"GHFSEEK1"
    rec = t[64:].view(rw.REC)
    assert list(rec["start"]) == [100, 100 + 4097]
    assert list(rec["run"][0]) == [513] + [512] * 7
    assert list(rec["run"][1]) == [512, 89, 0, 0, 0, 0, 0, 0]
