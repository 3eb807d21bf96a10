"""CPU: what tests/k6_pieces.py covers, asserted from the model alone before any GPU is asked, and the model of the
ghf_sync_piece contract held against the oracle, against crs_sweep's piece arithmetic and against the bit-serial stand-ins
of test_sharded_gloo.py.  No GPU, no library.  The pins are tests/golden/golden_k6_pieces.json."""
import json
import os

import numpy as np
import pytest

import code_sweep as cs
import crs_sweep as zs
import k6_pieces as kp
import shard_model as sm
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
LABELS = ["cls8/8-9", "cls4/4-5", "two/7-8", "two/1-2", "direct/1-12", "long16/1-16", "long32/1-31", "long32/1-32"]
CODES = kp.codes()
by_code = pytest.mark.parametrize("code", CODES, ids=[c.label for c in CODES])


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "golden_k6_pieces.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------ the cases
def test_the_cases_have_not_drifted(pins):
    assert kp.sha256() == pins["sha256"]
    assert [c.label for c in CODES] == pins["codes"] == LABELS
    census = kp.census()
    assert census == pins["census"] == {"A": 352, "B": 115, "C": 785, "D": 476, "E": 128}
    assert sum(census.values()) == kp.N_CASES == pins["cases"] == 1856  # no case is left out, for any reason


def test_the_codes_follow_the_rule():
    """all six shapes, and what K6 makes of each: its mode, its class and the stride of its function rows, from the lengths"""
    assert tuple(dict.fromkeys(c.shape for c in CODES)) == kp.SHAPES
    assert [(c.mode, c.cls, c.stride) for c in CODES] == [(2, 8, 16), (2, 4, 16), (2, 0, 16), (2, 0, 16), (1, 0, 16), (0, 0, 16), (0, 0, 32), (0, 0, 32)]
    pool = cs.pool()
    for c in CODES:
        assert any(e is c.entry for e in pool), c
        lens = c.length[c.length > 0]
        assert (lens.min(), lens.max()) == (c.min_len, c.max_len) and c.eof_len == c.length[256], c
        # k6_cls's conditions, from the codewords: the L-bit codes begin at 1, the end mark is an (L + 1)-bit code below them
        two = c.max_len - c.min_len <= 1 and c.max_len <= 31
        assert c.mode == (2 if two else 1 if c.max_len <= 12 else 0), c
        first_short = min(c.by_len[c.min_len])
        is_cls = two and c.max_len == c.min_len + 1 and c.min_len in (8, 4) and first_short == 1 and c.eof_len == c.max_len
        assert c.cls == (c.min_len if is_cls else 0), c
        assert c.stride == (16 if c.max_len <= 16 else 32), c
        assert sum(np.ldexp(1.0, -int(l)) for l in lens) == 1.0, c  # complete: the model is total
    a, b = CODES[0], CODES[1]
    assert kp.census_of(a.length) == {8: 255, 9: 2} and kp.census_of(b.length) == {4: 15, 5: 2}
    assert [(c.min_len, c.max_len) for c in CODES[2:4]] == [(7, 8), (1, 2)]
    assert len(kp.census_of(CODES[4].length)) >= 3 and CODES[4].max_len <= 12
    assert 13 <= CODES[5].max_len <= 16 and 17 <= CODES[6].max_len <= 31 and CODES[7].max_len == 32


# -------------------------------------------------------------------------------------------- the model against the oracle
@by_code
def test_true_chains_count_every_symbol_and_land_on_the_code_boundaries(code):
    for ch in kp.tier_a(code):
        s = ch.stream
        # the stream: the oracle's encoder under this code (what orc.compress runs behind its own code build), decoded back
        # by the oracle from header || body, and bit for bit the plain packer of shard_model
        assert np.array_equal(s.body, cs.orc_body(s.data, code.entry.code))
        assert np.array_equal(orc.decompress(s.image, cap=s.n + 16), s.data), s
        if ch.fill == "deep":
            bits = np.concatenate((sm.code_bits(s.data, code.t), sm.tail_bits(code.t, s.mark_bit % 8)))
            assert np.array_equal(np.packbits(bits), s.body), s
        chunk_bit, _ = cs.expected_index(s.data, code.length, 0)
        assert np.array_equal(chunk_bit.astype(np.int64), s.cum[:-1][::4096]), s
        assert sum(p.want.n_symbols for p in ch.pieces) == s.n, s
        k, first = 0, 0
        for i, p in enumerate(ch.pieces):
            assert p.first_bit == first and (p.lo == 0 if i == 0 else p.lo == ch.pieces[i - 1].hi), (s, i)
            assert s.cum[k] == 8 * p.lo + p.first_bit, (s, i)  # the entry bit is the true boundary
            k += p.want.n_symbols
            if i + 1 < len(ch.pieces):
                assert p.want.has_end_mark == 0 and 8 * p.hi + p.want.landing == s.cum[k], (s, i)
                assert s.cum[k - 1] < 8 * p.hi or p.want.n_symbols == 0, (s, i)
            first = p.want.landing
        last = ch.pieces[-1]
        assert last.hi == s.body.size and last.want.has_end_mark == 1 and last.want.landing is None, s  # ends with the stream
        owns = [p.hi - p.lo for p in ch.pieces]
        assert owns[: len(kp.A_OWN)] == list(kp.A_OWN) and ch.pieces[0].want == (0, 0, 0), s  # end_bit == 0 comes first
        if ch.fill == "typical":
            assert owns[len(kp.A_OWN) : -2] == list(kp.A_BIG), s
            # the end mark lies entirely in the look-ahead of the piece in front of the last one
            assert ch.pieces[-2].want.has_end_mark == 0 and ch.pieces[-2].want.n_symbols > 0 and last.want == (None, 0, 1), s
            assert 8 * last.lo <= s.mark_bit < 8 * last.lo + 8 and last.first_bit == s.mark_bit - 8 * last.lo, s
        else:
            assert last.want.n_symbols > 0, s  # symbols and the mark in one piece: counting stops at the mark
    assert {8 * o for o in kp.A_OWN + kp.A_BIG} == {0, 64, 504, 512, 520, 32760, 32768, 32776, 2096640, 2097152, 2097664}


@pytest.mark.parametrize("label", LABELS[:5])
def test_the_typical_stream_is_what_the_oracle_compresses_its_data_to(label):
    """where the code the oracle builds from the data itself is the pool entry's -- the `typical` draw of these five codes
    is long enough for that -- header || body is orc.compress(data) to the byte"""
    code = kp.by_label(label)
    s = kp.tier_a(code)[0].stream
    own = orc.build_code(orc.histogram(s.data))
    assert list(own.length) == list(code.entry.code.length) and list(own.codeword) == list(code.entry.code.codeword), s
    assert np.array_equal(orc.compress(s.data), s.image), s


def test_the_outputs_of_the_chains_begin_at_every_residue_mod_16():
    seen = set()
    for code in CODES:
        for ch in kp.tier_a(code):
            seen |= {o % 16 for o, p in zip(ch.out_offsets(), ch.pieces) if p.want.n_symbols}
    assert seen == set(range(16))


def crs_twin(code):
    """a .crs tree with the codewords of a canonical code that leaves a byte value free: the end mark takes that key"""
    strings = [""] * 256
    for s in code.live.tolist():
        strings[s] = format(int(code.t.codes[s]), "0%db" % code.length[s])
    free = next(k for k in range(256) if not strings[k])
    strings[free] = format(code.eof_cw, "0%db" % code.eof_len)
    return zs.Tree("twin/" + code.label, "hand", strings)


@pytest.mark.parametrize("code", [c for c in CODES if c.live.size < 256], ids=lambda c: c.label)
def test_the_model_agrees_with_the_piece_arithmetic_of_the_crs_sweep(code):
    """crs_sweep.Item.pieces() on a tree with the same codewords: every piece but its last (a .crs body has no end mark and
    its last piece ends with the last code)"""
    s = kp.tier_a(code)[1].stream
    it = zs.Item(crs_twin(code), "twin", "deep", s.data)
    assert it.total_bits == s.mark_bit and np.array_equal(it.body[: s.mark_bit // 8], s.body[: s.mark_bit // 8])
    seen = 0
    for own in zs.PIECE_SIZES:
        for lo, hi, first, end_bit, landing, nsym in it.pieces(own)[:-1]:
            assert s.sync(lo, hi, first) == (landing, nsym, 0), (code, own, lo)
            seen += 1
    assert seen >= 200 // max(1, code.max_len // 4)


def test_the_model_agrees_with_the_stand_ins_of_the_gloo_test():
    from test_sharded_gloo import OracleBackend

    code = kp.by_label("direct/1-12")
    cases = [(p.stream, p.lo, p.hi, p.first_bit, p.want) for p in kp.tier_a(code)[1].pieces]
    cases += [(g.stream, g.lo, g.hi, g.guess, g.want) for g in kp.tier_c(code) if g.hi - g.lo <= 2 * kp.SUB_BYTES]
    assert len(cases) >= 40
    for s, lo, hi, first, want in cases:
        piece = s.padded(32)[lo : hi + 16]
        bit, n, eof = OracleBackend._decode_from(piece, code.entry.code, first, 8 * (hi - lo))
        assert (None if eof else bit - 8 * (hi - lo), n, int(eof)) == want, (s, lo, hi, first)


# --------------------------------------------------------------------------------------------- coverage, from the model alone
@by_code
def test_every_true_entry_bit_occurs(code):
    pieces = kp.tier_b(code)
    assert [p.first_bit for p in pieces] == list(range(code.max_len)), code
    for p in pieces:
        assert p.stream.true_first(p.lo) == p.first_bit and p.hi - p.lo == kp.B_OWN and p.want.has_end_mark == 0, (code, p.lo)
        assert p.want.n_symbols > 0 and 8 * p.hi + p.want.landing in p.stream.cum, (code, p.lo)


@by_code
def test_the_wrong_guesses(code):
    cases = kp.tier_c(code)
    assert {g.kind for g in cases} == set(kp.c_kinds(code)) and (("run" in kp.c_kinds(code)) == (code.label in LABELS[:3]))
    assert {(g.hi - g.lo) // kp.SUB_BYTES for g in cases} == set(kp.C_SUBS) == {1, 2, 64, 65, 96}
    for kind in kp.c_kinds(code):
        for subs in kp.C_SUBS:
            mine = [g for g in cases if g.kind == kind and g.hi - g.lo == subs * kp.SUB_BYTES]
            guesses = [g.guess for g in mine]
            first = mine[0].true_first
            assert first == mine[0].stream.true_first(mine[0].lo) and first not in guesses and len(set(guesses)) == len(guesses)
            want = {code.stride - 1, code.stride, code.stride + 1, 255, 511} | set(range(code.max_len))
            assert set(guesses) <= want - {first} and len(guesses) == min(len(want - {first}), kp.C_MAX_GUESSES) <= 24, (code, kind)
            assert {code.stride - 1, code.stride, code.stride + 1, 255, 511} - {first} <= set(guesses), (code, kind)
            assert len([g for g in guesses if g < code.max_len]) >= min(code.max_len - 1, 19), (code, kind)
    # landing is compared for at least 8 wrong guesses of every code
    assert sum(1 for g in cases if g.want.has_end_mark == 0) >= 8, code
    for g in cases:
        assert (g.want.landing is None) == (g.want.has_end_mark == 1)
        assert g.true_want.has_end_mark == 0 and g.true_want == g.stream.sync(g.lo, g.hi, g.true_first)
    # drawn bytes: some wrong parse falls into step (it lands where the true one does) and some meets a fake end mark or
    # stays out of step to the end -- both outcomes are asserted on the GPU
    drawn = [g for g in cases if g.kind == "drawn"]
    assert any(g.want.landing == g.true_want.landing and g.want.n_symbols != g.true_want.n_symbols for g in drawn), code


@pytest.mark.parametrize("code", [c for c in CODES if "run" in kp.c_kinds(c)], ids=lambda c: c.label)
def test_on_run_bytes_a_wrong_parse_stays_wrong_in_every_subsequence(code):
    cases = [g for g in kp.tier_c(code) if g.kind == "run"]
    assert len(cases) == 5 * len(kp.guesses_for(code, cases[0].true_first))
    assert any(g.guess >= code.stride for g in cases) and any(0 < g.guess < code.stride for g in cases)
    for g in cases:
        assert g.want.has_end_mark == 0 and g.want.landing != g.true_want.landing, (code, g.guess)
        true, wrong = [], []
        g.stream.sync(g.lo, g.hi, g.true_first, trace=true)
        g.stream.sync(g.lo, g.hi, g.guess, trace=wrong)
        assert not set(true) & set(wrong), (code, g.guess)
        subs = (g.hi - g.lo) // kp.SUB_BYTES
        for starts in (true, wrong):  # both parses have codes in every subsequence they can reach
            have = {(p - 8 * g.lo) // kp.SUB_BITS for p in starts}
            assert have == set(range(subs)), (code, g.guess)


def test_landing_is_compared_in_most_wrong_guesses():
    cases = [g for c in CODES for g in kp.tier_c(c)]
    marked = sum(1 for g in cases if g.want.has_end_mark == 1)
    assert len(cases) == 785 and marked == sum(1 for g in cases if g.want.landing is None)
    assert marked / len(cases) <= 0.40, (marked, len(cases))


@by_code
def test_the_end_mark_starts_at_every_bit_around_the_edges(code):
    cases = kp.tier_d(code)
    for edge in (kp.D_SUB_EDGE, kp.D_GROUP_EDGE):
        mine = [m for m in cases if m.edge == edge]
        assert [m.offset for m in mine] == list(range(-code.max_len, code.max_len + 1)), (code, edge)
        for m in mine:
            s = m.stream
            assert s.mark_bit == edge + m.offset and s.sync(0, s.body.size, 0) == (None, s.n, 1), s
            assert np.array_equal(orc.decompress(s.image, cap=s.n + 16), s.data), s
            s.forget()
    assert (kp.D_SUB_EDGE, kp.D_GROUP_EDGE) == (3 * 512, 64 * 512)
    # the end mark ends exactly on end_bit (no 1 bits behind it), at both edges; and the body's last byte straddles each
    # edge or ends on it, so that n_settle (whole groups, never the last subsequence) takes both of its values
    for edge in (kp.D_SUB_EDGE, kp.D_GROUP_EDGE):
        mine = [m for m in cases if m.edge == edge]
        assert any(kp.ends_on_end_bit(m) for m in mine), (code, edge)
        assert {8 * m.stream.body.size <= edge for m in mine} == {True, False}, (code, edge)
        assert any(8 * m.stream.body.size == edge for m in mine), (code, edge)


@by_code
def test_the_images_have_exactly_the_subsequences_of_the_scans_levels(code):
    images = kp.tier_e(code)
    hdr = int(code.entry.header.size)
    assert hdr == 1040 + 8 * code.max_len
    assert [im.nsub for im in images if not im.stale] == [1, 2, 63, 64, 65, 4095, 4096, 4097]
    for im in images:
        raw = kp.image_bytes(im)
        assert -(-(8 * raw.size - 8 * hdr) // 512) == im.nsub, (code, im.nsub)
        assert raw.size == hdr + im.stream.body.size + im.stale and im.stale in (0, 4096)
        if im.stale:
            assert (raw[-im.stale :] == 0xFF).all() and im.nsub - 64 in kp.E_NSUB
        else:
            assert np.array_equal(orc.decompress(raw, cap=im.stream.n + 16), im.stream.data), (code, im.nsub)


# ------------------------------------------------------------------------------------------------------------- mutants
def test_a_wrong_model_changes_the_digest():
    some = (kp.by_label("cls8/8-9"), kp.by_label("direct/1-12"))
    good = kp.sha256(of_codes=some)
    assert kp.MUTANTS == ("counts_a_code_at_end_bit", "drops_the_last_code", "ignores_first_bit")
    digests = {m: kp.sha256(m, of_codes=some) for m in kp.MUTANTS}
    assert len(set(digests.values()) | {good}) == 4, digests
    # and each of them is wrong where it says: a piece whose last code ends on end_bit, any piece, a piece entered off bit 0
    s = kp.tier_a(some[1])[1].stream
    p = next(p for ch in kp.tier_a(some[1]) for p in ch.pieces if p.first_bit and p.want.n_symbols and not p.want.has_end_mark)
    assert p.stream.sync(p.lo, p.hi, p.first_bit, "drops_the_last_code").n_symbols == p.want.n_symbols - 1
    assert p.stream.sync(p.lo, p.hi, p.first_bit, "ignores_first_bit") != p.want
    hi = next(h for h in range(1, s.body.size) if 8 * h in s.cum[:-1])
    assert s.sync(0, hi, 0, "counts_a_code_at_end_bit").n_symbols == s.sync(0, hi, 0).n_symbols + 1
