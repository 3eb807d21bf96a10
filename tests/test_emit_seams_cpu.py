"""CPU: what tests/emit_seams.py covers, asserted from the model alone before any GPU is asked, and the model held against
the oracle.  No GPU.  The pins are tests/golden/golden_emit_seams.json."""
import json
import os

import numpy as np
import pytest

import code_sweep as cs
import emit_seams as es
import pkgload
import shard_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 9), (8, 9), (1, 12), (7, 10), (1, 16), (2, 16), (1, 32), (2, 32), (1, 1), (1, 2), (1, 40), (1, 64)]


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "golden_emit_seams.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------ the cases
def test_the_cases_have_not_drifted(pins):
    assert es.sha256() == pins["sha256"] and es.sha256_small() == pins["sha256_small"]
    assert [c.label for c in es.codes()] == pins["codes"]
    assert es.count() == es.N_TUPLES == pins["tuples"] == 32824  # no case is left out, for any reason
    per_tier = [sum(len(vs) for code in es.codes() for _, vs in es.tier_a(code)),
                sum(len(vs) for code in es.route_codes() for a in es.ALIGNS for _, vs in es.tier_b(code, a)),
                sum(len(vs) for code in es.short_codes() for _, vs in es.tier_c(code))]
    assert per_tier == [12 * 4 * 128, 2 * (4 * 15 * 3 * 2 * 33 + 15 * 3 * 2 * 16), 10 * 2 * 2] == [6144, 26640, 40]
    assert es.FILLS == ("shallow", "deep", "mixed", "ones") and es.B_FILLS == ("deep", "ones")
    for cs_, vs in es.all_tuples():
        assert len(set(vs)) == len(vs), cs_


def test_the_codes_follow_the_rule():
    codes = es.codes()
    assert [c.shape for c in codes] == SHAPES
    assert [c.packer for c in codes] == [0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 4, 4]
    pool = cs.pool()
    for p in range(4):
        mine = [e for e in pool if es.packer_of(e.max_len) == p]
        a, b = codes[2 * p], codes[2 * p + 1]
        assert a.min_len == 1 and all((e.max_len, e.live.size) <= (a.max_len, a.live.size) for e in mine if e.min_len == 1)
        assert all((e.min_len, e.max_len, e.live.size) <= (b.min_len, b.max_len, b.live.size) for e in mine)
    assert [c.shape for c in es.route_codes()] == [(1, 9), (1, 12), (1, 16), (1, 32), (1, 64)]
    assert [c.packer for c in es.route_codes()] == [0, 1, 2, 3, 4]
    for c in codes:
        assert c.length[c.shallowest] == c.length[c.live].min() and c.length[c.deepest] == c.length[c.live].max(), c
        assert c.long == (c.max_len > 32) and (c.header is None) == c.long


def test_every_size_is_cut_into_chunks_of_16384():
    ghf = pkgload.load().ghf
    sizes = {cs_.n for cs_, _ in es.all_tuples()}
    assert sizes == {es.N_A} | set(es.B_SIZES) and len(es.B_SIZES) == 15
    assert es.B_SIZES == tuple(es.C + d for d in (1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 5120, 5121, 9223)) + (2 * es.C, 3 * es.C)
    for n in sorted(sizes):
        assert ghf.chunk_symbols(n) == es.C == 16384, n


def test_the_data_is_what_the_fills_say():
    for code in es.codes():
        live = set(code.live.tolist())
        for fill in es.FILLS:
            cs_ = es.case(code, fill, es.N_A)
            assert cs_.data.size == es.N_A and cs_.nchunks == 3 and set(np.unique(cs_.data).tolist()) <= live, cs_
            for c in (1, 2):
                tail = cs_.data[c * es.C - 128 : c * es.C]
                if fill == "shallow":
                    assert np.all(tail == code.shallowest) and code.length[code.shallowest] == code.length[code.live].min(), cs_
                if fill == "deep":
                    assert np.all(tail == code.deepest) and code.length[code.deepest] == code.length[code.live].max(), cs_
                if fill == "ones":
                    assert np.all(tail == code.ones), cs_
            mixed = es.case(code, "mixed", es.N_A).data
            keep = np.ones(es.N_A, dtype=bool)
            keep[es.C - 128 : es.C] = keep[2 * es.C - 128 : 2 * es.C] = False
            assert np.array_equal(cs_.data[keep], mixed[keep]), cs_  # the fills differ in those 128 symbols alone
    for code in es.route_codes():
        for fill, sym in (("deep", code.deepest), ("ones", code.ones)):
            for n in es.B_SIZES:
                d = es.case(code, fill, n).data
                for c in range(n // es.C):
                    assert np.all(d[(c + 1) * es.C - 128 : (c + 1) * es.C] == sym), (code, fill, n)


# ---------------------------------------------------------------------------------------------- the model and the oracle
def test_the_model_is_the_oracle_at_the_header_front():
    """HEADER | LAST at the header's end: the model's bytes are header || orc_encode_body(data), for every code the
    oracle can pack, every fill, and every size of tier B"""
    todo = [es.case(code, fill, es.N_A) for code in es.short_codes() for fill in es.FILLS]
    todo += [es.case(code, fill, n) for code in es.route_codes() if not code.long for fill in es.B_FILLS for n in es.B_SIZES]
    for cs_ in todo:
        e = cs_.expect(es.Variant("header_last", 0))
        want = np.concatenate((cs_.code.header, cs.orc_body(cs_.data, cs_.code.code)))
        assert e.S is None and e.flags == es.HEADER | es.LAST and e.lead == 8 * cs_.code.header.size, cs_
        assert (e.end, e.nbytes) == (8 * want.size, want.size) and np.array_equal(e.image[: e.nbytes], want), cs_
        assert e.cap == sm.min_cap(e.lead, e.end, 0), cs_
        assert not e.image[e.nbytes :].any(), cs_


def test_the_long_codes_are_the_comb():
    """no oracle packs codes beyond 32 bits: the model's bits are the format's definition, every code MSB first"""
    for code in es.codes()[10:]:
        depth = code.max_len
        assert code.long and code.live.tolist() == list(range(depth + 1))
        strings = ["1" * i + "0" for i in range(depth)] + ["1" * depth]
        cs_ = es.case(code, "mixed", es.N_A)
        assert "".join(map(str, cs_.bits.tolist())) == "".join(strings[v] for v in cs_.data.tolist())


def test_the_front_that_keeps_what_the_buffer_held():
    """keep_front, bit by bit: in front of S the buffer's bits, from S on the model's, zeros through the end bit's unit"""
    for code in (es.codes()[0], es.codes()[7], es.codes()[11]):
        cs_ = es.case(code, "deep", es.C + 17)
        for ph in es.PHASES8:
            for front in ("keep",) if code.long else ("keep", "keep_last"):
                e = cs_.expect(es.Variant(front, ph))
                body = cs_.bits if front == "keep" else np.concatenate([cs_.bits, sm.tail_bits(code.t, (e.S + cs_.bits.size) % 8)])
                assert e.S == 384 + ph and e.end == e.S + body.size and e.nbytes == (e.end + 7) // 8 and e.held.size == e.cap
                assert e.cap == sm.min_cap(e.S, e.end, 0)
                want = np.unpackbits(e.held)
                want[e.S : 8 * e.cap] = 0
                want[e.S : e.end] = body
                assert np.array_equal(np.unpackbits(e.image), want), (cs_, front, ph)
                r = cs_.expect(es.Variant("rebase" if front == "keep" else "rebase_last", ph))
                assert r.S == (1 << 35) + ph and r.cap == e.cap - 48 and np.array_equal(r.image[16:], e.image[64:])


# -------------------------------------------------------------------------------------------------------------- coverage
def test_both_seams_take_every_carry():
    for code in es.codes():
        for cs_, vs in es.tier_a(code):
            assert [v.ph for v in vs] == list(range(128)) and all(v.car and v.align == 0 for v in vs)
            assert {v.front for v in vs} == ({"rebase"} if code.long else {"rebase_last"})
            seen = {1: set(), 2: set()}
            for v in vs:
                for c, carry in cs_.seams(v.ph):
                    assert carry == (v.ph + int(code.length[cs_.data[: c * es.C]].sum())) % 128
                    seen[c].add(carry)
            assert seen == {1: set(range(128)), 2: set(range(128))}, cs_


def test_the_shallow_fill_reaches_the_limit_of_the_reload():
    """127 carry bits of 1-bit codes are 127 of the 128 symbols loaded again: the rule's exact limit.  With a least length
    of 2 the reload reaches 64 symbols, with l it reaches ceil(127 / l)."""
    least = {c.shape: int(c.length[c.shallowest]) for c in es.codes()}
    assert least == {(1, 9): 1, (8, 9): 8, (1, 12): 1, (7, 10): 7, (1, 16): 1, (2, 16): 2, (1, 32): 1, (2, 32): 2, (1, 1): 1,
                     (1, 2): 2, (1, 40): 1, (1, 64): 1}  # (1, 2): the 1-bit code is the end mark's
    for code in es.codes():
        cs_ = es.case(code, "shallow", es.N_A)
        l = least[code.shape]
        for c in (1, 2):
            reach = [cs_.reload(c, carry)[0] for carry in range(128)]
            assert reach == [-(-carry // l) for carry in range(128)], cs_
            assert max(reach) == reach[127] == {1: 127, 2: 64, 7: 19, 8: 16}[l] <= 127, cs_
    assert sorted(p for p in {c.packer for c in es.codes() if least[c.shape] == 1}) == [0, 1, 2, 3, 4]  # every packer reaches 127


def test_the_deep_fill_cuts_the_longest_code_at_every_position():
    for code in es.codes():
        cs_ = es.case(code, "deep", es.N_A)
        L = int(code.length[code.deepest])  # (2, 16) and (2, 32): the end mark's is one bit longer
        assert L == code.length[code.live].max() and L >= code.max_len - 1
        for c in (1, 2):
            cut = [carry for carry in range(1, 128) if cs_.reload(c, carry)[1]]
            assert cut == [carry for carry in range(1, 128) if carry % L], cs_
            assert bool(cut) == (L >= 2), cs_
            # the bits of the cut code that stay inside the unit: every position 1 .. L - 1 (as far as 127 bits go)
            assert {carry % L for carry in cut} == set(range(1, min(L, 128))), cs_
        over = {carry: ph for ph in range(128) for c, carry in cs_.seams(ph) if c == 1}
        assert sorted(over) == list(range(128))  # ... and tier A reaches each of them (see above)


def test_the_ones_fill_puts_1_bits_on_either_side_of_the_cut():
    """The canonical codes give their deepest symbol a codeword of 0 bits (at most a last 1): a seam that cuts such a code at
    the wrong bit, or leaves a symbol out, still writes the right bytes.  The `ones` fill is the live symbol with the most 1
    bits: it is cut at every carry that is no multiple of its length, and wherever the code has two 1 bits there is a carry
    that leaves a 1 on either side of the unit boundary.  The one code without a 1 bit in any live codeword is (1, 1)."""
    for code in es.codes():
        word, L = code.t.codes[code.ones], int(code.length[code.ones])
        pop = bin(word).count("1")
        assert pop == max(bin(code.t.codes[s]).count("1") for s in code.live), code
        assert (pop == 0) == (code.shape == (1, 1)) and word % 2 == (pop > 0), code  # ... and its last bit is a 1
        assert pop >= 2 or code.shape in ((1, 9), (1, 1), (1, 2)), code
        cs_ = es.case(code, "ones", es.N_A)
        for c in (1, 2):
            cut = [carry for carry in range(1, 128) if cs_.reload(c, carry)[1]]
            assert cut == [carry for carry in range(1, 128) if carry % L], cs_
            inside = {carry % L for carry in cut}  # the bits of the cut code that stay inside the unit
            assert inside == set(range(1, min(L, 128))), cs_
            both = [k for k in inside if word & ((1 << k) - 1) and word >> k]
            assert bool(both) == (pop >= 2), cs_


def test_every_packer_takes_every_route_behind_a_seam(pins):
    tab = es.route_table()
    assert tab == pins["routes"]
    for p, name in enumerate(es.PACKERS):
        can = es.routes_of_packer(p)
        assert {r for r in es.ROUTES if tab[r][p]} == set(can), name
    assert es.routes_of_packer(0) == es.routes_of_packer(1) == es.routes_of_packer(2) == es.ROUTES
    assert set(es.ROUTES) - set(es.routes_of_packer(3)) == {"trips_car", "trips"}
    assert set(es.ROUTES) - set(es.routes_of_packer(4)) == {"trips_car", "trips", "end_full", "end_tile", "end_ragged", "front_header"}
    # ... and every combination of a body route with a front, for every packer that can take both
    body = ("trips_car", "trips", "odd_tile", "ragged", "unaligned")
    fronts = ("front_zeros", "front_header", "front_keep")
    for code in es.route_codes():
        pairs = set()
        for a in es.ALIGNS:
            for cs_, vs in es.tier_b(code, a):
                for v in vs:
                    r = es.routes(cs_, v, behind_seam=True)
                    pairs |= {(x, y) for x in r for y in r}
        can = es.routes_of_packer(code.packer)
        assert {(x, y) for x in body for y in fronts if x in can and y in can} <= pairs, code
        # ... and of a body route behind a seam with the end mark that follows it.  A ragged tail is followed by end_ragged
        # alone; behind a full last chunk the end mark follows trips, and a plain tile only where there are no trips
        for end in (r for r in ("end_full", "end_tile", "end_ragged") if r in can):
            for x in (r for r in body if r in can):
                possible = not (x == "ragged" and end != "end_ragged") and not (x == "odd_tile" and end == "end_full" and code.packer < 3)
                assert ((x, end) in pairs) == possible, (code, x, end)


def test_the_routes_are_read_off_size_alignment_and_side_car():
    code, wide = es.codes()[0], es.codes()[6]
    for nsym, aligned, car, want in ((16384, True, True, {"trips_car"}), (16384, True, False, {"trips"}), (16384, False, True, {"unaligned"}),
                                     (1, True, True, {"ragged"}), (1024, True, True, {"odd_tile"}), (4095, True, False, {"odd_tile", "ragged"}),
                                     (4096, True, False, {"trips"}), (5120, True, True, {"trips_car", "odd_tile"}),
                                     (9223, True, True, {"trips_car", "odd_tile", "ragged"}), (9223, False, False, {"unaligned"})):
        assert es.chunk_routes(code, nsym, aligned, car) == want, (nsym, aligned, car)
    assert es.chunk_routes(wide, 16384, True, True) == {"odd_tile"} and es.chunk_routes(wide, 4097, True, False) == {"odd_tile", "ragged"}


# ---------------------------------------------------------------------------------------------------- nothing can go missing
@pytest.mark.parametrize("name,value", [("FILLS", ("shallow", "deep", "ones")), ("B_FILLS", ("deep",)), ("B_SIZES", es.B_SIZES[1:]), ("ALIGNS", (0, 15)),
                                        ("PHASES8", es.PHASES8[:-1]), ("FRONTS", es.FRONTS[:-1]), ("C_OFFSETS", (0,)),
                                        ("C_PLANS", ("direct",))])
def test_a_removed_fill_size_or_variant_is_noticed(monkeypatch, pins, name, value):
    monkeypatch.setattr(es, name, value)
    assert es.count() < es.N_TUPLES  # (the digest cannot tell: alignment, side-car and plan change no expected byte)


def test_a_removed_code_is_noticed(monkeypatch, pins):
    full = es.codes()
    for drop in range(12):
        monkeypatch.setattr(es, "codes", lambda: full[:drop] + full[drop + 1 :])
        monkeypatch.setattr(es, "short_codes", lambda: tuple(c for c in es.codes() if not c.long)[:10])
        monkeypatch.setattr(es, "route_codes", lambda: tuple(c for c in (full[0], full[2], full[4], full[6], full[11]) if c in es.codes()))
        assert es.count() < es.N_TUPLES, drop
    assert es.sha256() != pins["sha256"]


@pytest.mark.parametrize("name", ["SEED_DATA", "SEED_HELD", "N_A", "KEEP_UNITS", "RELOAD"])
def test_a_changed_generator_constant_changes_the_digest(monkeypatch, pins, name):
    before = getattr(es, name)
    monkeypatch.setattr(es, name, before + 1)
    es.case.cache_clear()
    try:
        assert es.sha256_small() != pins["sha256_small"]
    finally:
        monkeypatch.undo()
        es.case.cache_clear()
    assert getattr(es, name) == before
