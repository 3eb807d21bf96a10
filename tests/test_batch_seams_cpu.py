"""CPU: what tests/batch_seams.py covers, asserted from the model alone before any GPU is asked; the model's two
restatements of the kernels' round loops held against the oracle; and the mutants of those restatements, each of which must
change an expected byte -- the proof that the sweep would notice a wrong seam.  No GPU.  The pins are
tests/golden/golden_batch_seams.json (tests/golden/make_golden_batch_seams.py)."""
import json
import os
import re
import time

import numpy as np
import pytest

import batch_seams as bs
import shard_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "golden-huffman_amd", "csrc")
SHAPES = [(1, 9), (8, 9), (1, 12), (7, 10), (1, 16), (2, 16), (1, 32), (2, 32), (1, 1), (1, 2)]
ONE_LENGTH = [(1, 1), (1, 2)]  # every live byte symbol has the same length (under (1, 2) both have 2 bits: the end mark has 1)


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "golden_batch_seams.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------ the geometry
def constexprs():
    """every `constexpr <integer type> name = expression;` of ghf_internal.h and ghf_batch_core.h, evaluated"""
    env = {}
    for name in ("ghf_internal.h", "ghf_batch_core.h"):
        with open(os.path.join(CSRC, name)) as f:
            for m in re.finditer(r"^constexpr (?:int|uint32_t) (\w+) = ([^;]+);", f.read(), re.M):
                expr = re.sub(r"\b(\d+)u\b", r"\1", m.group(2))
                try:
                    env[m.group(1)] = int(eval(expr, {"__builtins__": {}}, dict(env)))  # noqa: S307 (names and integers only)
                except Exception:  # an expression over something that is no integer constant
                    pass
    return env


def test_the_geometry_is_the_kernels():
    k = constexprs()
    assert k["kBatchThreads"] == bs.LANES == 256
    assert k["kBatchRoundSymbols"] == bs.ROUND == 4096 and k["kBatchStageWords"] == bs.STAGE_WORDS
    assert k["kBatchDecRoundSegs"] * k["kSegSymbols"] == k["kBatchDecRoundBytes"] == bs.SIDE_ROUND == 16384
    assert k["kImgSubBits"] == bs.SUB_BITS == 512 and k["kImgRoundBits"] == bs.EDGE_BITS == 131072
    assert k["kImgStageBytes"] == bs.SLICE == 16 * 1024
    assert k["kBatchRunSymbols"] == bs.RUN == 128 and k["kBatchSeekRoundRuns"] == 256
    assert k["kBatchSeekRoundBytes"] == bs.RUN_ROUND == 128 * 256
    assert k["kSegSymbols"] == bs.SEG and k["kBlockSymbols"] == bs.BLOCK
    with open(os.path.join(CSRC, "ghf_batch_core.h")) as f:
        text = f.read()
    # the rules the model restates, as the header writes them
    assert "const uint32_t carry = B & 127u;" in text and "carry = R.over[po][kBatchThreads - 1];" in text
    assert "first_moved == kImgNone || first_moved > first_stop || first_stop < round_passes" in text
    assert "store(out, total + lo, stage, rbytes, tid);" in text and "const uint32_t start = carry + before + incl - bits;" in text


# --------------------------------------------------------------------------------------------------------------- the cases
def test_the_cases_have_not_drifted(pins):
    t0 = time.time()
    census = bs.census()
    digest = bs.sha256()
    took = time.time() - t0
    for name, (items, symbols, nbytes) in census.items():
        print("%-14s %6d items %10d symbols %10d expected bytes" % (name, items, symbols, nbytes))
    print("model built in %.1f s" % took)
    assert took < 60
    assert [bs.label(c) for c in bs.codes()] == pins["codes"] and [c.shape for c in bs.codes()] == SHAPES
    assert {k: list(v) for k, v in census.items()} == pins["census"]
    assert digest == pins["sha256"]


def test_what_cannot_exist_is_what_the_golden_file_names(pins):
    """The list may hold nothing but what a code whose live symbols all have one length cannot have: a packer carry other
    than the one in front of round 0 (4096 l bits a round), and a straddle of the edge at a bit where none of its codes
    begins.  That is code (1, 1) -- and code (1, 2), whose two byte symbols both have 2 bits (the 1-bit code is the end
    mark's): its rounds are 8192 bits, its codes begin at even bits, its end mark never straddles."""
    names = bs.unreachable()
    assert names == pins["unreachable"]
    one_length = [bs.label(c) for c in bs.codes() if c.shape in ONE_LENGTH]
    for c in bs.codes():
        assert (bs.steer_pair(c) is None) == (c.shape in ONE_LENGTH) == (np.unique(c.length[c.live]).size == 1), c
    assert all(any(n.startswith(l + ": ") for l in one_length) for n in names)
    assert len(names) == 2 * 127 + 5
    assert [n for n in names if "carry" not in n] == ["ties/c1/k2/drawn (1, 2): " + x for x in (
        "deep/over 1", "ones/over 1", "mark ends on the edge/over 0", "mark behind the straddler/over 1", "cap/over 1")]


def test_the_fills_are_what_they_say():
    for code in bs.codes():
        for it in bs.p_items(code):
            fill = it.tag.split("/")[0]
            assert it.n == bs.N_P == 2 * 4096 + 37 and set(np.unique(it.data).tolist()) <= set(code.live.tolist()), it
            if fill != "mixed":
                for s in (bs.ROUND, 2 * bs.ROUND):
                    assert np.all(it.data[s - 64 : s + 64] == bs.fill_symbol(code, fill)), it
        assert code.length[code.shallowest] == code.length[code.live].min() and code.length[code.deepest] == code.length[code.live].max()
        word = code.t.codes[code.ones]
        assert bin(word).count("1") == max(bin(code.t.codes[s]).count("1") for s in code.live)
        assert (word == 0) == (code.shape == (1, 1))


# ----------------------------------------------------------------------------------------------------------- tier P: coverage
def test_every_flat_packer_seam_sees_every_carry():
    for code in bs.codes():
        for fill in bs.FILLS:
            seen = [set(), set()]
            for it in (x for x in bs.p_items(code) if x.tag.startswith(fill + "/")):
                c = int(it.tag.split()[-1])
                assert it.carries() == ([c, 127 - c] if bs.steer_pair(code) else [0, 0]), it
                seen[0].add(it.carries()[0])
                seen[1].add(it.carries()[1])
            assert seen == ([set(range(128))] * 2 if code.shape not in ONE_LENGTH else [{0}, {0}]), (code, fill)
    assert sum(len(bs.p_items(c)) for c in bs.codes()) == 8 * 4 * 128 + 2 * 4


@pytest.mark.parametrize("e", bs.WIDTHS)
def test_every_plane_packer_seam_sees_every_carry(e):
    """plane p of launch k is under code (k + p) % 10 at carry (c + 17 p) % 128: every plane of a tensor at its own carry,
    every (code, seam) at all 128 -- in the forms launches too, where one plane of each launch is raw"""
    cc = bs.codes()
    for forms in (False, True):
        seen = {(j, s): set() for j in range(10) for s in (0, 1)}
        for k in range(10):
            ts = bs.p_planes(k, e)
            assert len(ts) == 4 * 128 + 16 and all(t.e == e and t.n == t.planes[0].n for t in ts)
            assert bin(bs.raw_of(k, e)).count("1") == 1 and bs.raw_of(k, e) < 1 << e
            for t in ts[: 4 * 128]:
                for p, pl in enumerate(t.planes):
                    assert pl.code is cc[(k + p) % 10]
                    if not (forms and bs.raw_of(k, e) >> p & 1):
                        for s, c in enumerate(pl.carries()):
                            seen[((k + p) % 10, s)].add(c)
            t = ts[17]
            if all(bs.steer_pair(pl.code) for pl in t.planes):
                assert len({pl.carries()[0] for pl in t.planes}) == e  # each plane at a carry of its own
            assert [t.planes[0].body.size % 16 for t in ts[4 * 128 :]] == list(range(16))
        for (j, s), got in seen.items():
            assert got == (set(range(128)) if cc[j].shape not in ONE_LENGTH else {0}), (e, forms, cc[j], s)


def test_the_last_unit_takes_every_size():
    for code in bs.codes():
        its = bs.tails(code)
        assert [it.body.size % 16 for it in its] == list(range(16)) and all(bs.ROUND < it.n < 2 * bs.ROUND for it in its), code
    # ... and the items at the carries end at many: the mutant that stores the last unit whole is caught there too
    assert len({it.body.size % 16 for it in bs.p_items(bs.codes()[0])}) == 16


def test_the_items_with_codes_of_their_own(pins):
    """ghf_compress_batch: the code is the item's own, so a shape is what orc.build_code makes of 8229 symbols -- at most
    13 bits -- and a carry is reached by exchanges that leave the multiset alone.  Seam 1 is at every carry wherever the
    multiset has 127 symbols of two lengths an odd number apart; seam 2 is the last round's 37 symbols' to give.  Both
    parities of max_len occur: the header leaves carry 64 and carry 0 in front of round 0."""
    own = bs.own_items()
    seen, shapes = {}, {}
    for it in own:
        key = it.base.label
        shapes[key] = (int(it.code.min_len), int(it.code.max_len), it.lead % 128)
        a, b = it.carries()
        seen.setdefault(key, [set(), set()])
        seen[key][0].add(a)
        seen[key][1].add(b)
        assert it.lead == 8 * (1040 + 8 * it.code.max_len) and it.lead % 128 == (64 if it.code.max_len % 2 else 0)
    table = {k: [shapes[k][0], shapes[k][1], shapes[k][2], len(v[0]), len(v[1])] for k, v in seen.items()}
    print(table)
    assert table == pins["own_codes"]
    assert {s[2] for s in shapes.values()} == {0, 64}
    full = [k for k, v in table.items() if v[3] == 128]
    assert len(full) == 8 and sum(v[4] == 128 for v in table.values()) >= 6
    assert table["ties/c1/k1/first"] == [1, 1, 64, 1, 1]  # 4096 bits a round: the header's 64 and nothing else
    for it in own[:: len(own) // 40]:  # the model's restatement with the header in front is the oracle's image
        t = sm.tables(it.code)
        end = np.array([(t.codes[256] >> (t.lens[256] - 1 - i)) & 1 for i in range(t.lens[256])], dtype=np.uint8)
        room = (it.image.size + 15 & ~15) + 16
        got = bs.pack_model(it.data, it.length, sm.code_bits(it.data, t), end, room, header=it.header)
        assert np.array_equal(got[: it.image.size], it.image) and np.all(got[it.image.size :] == bs.GUARD), it


# ------------------------------------------------------------------------------------------ tier P: the model notices a wrong seam
def test_the_packer_restated_is_the_oracle_and_every_mutant_is_caught(pins):
    """pack_model -- the stage, carry, keep and the last unit as ghf_batch_core.h has them -- gives orc_encode_body's bytes
    on every item of tier P; each mutant of it changes a byte at 64 or more of the 128 carries of the `ones` fill, for
    every code that has carries (the one live codeword of (1, 1) is a 0 bit: nothing it loses shows)"""
    for code in bs.codes():
        for it in bs.p_items(code) + list(bs.tails(code)):
            assert np.array_equal(bs.packed(it), bs.slot_of(it)), it
    table = bs.pack_mutant_table()
    for code in bs.codes():
        if bs.steer_pair(code):
            assert all(v >= 64 for v in table[bs.label(code)]), (code, table[bs.label(code)])
    for name, row in table.items():
        print("%-44s %s" % (name, dict(zip(bs.PACK_MUTANTS, row))))
    assert table == pins["pack_mutants"]
    assert table["ties/c1/k2/drawn (1, 2)"] == [0, 1, 0, 1]  # its one carry is 0: no keep to lose, nothing mod 64 changes


# ------------------------------------------------------------------------------------------------------------------ tier R
def test_every_code_straddles_the_edge_by_every_over():
    for code in bs.codes():
        items, missing = bs.r_items(code)
        by = {}
        for it in items:
            by.setdefault(it.family, []).append(it)
        one = code.shape in ONE_LENGTH
        L, Lo, el = int(code.length[code.deepest]), int(code.length[code.ones]), int(code.length[256])
        assert L == code.max_len
        assert [it.over for it in by["deep"]] == (list(range(L)) if code.shape != (1, 2) else [0]), code
        assert [it.over for it in by["ones"]] == (list(range(Lo)) if code.shape != (1, 2) else [0]), code
        for it in by["deep"] + by["ones"]:
            x = it.n - bs.SUFFIX - 1  # the straddling code
            assert it.cum[x + 1] == bs.EDGE_BITS + it.over and it.round_totals.tolist() == [x + 1, bs.SUFFIX], it
            assert it.verdict == (bs.OK, it.n, it.n, 2)
        (it,) = by["mark begins on the edge"]
        assert it.cum[it.n] == bs.EDGE_BITS and it.round_totals.tolist() == [it.n, 0] and it.verdict[3] == 2  # a round without a symbol
        if code.shape != (1, 2):
            (it,) = by["mark ends on the edge"]
            assert it.cum[it.n] + el == bs.EDGE_BITS and it.verdict[3] == 1
        assert [it.over for it in by.get("mark straddles", [])] == list(range(1, el))
        for it in by.get("mark straddles", []):
            assert it.cum[it.n] + el == bs.EDGE_BITS + it.over and it.verdict == (bs.OK, it.n, it.n, 1)
        assert [it.over for it in by.get("mark behind the straddler", [])] == ([] if one else list(range(1, L)))
        for it in by.get("mark behind the straddler", []):
            assert it.cum[it.n] == bs.EDGE_BITS + it.over and it.round_totals.tolist() == [it.n, 0]
        assert [it.over for it in by.get("cut inside the mark", [])] == list(range(1, el))
        for it in by.get("cut inside the mark", []):
            assert it.verdict == (bs.E_CORRUPT, 0, 0, 1) and it.sizes_verdict == it.verdict and 8 * it.stream_bytes == bs.EDGE_BITS
        if code.shape != (1, 2):
            (it,) = by["cap"]
            assert it.cap == it.n - 1 and it.verdict == (bs.E_CAP, 0, it.n - bs.SUFFIX, 2) and it.sizes_verdict == (bs.OK, it.n, 0, 2)
        if code.ci in bs.PHASE_CODES:
            assert [by["phase %d" % m][0].round_totals[0] % 16 for m in range(16)] == list(range(16)), code
    shapes = {bs.codes()[k].shape for k in bs.PHASE_CODES}
    assert shapes == {(1, 9), (2, 32)}


def test_the_plane_launches_of_tier_r():
    for k in range(10):
        whole = [it for it in bs.r_items(bs.codes()[k])[0] if it.cut is None and it.cap is None]
        for e in bs.WIDTHS:
            ts = bs.r_planes(k, e)
            assert [t.planes[0] for t in ts] == [it for it in whole if it.n * e <= 1 << 20] and all(t.e == e for t in ts)
            assert len(ts) >= 2, (k, e)
            if k not in (0, 8, 9):
                assert len(ts) == len(whole)  # (the items of many slices are more than 1 MiB as elements)


def test_the_slices():
    """a round of 1-bit codes leaves in eight slices; behind (1, 9)'s round 0 of 131 067 symbols round 1 starts at output
    phase 11, and a lane's symbols lie on both sides of a slice edge; rounds of exactly one slice, and of one symbol more"""
    cc = bs.codes()
    by = {(it.code.shape, it.family): it for c in cc for it in bs.r_items(c)[0] if it.family == "slices" or it.family.startswith("round of")}
    assert sorted(by) == [((1, 1), "slices"), ((1, 2), "slices"), ((1, 9), "slices"), ((7, 10), "round of 16384"), ((7, 10), "round of 16385")]
    assert by[((1, 1), "slices")].round_totals.tolist() == [131072, 131072, 5]
    assert by[((1, 2), "slices")].round_totals.tolist() == [65536, 65536, 5]  # (two bits a symbol: four slices)
    thick = by[((1, 9), "slices")]
    assert thick.round_totals.tolist() == [131067, 131069, 5] and -(-131067 // bs.SLICE) == 8
    assert thick.round_totals[0] % 16 == 11 and thick.round_totals[:2].sum() % 16 == 8 and thick.straddles_a_slice()
    assert not by[((1, 1), "slices")].straddles_a_slice()  # 512 symbols a lane: the lanes end on the slice edges
    assert by[((7, 10), "round of 16384")].round_totals.tolist() == [16384, 100]
    assert by[((7, 10), "round of 16385")].round_totals.tolist() == [16385, 100]


def test_the_decoder_restated_is_the_model_and_both_mutants_are_caught(pins):
    """decode_model gives every item of tier R its verdict, its rounds and its bytes; with the carry forced to 0 every
    item of the `ones` family with over > 0 changes (and so does the `deep` one, by its size), with the slices stored at
    `total` every item whose round has more than one slice does"""
    for code in bs.codes():
        for it in bs.r_items(code)[0]:
            want = bs.want_decoded(it)
            got = bs.decoded(it)
            assert got[:3] == want[:3] and np.array_equal(got[3], want[3]), it
            sized = bs.decode_model(it.body[: it.stream_bytes], code, scan=bs.scan_of(it))
            assert sized[:3] == it.sizes_verdict[:2] + (it.sizes_verdict[3],), it
    table = bs.decode_mutant_table()
    for name, row in table.items():
        for m, (hit, of) in row.items():
            assert hit == of, (name, m, hit, of)
    for name, row in table.items():
        print("%-44s %s" % (name, row))
    assert table == pins["decode_mutants"]
    assert sum(v["carry_zero"][1] for v in table.values()) == sum(int(c.length[c.ones]) - 1 for c in bs.codes() if c.shape != (1, 2))
    assert all(v["slice_at_total"][1] >= 1 for k, v in table.items() if k.split("(")[1] in ("1, 9)", "1, 1)", "1, 2)", "7, 10)"))


# ------------------------------------------------------------------------------------------------------------ tiers S and U
def test_the_side_car_and_run_record_rounds():
    cc = bs.codes()
    assert [cc[k].shape for k in bs.S_CODES] == [(1, 1), (2, 32)] == [cc[k].shape for k in bs.U_CODES]
    assert bs.S_SIZES == (16384, 16385, 16447, 16448, 16449, 32768, 32769, 32831, 32832, 32833)
    assert bs.U_SIZES == (32768, 32769, 32895, 32896, 32897, 65536, 65537, 65663, 65664, 65665)
    for k in bs.S_CODES:
        its = bs.s_items(cc[k])
        assert [it.n for it in its] == list(bs.S_SIZES) * 2
        for it in its:
            sym = bs.fill_symbol(cc[k], it.tag.split("/")[0])
            for s in range(bs.SIDE_ROUND, it.n + 1, bs.SIDE_ROUND):
                assert np.all(it.data[s - 64 : min(s + 64, it.n)] == sym), it
    for k in bs.U_CODES:
        its = bs.u_items(cc[k])
        assert [it.n for it in its][:20] == list(bs.U_SIZES) * 2
        for it in its:
            bits = it.record[8:].view("<u2")[: -(-it.n // bs.RUN)]
            if cc[k].shape == (1, 1):
                assert np.all(bits[: it.n // bs.RUN] == 128), it  # every whole run is 128 bits
            if it.tag == "deepest/U":
                assert it.n == 2 * 32768 + 1 and bits.max() == 4096 and np.all(bits[:-1] == 4096), it  # the u16 format's most: 128 x 32
        assert (len(its) == 21) == (cc[k].shape == (2, 32))
        d = bs.u_damaged(cc[k])
        rec = bs.damaged_record(d)
        assert d.n == 32768 + 129 and rec.size == d.record.size and np.flatnonzero(rec != d.record).tolist()[0] // 2 == 4 + 256
        assert rec[8:].view("<u2")[256] == 1 != d.record[8:].view("<u2")[256]
    for e in bs.WIDTHS:
        for k in (0, 1):
            assert [t.n for t in bs.s_planes(k, e)] == list(bs.S_SIZES) * 2 and [t.n for t in bs.u_planes(k, e)] == list(bs.U_SIZES) * 2
            assert [pl.code.shape for pl in bs.s_planes(k, e)[0].planes] == [[(1, 1), (2, 32)][(k + p) % 2] for p in range(e)]
