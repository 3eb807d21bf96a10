"""CPU: what tests/forms_sweep.py covers, pinned before any kernel runs (tests/golden/golden_forms_sweep.json), and its
expectations held against the numpy models of the calls: sparse_range_model for the forms and range calls, gather_model and
gather_forms_model for the two gather calls.  No GPU."""
import json
import os

import numpy as np
import pytest

import code_sweep as cs
import forms_sweep as fs
import gather_forms_model as fm
import gather_model as gm
import range_worlds as rw
import sparse_range_model as srm

HERE = os.path.dirname(os.path.abspath(__file__))
OK, E_CORRUPT = fm.OK, fm.E_CORRUPT
LEFT_OUT = ["ties/c1/k1/first", "wide/s33/ties/c1/k1/first"]  # one live symbol, and it is 0: no byte a values stream could hold


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(HERE, "golden", "golden_forms_sweep.json")) as f:
        return json.load(f)


def all_cases():
    return [c for e in fs.WIDTHS for c in fs.cases(e)]


def sparse_planes(c):
    return [(i, p) for i, p in enumerate(c.planes) if p.kind == "sparse"]


def test_the_sweep_has_not_drifted(pins):
    assert fs.FORMS_CASES == 36 == pins["cases_per_width"] and fs.WIDTHS == (2, 4, 8)
    assert [len(fs.cases(e)) for e in fs.WIDTHS] == [36] * 3 and [len(fs.typed_rows(e)) for e in fs.WIDTHS] == [cs.TYPED_CASES] * 3
    assert fs.sha256() == pins["sha256"]
    assert fs.coverage() == pins["coverage"]


def test_every_code_shape_meets_every_role(pins):
    cov = fs.coverage()
    for role in fs.ROLES:
        assert len(cov["max_len"][role]) == 32 and min(cov["max_len"][role]) >= 1, role  # every max_len 1..32, the widths together
        for e in fs.WIDTHS:
            assert min(cov["classes"][role][str(e)]) >= 1, (role, e)                     # every decoder class at every width
    for e in fs.WIDTHS:
        leads = [c.lead for c in fs.cases(e)]
        assert [leads.count(v) for v in range(6)] == [6] * 6, e                          # six tensors per id of the GPU module
        assert cov["forms"][str(e)].get("z", 0) >= 1, e
    assert cov["ragged"] >= 18 and cov["largest_n"] == 8 * fs.MASK_BYTES_MAX == 66056


def test_only_codes_without_a_non_zero_live_symbol_are_kept_from_the_values(pins):
    assert fs.values_left_out() == LEFT_OUT == pins["values_left_out"]
    assert [en.label for en in fs.zero_only()] == LEFT_OUT
    pool = cs.pool()
    may = [en for r in fs._by_len()["values"].values() for en in r]
    assert len(may) == len(pool) - 2 and all(sum(len(v) for v in fs._by_len()[r].values()) == len(pool) for r in ("mask", "dense"))
    for c in all_cases():
        for _, p in sparse_planes(c):
            if p.values is not None:
                assert p.values.entry.label not in LEFT_OUT and not np.any(p.vals == 0), c


def test_tensors_have_the_stated_forms_and_sizes():
    sizes = set()
    for c in all_cases():
        kinds = [p.kind for p in c.planes]
        assert "sparse" in kinds and "dense" in kinds and len(kinds) == c.e, c
        assert ("raw" in kinds) == (c.k % 3 == 2 and c.e > 2), c  # bf16 has no room for a third form
        if c.e == 8:
            assert sum(1 for p in c.planes if p.form == "s") >= 2, c
        mb = (c.n + 7) // 8
        sizes.add(mb)
        assert 1 <= mb <= fs.MASK_BYTES_MAX and (c.n % 8 == 0 if c.k % 2 == 0 else True), c
        if c.k < len(fs.MASK_BYTES):
            assert mb == fs.MASK_BYTES[c.k], c
        if c.k % 2:
            widest = max(int(p.mask[-1]).bit_length() for _, p in sparse_planes(c))
            assert c.n == 8 * (mb - 1) + max(1, widest), c
        assert c.tensor.size == c.base.size == c.n * c.e and np.array_equal(c.new ^ c.base, c.tensor), c
        for i, p in enumerate(c.planes):
            assert np.array_equal(c.tensor[i :: c.e], p.data), (c, i)
            if p.kind == "dense":
                assert set(np.unique(p.data).tolist()) <= set(p.main.entry.live.tolist()), (c, i)
            if p.kind == "sparse":
                assert p.mask.size == mb and set(np.unique(p.mask).tolist()) <= set(p.main.entry.live.tolist()), (c, i)
                assert (p.values is None) == (p.n_vals == 0) == (p.form == "z"), (c, i)
                if p.values is not None:
                    assert set(np.unique(p.vals).tolist()) <= set(p.values.entry.live.tolist()) - {0}, (c, i)
    assert sizes >= set(fs.MASK_BYTES)


def test_sparse_form_gives_back_the_drawn_mask_and_values():
    for c in all_cases():
        for i, p in sparse_planes(c):
            mask, vals = srm.sparse_form(p.data)
            assert np.array_equal(mask, p.mask) and np.array_equal(vals, p.vals), (c, i)
            assert not np.unpackbits(p.mask, bitorder="little")[c.n :].any(), (c, i)  # the pad bits are clear by construction
            assert int(srm.cum_in(p.rank)[-1]) == p.n_vals and p.rank.size == srm.rank_bytes(c.n), (c, i)


def test_every_range_is_the_numpy_slice_under_the_range_model():
    crossing = 0
    for c in all_cases():
        assert len(c.ranges) == 4 and c.ranges[1][1] == 1 and c.ranges[2] == (0, c.n), c
        first, count = c.ranges[3]
        if c.n > fs.RANK:
            assert first < fs.RANK <= first + count - 1 and first + count <= min(c.n, 2 * fs.RANK), c
            crossing += 1
        else:
            assert (first, count) == (0, c.n), c
        for first, count in c.ranges:
            for i, p in sparse_planes(c):
                got = srm.sparse_range(p.mask, p.vals, p.rank, c.n, first, count)["out"]
                assert np.array_equal(got, p.data[first : first + count]), (c, i, first, count)
    assert crossing >= 9


def test_every_row_is_served_and_is_the_numpy_slice():
    edges = 0
    for c in all_cases():
        re_, firsts, e = c.row_elems, c.firsts, c.e
        assert 1 <= re_ <= min(c.n, fs.ROW_ELEMS_MAX) and firsts[:-1] == sorted(set(firsts), reverse=True) and firsts[-1] == firsts[0], c
        assert {0, c.n - re_} <= set(firsts) and 2 <= len(firsts) <= 6, c  # (a tensor of one row has two: the row and its repeat)
        edges += any(f < fs.RANK < f + re_ for f in firsts)
        planes = c.model_planes()
        status = [fm.row_verdict(f, 1, re_, c.n, planes) for f in firsts]
        assert status == [OK] * len(firsts), (c, status)
        for base, src in ((None, c.tensor), (c.base, c.new)):
            out = np.zeros(len(firsts) * re_ * e, dtype=np.uint8)
            fm.expected_rows(planes, c.n, base, firsts, 1, re_, status, out, re_ * e)
            want = np.concatenate([src[f * e : (f + re_) * e] for f in firsts])
            assert np.array_equal(out, want), (c, base is not None)
    assert edges >= 9  # rows that straddle the edge of rank blocks 0 and 1


def typed_model(t, raw):
    out = []
    for p in range(t.e):
        if raw >> p & 1:
            out.append(None)
            continue
        en, image, table = t.entries[p], t.image(p), t.table(p)
        out.append({"table": table, "true_table": table, "stream": image, "stream_bytes": int(image.size), "length": [int(v) for v in en.code.length],
                    "codeword": [int(v) for v in en.code.codeword], "code_ok": True})
    return out


@pytest.mark.parametrize("e", fs.WIDTHS)
def test_the_rows_of_the_typed_tensors_are_served(e):
    raws = 0
    for k, (t, raw, re_, firsts) in enumerate(fs.typed_rows(e)):
        assert raw == (1 << (k % e) if k % 3 == 2 else 0) and 1 <= re_ <= min(t.n, fs.TYPED_ROW_ELEMS_MAX), t
        assert {0, t.n - re_} <= set(firsts) and firsts[-1] == firsts[0] and firsts[:-1] == sorted(set(firsts), reverse=True), t
        planes = typed_model(t, raw)
        assert [gm.row_verdict(f, 1, re_, t.n, planes) for f in firsts] == [OK] * len(firsts), t
        raws += raw != 0
    assert raws == cs.TYPED_CASES // 3


def test_no_run_of_512_symbols_exceeds_a_u16():
    deepest = 0
    for c in all_cases():
        for s in c.streams():
            bits = np.add.reduceat(s.entry.length[s.data], range(0, s.n, 512))
            assert bits.max() <= 0xFFFF, (c, s.entry.label)
            tab = np.frombuffer(s.table[64:].tobytes(), dtype=rw.REC)
            assert int(tab["start"][0]) == s.entry.first_bit and int(tab["run"].astype(np.int64).sum()) == int(bits.sum()), (c, s.entry.label)
            assert s.image.size == s.entry.header.size + -(-(int(bits.sum()) + int(s.entry.length[256])) // 8), (c, s.entry.label)
            deepest = max(deepest, int(bits.max()))
    assert deepest > 512 * 20  # runs far beyond what data-derived codes reach


def test_a_flipped_run_length_of_a_32_bit_values_stream_turns_the_row_corrupt():
    """the expected-value path is sensitive at that depth: on the CPU model only"""
    hits = 0
    for c in all_cases():
        for i, p in sparse_planes(c):
            if p.values is None or p.values.entry.max_len != 32 or hits:
                continue
            planes = c.model_planes()
            for f in c.firsts:
                st, v0, nv = fm.sparse_verdict(planes[i][1], c.n, f, c.row_elems)
                assert st == OK
                if not nv:
                    continue
                g, k = divmod(v0 // gm.RUN, gm.RUNS_PER_BLOCK)
                vs = p.values
                # the model's own walker lands on the recorded end of that run, so it is the walk that the flip contradicts
                cnt = min(gm.RUN, vs.n - (v0 // gm.RUN) * gm.RUN)
                true_bits = int(gm.records(vs.table)[g]["run"][k])
                dec = gm.Decoder(vs.model()["length"], vs.model()["codeword"])
                assert dec.run_bits(vs.image, int(vs.image.size), gm.run_start(vs.table, g, k), cnt) == true_bits, (c, i)
                rec = np.frombuffer(vs.table[gm.HEADER :].tobytes(), dtype=gm.REC).copy()
                rec["run"][g][k] = true_bits ^ 1
                bad = vs.table.copy()
                bad[gm.HEADER :] = np.frombuffer(rec.tobytes(), dtype=np.uint8)
                damaged = list(planes)
                damaged[i] = p.model(vals_stream=vs.model(table=bad))
                assert fm.row_verdict(f, 1, c.row_elems, c.n, planes) == OK, (c, i, f)
                assert fm.row_verdict(f, 1, c.row_elems, c.n, damaged) == E_CORRUPT, (c, i, f)
                hits += 1
                break
    assert hits == 1
