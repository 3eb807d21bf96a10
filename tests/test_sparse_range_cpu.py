"""CPU (-m "not gpu"): the element range of zero-suppressed byte planes.  The numpy model of the rank
table and of the plan (tests/sparse_range_model.py) gives x[first : first + count] on every edge of the grid; the host-only
ghf_sparse_rank_bytes and ghf_sparse_rank_parse agree with the model and the parse refuses every single-field damage; the
eight entry points are exported, bound and declared directly in front of the sparse section of the header; a null context is
refused without a device; and a resource guard keeps the four new kernels free of spills and scratch and at the LDS that
DESIGN.md states.  In the style of tests/test_sparse_cpu.py."""
import os
import re

import numpy as np
import pytest

import pkgload
import sparse_range_model as model
import test_sparse_cpu as tsc

ROOT = tsc.ROOT
E_INVAL, E_FORMAT = 1, 6
R = model.RANK_ELEMS
N = 3 * R + 4099
FIRSTS = (0, 1, 7, 8, 15, 4095, 4096, 32767, 32768, 32769, N - 1)
COUNTS = (1, 9, 4097, 32768, None)  # None: n - first

ARGC = {"ghf_sparse_rank_pack": 5, "ghf_sparse_rank_parse": 3, "ghf_sparse_merge_at": 7, "ghf_compress_planes_sparse_ranked": 14,
        "ghf_compress_planes_sparse_ranked_delta": 15, "ghf_decode_planes_sparse_range": 17, "ghf_decode_planes_sparse_range_delta": 18}
METHODS = ("sparse_rank_bytes", "sparse_rank_parse", "sparse_rank_pack", "sparse_merge_at", "compress_planes_sparse_ranked",
           "compress_planes_sparse_ranked_delta", "decode_planes_sparse_range", "decode_planes_sparse_range_delta")
# unit -> kernel -> its static LDS in bytes, as DESIGN.md section 21 states it
KERNELS = {"ghf_sparse": {"_ZN3ghf22k_sparse_merge_move_atEPKhS1_mmPhPKmPKi": 4128, "_ZN3ghf19k_sparse_rank_writeEPKhmPKmPmPKi": 0},
           "ghf_seek": {"_ZN3ghf21k_seek_expand_streamsENS_23SeekExpandStreamsParamsE": 71488},
           "ghf_decode": {"_ZN3ghf27k_build_decode_tables_slotsEPK8ghf_codePNS_9DecTablesEjPi": 13112}}
SHORT = {"k_sparse_merge_move_at": 4128, "k_sparse_rank_write": 0, "k_seek_expand_streams": 71488, "k_build_decode_tables_slots": 13112}


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


# ---------------------------------------------------------------- 1. the model
def strings():
    """random strings at 1 %, 25 % and 100 % non-zero, an all-zero string, and one whose middle rank block is all zero"""
    rng = np.random.default_rng(21)
    out = {}
    for name, density in (("1%", 0.01), ("25%", 0.25), ("100%", 1.0)):
        x = rng.integers(1, 256, N, dtype=np.uint8)
        x[rng.random(N) >= density] = 0
        out[name] = x
    out["zeros"] = np.zeros(N, dtype=np.uint8)
    hole = out["25%"].copy()
    hole[R : 2 * R] = 0
    out["hole"] = hole
    assert np.count_nonzero(out["100%"]) == N and 0 < np.count_nonzero(out["1%"]) < N // 50
    return out


STRINGS = strings()


def ranges():
    for first in FIRSTS:
        for count in COUNTS:
            count = N - first if count is None else count
            if first + count <= N:
                yield first, count


@pytest.mark.parametrize("name", list(STRINGS))
def test_the_model_of_the_plan_gives_the_slice(name):
    x = STRINGS[name]
    mask, vals = model.sparse_form(x)
    table = model.table_of(x)
    assert table.size == model.rank_bytes(N) == 64 + 8 * 5
    seen = 0
    for first, count in ranges():
        p = model.sparse_range(mask, vals, table, N, first, count)
        assert np.array_equal(p["out"], x[first : first + count]), (first, count)
        assert p["from"] % R == 0 and p["from"] <= first < p["from"] + R and p["lead"] == first - p["from"]
        assert p["m_lo"] % 4096 == 0 and (p["v_lo"] - p["vals_skip"]) % 4096 == 0  # both decodes begin on a seek block
        seen += 1
    assert seen >= 40
    if name == "hole":  # a range inside the empty block reads two equal entries and decodes no value
        p = model.sparse_range(mask, vals, table, N, R + 5, 100)
        assert p["v_lo"] == p["v_hi"] > 0 and not p["out"].any()
    if name == "zeros":
        assert not model.cum_in(table).any()


def test_the_numpy_helper_of_the_binding_is_the_model_s_table(ghf):
    for x in list(STRINGS.values()) + [STRINGS["25%"][:1], STRINGS["25%"][:R], STRINGS["25%"][: R + 1]]:
        assert np.array_equal(ghf.sparse_rank_table(x), model.table_of(x))
    assert ghf.SPARSE_RANK_ELEMS == R


# ---------------------------------------------------------------- 2. the host-only calls
def test_sparse_rank_bytes(ghf):
    want = {1: 64 + 16, 32767: 64 + 16, 32768: 64 + 16, 32769: 64 + 24, (1 << 32) + 1: 64 + 8 * ((1 << 17) + 2)}
    for n, b in want.items():
        assert ghf.sparse_rank_bytes(n) == b == model.rank_bytes(n), n
    assert ghf.Context.sparse_rank_bytes(32769) == 88
    assert re.search(r"^#define GHF_SPARSE_RANK_ELEMS 32768u$", tsc.header(), flags=re.M)


def parse_rc(ghf, table):
    a = np.ascontiguousarray(table, dtype=np.uint8)
    info = ghf.SparseRankInfo()
    return ghf.lib().ghf_sparse_rank_parse(a.ctypes.data, a.size, ghf.C.byref(info)), info


def test_rank_parse_accepts_the_model_s_tables(ghf):
    for name, x in STRINGS.items():
        for n in (N, 1, 7, R - 1, R, R + 1):
            rc, info = parse_rc(ghf, model.table_of(x[:n]))
            assert rc == 0, (name, n)
            assert (info.n, info.n_vals, info.n_blocks, info.version) == (n, np.count_nonzero(x[:n]), model.rank_blocks(n), 1)
    info = ghf.sparse_rank_parse(model.table_of(STRINGS["hole"]))
    assert info.n == N and info.n_blocks == 4


def with_u64(table, at, value):
    t = table.copy()
    t[at : at + 8] = np.frombuffer(int(value).to_bytes(8, "little"), dtype=np.uint8)
    return t


def test_rank_parse_refuses_every_single_field_damage(ghf):
    x = STRINGS["25%"]
    good = model.table_of(x)
    cum = [int(v) for v in model.cum_in(good)]
    assert len(cum) == 5 and cum[4] - 4100 >= cum[2]
    full = model.table_of(STRINGS["100%"])
    c0 = model.HEADER_BYTES
    bad = {
        "magic": with_u64(good, 0, int.from_bytes(b"GHFSEEK1", "little")),
        "version": with_u64(good, 8, 2 | R << 32),
        "block size": with_u64(good, 8, 1 | 4096 << 32),
        "n (another size follows)": with_u64(good, 16, N + R),
        "n (the last block shrinks below its step)": with_u64(good, 16, 3 * R + 1),
        "n_vals": with_u64(good, 24, cum[4] + 1),
        "n_blocks": with_u64(good, 32, 5),
        "a reserved byte": with_u64(good, 40, 1),
        "truncated": good[:-8],
        "a word behind it": np.concatenate([good, np.zeros(8, np.uint8)]),
        "a byte behind it": np.concatenate([good, np.zeros(1, np.uint8)]),
        "the header alone": good[:64],
        "cum[0]": with_u64(good, c0, 1),
        "a cum that decreases": with_u64(good, c0 + 16, cum[1] - 1),
        "cum[nb] is not n_vals": with_u64(good, c0 + 32, cum[4] - 1),
        "a step above 32768": with_u64(full, c0 + 8, R + 1),
        "a step above the last block's elements": with_u64(good, c0 + 24, cum[4] - 4100),
    }
    assert parse_rc(ghf, good)[0] == 0 and parse_rc(ghf, full)[0] == 0
    for what, t in bad.items():
        rc, info = parse_rc(ghf, t)
        assert rc == E_FORMAT, what
        assert (info.n, info.n_vals, info.n_blocks, info.version) == (0, 0, 0, 0), what
    with pytest.raises(ghf.GhfError) as e:
        ghf.sparse_rank_parse(bad["magic"])
    assert e.value.status == E_FORMAT
    L = ghf.lib()
    assert L.ghf_sparse_rank_parse(None, 80, ghf.C.byref(ghf.SparseRankInfo())) == E_INVAL
    assert L.ghf_sparse_rank_parse(good.ctypes.data, good.size, None) == E_INVAL


# ---------------------------------------------------------------- 3. header and binding
def test_library_exports_the_entry_points(ghf):
    L = ghf.lib()
    hdr = tsc.header()
    for name, argc in ARGC.items():
        assert name in ghf.EXPORTS, name
        assert len(getattr(L, name).argtypes) == argc, name
        assert len(tsc.declaration(hdr, name).split(",")) == argc, name
    assert "ghf_sparse_rank_bytes" in ghf.EXPORTS and len(L.ghf_sparse_rank_bytes.argtypes) == 1
    assert len(tsc.declaration(hdr, "ghf_sparse_rank_bytes", ret="size_t").split(",")) == 1
    for plain in ("ghf_compress_planes_sparse_ranked", "ghf_decode_planes_sparse_range"):
        # the _delta form is the plain form with d_base added
        assert ARGC[plain + "_delta"] == ARGC[plain] + 1
        assert "const uint8_t* d_base" in tsc.declaration(hdr, plain + "_delta") and "d_base" not in tsc.declaration(hdr, plain)
    for old, new in (("ghf_compress_planes_sparse", "ghf_compress_planes_sparse_ranked"),
                     ("ghf_compress_planes_sparse_delta", "ghf_compress_planes_sparse_ranked_delta")):
        # the ranked form is the existing call with (d_ranks, rank_slot_bytes) behind its arguments
        a, b = tsc.declaration(hdr, old).split(","), tsc.declaration(hdr, new).split(",")
        assert [s.split()[-1] for s in b[: len(a)]] == [s.split()[-1] for s in a]
        assert [s.split()[-1] for s in b[len(a) :]] == ["d_ranks", "rank_slot_bytes"]
    assert ghf.C.sizeof(ghf.SparseRankInfo) == 32
    for m in METHODS:
        assert hasattr(ghf.Context, m), m


def test_the_section_stands_directly_in_front_of_the_sparse_section(ghf):
    hdr = tsc.header()
    sec = hdr.index("/* ---- an element range of zero-suppressed byte planes (DESIGN.md section 21)")
    nxt = hdr.index("/* ---- zero-suppressed byte planes")
    assert hdr.index("int ghf_crs_sync_piece(") < sec < nxt
    assert hdr[hdr.index(");", hdr.index("int ghf_crs_sync_piece(")) + 2 : sec].strip() == ""  # directly behind that declaration
    block = hdr[sec:nxt]
    for name in list(ARGC) + ["ghf_sparse_rank_bytes"]:
        ret = "size_t" if name == "ghf_sparse_rank_bytes" else "int"
        assert len(re.findall(r"^%s %s\(" % (ret, name), hdr, flags=re.M)) == 1, name
        at = block.index("%s %s(" % (ret, name))  # declared in this section
        comment = block[:at].rstrip()
        assert comment.endswith("*/"), name
        comment = comment[comment.rindex("/*") :]
        assert comment.startswith("/* No reference counterpart"), name
        assert re.search(r"include/compressor\.h:\d+-\d+", comment), name
    assert block.count("No reference counterpart") == len(ARGC) + 1
    for old in tsc.ARGC:  # no comment outside the sparse section writes an existing sparse name as a call
        assert old + "(" not in hdr[:nxt], old
    assert "GHFRANK1" in block and "NOT TRUSTED" in block and "never synchronise" in block
    assert "d_base == d_out is allowed" in block and "At most 32767 elements" in block


def test_a_null_context_is_refused_without_a_device(ghf):
    L, C = ghf.lib(), ghf.C
    idx = (ghf.Index * 16)()
    infos = (ghf.SeekInfo * 16)()
    vp16, sz16 = (C.c_void_p * 16)(*[4096] * 16), (C.c_size_t * 16)(*[64] * 16)
    r_infos, r_ptrs = (ghf.SparseRankInfo * 8)(), (C.c_void_p * 8)(*[4096] * 8)
    n_vals = (C.c_size_t * 8)(*[3] * 8)
    chosen = C.c_uint(0)
    slot, rslot = ghf.planes_slot_bytes(64), 80
    d_in, d_base, d_out, d_codes, d_bytes, d_ranks = 4096, 8192, 1 << 20, 1 << 21, 1 << 22, 1 << 23
    for e in (2, 4, 8, 0, 3):
        for mask in (0, 1, 3, 1 << 8, ghf.SPARSE_AUTO):
            for ix in (None, idx):
                assert L.ghf_compress_planes_sparse_ranked(None, d_in, 64, e, mask, d_out, slot, d_bytes, d_codes, ix, C.byref(chosen),
                                                           n_vals, d_ranks, rslot) == E_INVAL, (e, mask)
                assert L.ghf_compress_planes_sparse_ranked_delta(None, d_in, d_base, 64, e, mask, d_out, slot, d_bytes, d_codes, ix,
                                                                 C.byref(chosen), n_vals, d_ranks, rslot) == E_INVAL, (e, mask)
                tables = (None, None, None) if ix else (infos, vp16, sz16)
                assert L.ghf_decode_planes_sparse_range(None, vp16, sz16, d_codes, ix, *tables, r_infos, r_ptrs, mask, 64, e, 3, 9, d_out,
                                                        9 * 8) == E_INVAL, (e, mask)
                assert L.ghf_decode_planes_sparse_range_delta(None, vp16, sz16, d_codes, ix, *tables, r_infos, r_ptrs, d_base, mask, 64, e, 3,
                                                              9, d_out, 9 * 8) == E_INVAL, (e, mask)
    for n in (0, 1, 64, 32769):
        assert L.ghf_sparse_rank_pack(None, d_in, n, d_out, 1 << 10) == E_INVAL, n
        assert L.ghf_sparse_merge_at(None, d_in, d_base, 5, 3, n, d_out) == E_INVAL, n
    assert L.ghf_sparse_rank_pack(None, None, 0, None, 0) == E_INVAL
    assert L.ghf_sparse_merge_at(None, None, None, 0, 0, 0, None) == E_INVAL
    assert L.ghf_compress_planes_sparse_ranked(None, None, 0, 2, 0, None, 0, None, None, None, None, None, None, 0) == E_INVAL
    assert L.ghf_compress_planes_sparse_ranked_delta(None, None, None, 0, 2, 0, None, 0, None, None, None, None, None, None, 0) == E_INVAL
    assert L.ghf_decode_planes_sparse_range(None, None, None, None, None, None, None, None, None, None, 0, 0, 2, 0, 0, None, 0) == E_INVAL
    assert L.ghf_decode_planes_sparse_range_delta(None, None, None, None, None, None, None, None, None, None, None, 0, 0, 2, 0, 0, None,
                                                  0) == E_INVAL


def test_the_exported_geometry_is_the_source_s(ghf):
    src = open(os.path.join(ROOT, "golden-huffman_amd", "csrc", "ghf_internal.h")).read()
    assert re.search(r"constexpr uint32_t kSparseRankElems = (\d+);", src).group(1) == str(ghf.SPARSE_RANK_ELEMS)
    assert ghf.SPARSE_RANK_ELEMS == 8 * ghf.SPARSE_TILE == 8 * model.SEEK_BLOCK  # 4096 mask bytes: one seek block of the mask's stream
    assert re.search(r"constexpr uint32_t kSeekStreamsMax = 2 \* GHF_PLANES_MAX;", src)


# ---------------------------------------------------------------- 4. the resource guard
def test_design_states_the_lds_of_every_new_kernel():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 21.") :]
    for name, lds in SHORT.items():
        row = re.search(r"^\| `%s` \|[^\n]*$" % name, sec, flags=re.M)
        assert row, name
        assert re.search(r"\| %d \|" % lds, row.group(0)), (name, row.group(0))


@pytest.mark.parametrize("unit,sym", [(u, s) for u in KERNELS for s in KERNELS[u]])
def test_new_kernels_have_no_spills_no_scratch_and_the_stated_lds(ghf, unit, sym):
    """from the kernel metadata alone, as tests/test_sparse_cpu.py does it for section 20; the expansion kernel takes its
    sixteen streams as arguments and must stay under the 4 KiB a launch can carry"""
    text = tsc._kernel_asm(unit)
    res = tsc._resources(text, sym)
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (sym, res)
    assert res["private_segment_fixed_size"] == 0, (sym, res)
    assert res["group_segment_fixed_size"] == KERNELS[unit][sym], (sym, res)
    assert res["vgpr_count"] <= 128, (sym, res)
    meta = re.search(r"\.name:\s+%s\b" % re.escape(sym), text)
    head = text[: meta.start()]
    assert int(re.search(r"\.kernarg_segment_size:\s+(\d+)", head[head.rindex("- .agpr_count") :]).group(1)) <= 4096, sym


def test_the_existing_move_kernel_keeps_its_resources(ghf):
    """ghf_sparse_merge_at is a sibling kernel on the shared body; the listing comparison of DESIGN.md section 21 in one line:
    the kernel of section 20 keeps the registers and the LDS of its table"""
    old = tsc._resources(tsc._kernel_asm("ghf_sparse"), "_ZN3ghf19k_sparse_merge_moveEPKhS1_mPhPKmPKi")
    new = tsc._resources(tsc._kernel_asm("ghf_sparse"), "_ZN3ghf22k_sparse_merge_move_atEPKhS1_mmPhPKmPKi")
    assert old["group_segment_fixed_size"] == new["group_segment_fixed_size"] == 4128
    assert old["vgpr_count"] <= 128 and new["vgpr_count"] <= 128
    for r in (old, new):
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
