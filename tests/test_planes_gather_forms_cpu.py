"""CPU (-m "not gpu"): ghf_decode_planes_gather_forms is exported, bound and declared, a null context is refused without a
device, the numpy model of the call (tests/gather_forms_model.py) agrees with tests/sparse_range_model.py and with plain slices
of the tensor on every row the GPU test asks for, the stored bytes of the test tensors are the oracle's, and an ISA guard keeps
the three instantiations of k_decode_planes_gather_forms free of spills, scratch and a private segment and, with the largest
stage a launch asks for, within 64 KiB of LDS.  In the style of tests/test_planes_gather_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import gather_forms_model as fm
import gather_forms_planes as fp
import pkgload
import sparse_range_model as srm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
NAME, ARGC = "ghf_decode_planes_gather_forms", 22
LDS_BUDGET = 64 * 1024
KERNELS = ["_ZN3ghf28k_decode_planes_gather_formsILi%dEEEvNS_23PlanesGatherFormsParamsEjj" % e for e in (2, 4, 8)]
# the oracle's numbers for the tensors of tests/gather_forms_planes.py: per plane the bytes of its stored streams (a raw plane:
# the plane), and the values of its sparse planes
STORED = {
    2: ([11660, 16318], [8930, None]),
    4: ([4377, 70149, 2145, 16285], [828, None, 0, None]),
    8: ([11660, 16318, 70149, 2145, 4454, 16344, 70149, 4354], [8930, None, None, 0, 875, None, None, 811]),
}


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_forms_gather_entry_point(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    block = hdr[hdr.index("/* ---- byte planes: many rows of a tensor stored sparse or against a base") : hdr.index(" * SURVEY 8(e): one stream sharded")]
    assert NAME in ghf.EXPORTS
    assert getattr(L, NAME) is not None
    assert len(getattr(L, NAME).argtypes) == ARGC
    decl = re.search(r"^int %s\(([^;]*)\);" % NAME, block, flags=re.M | re.S)
    assert decl
    assert hdr.index("int ghf_decode_planes_gather(") < hdr.index("int %s(" % NAME)  # behind its parent
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == ARGC
    comment = block[: decl.start()].rstrip()  # the comment that ends right in front of the declaration
    assert comment.endswith("*/")
    comment = comment[comment.rindex("/*") :]
    assert "No reference counterpart" in comment and "include/compressor.h:87-92" in comment
    assert "READ:" in comment and "WRITTEN:" in comment and "CALL-LEVEL REFUSALS" in comment and "DIFFERENCES" in comment
    assert re.search(r"^#define GHF_GATHER_SPARSE_MAX_ROW_ELEMS 8192u\b", block, flags=re.M)
    assert ghf.GATHER_SPARSE_MAX_ROW_ELEMS == fm.SPARSE_MAX_ROW_ELEMS == 8192
    assert hasattr(ghf.Context, "decode_planes_gather_forms")


def test_a_null_context_is_refused_without_a_device(ghf):
    """the call-level checks come before anything touches HIP; with no device the null context answers for every width"""
    L = ghf.lib()
    infos = (ghf.SeekInfo * 16)()
    ptrs = (ghf.C.c_void_p * 16)(*[4096] * 16)
    sizes = (ghf.C.c_size_t * 16)(*[2048] * 16)
    rinfos = (ghf.SparseRankInfo * 8)()
    for e in (2, 4, 8, 0, 1, 3, 16):
        for n_rows in (4, 0):
            assert L.ghf_decode_planes_gather_forms(None, ptrs, sizes, 1 << 20, infos, ptrs, sizes, rinfos, ptrs, sizes, None, 0, 1, 2048, e,
                                                    4096, 1, 16, n_rows, 8192, 16 * 16, 16384) == E_INVAL, e
    assert L.ghf_decode_planes_gather_forms(None, None, None, None, None, None, None, None, None, None, None, 0, 0, 0, 2, None, 0, 0, 0,
                                            None, 0, None) == E_INVAL


# ---------------------------------------------------------------- the tensors
@pytest.mark.parametrize("e", (2, 4, 8))
def test_the_tensors_are_what_the_gpu_test_names_and_store_the_oracles_bytes(e):
    t = fp.tensor(e)
    assert t.n == 2 * 32768 + 4096 + 517 and srm.rank_blocks(t.n) == 3 and t.n % 32768 != 0 and t.n % 8 == 5
    assert [p.stored_bytes() for p in t.planes] == STORED[e][0]
    assert [p.n_vals if p.kind == "sparse" else None for p in t.planes] == STORED[e][1]
    kinds = {p.kind for p in t.planes}
    assert kinds >= {"dense", "sparse"} and (e == 2 or "raw" in kinds)
    assert t.raw & t.sparse == 0
    for p in t.planes:
        if p.kind != "sparse":
            continue
        assert np.array_equal(srm.merge(p.mask, p.vals, t.n), p.data)
        assert p.rank.size == srm.rank_bytes(t.n) and int(srm.cum_in(p.rank)[-1]) == p.n_vals
        if p.form == "r":  # a row inside the run has a value per element, and the run crosses a rank-block edge
            assert np.all(p.data[fp.RUN_AT : fp.RUN_AT + fp.RUN_LEN] != 0) and fp.RUN_AT < 32768 < fp.RUN_AT + fp.RUN_LEN
            assert fm.ranks_of(p.mask, t.n, fp.RUN_AT + 5, 8187)[1] == 8187
        if p.form == "z":
            assert p.n_vals == 0 and p.values is None
        if p.form == "s":
            assert 0.005 * t.n < p.n_vals < 0.02 * t.n
    assert np.array_equal(t.new ^ t.base, t.delta)


# ---------------------------------------------------------------- the model
def _all_rows(t):
    return [(f, re_) for re_, firsts in fp.row_cases(t) for f in firsts]


@pytest.mark.parametrize("e", (2, 4, 8))
def test_the_model_gives_the_slices_of_the_tensor_and_agrees_with_the_range_model(e):
    t = fp.tensor(e)
    rows = _all_rows(t)
    assert {c for _, c in rows} == set(fm.ROW_ELEMS)
    assert {0, 32767, 32768, t.n - 1} <= {f for f, _ in rows} and any(f + c == t.n for f, c in rows)
    assert any(f < 32768 < f + c for f, c in rows) and any(f < 65536 < f + c for f, c in rows)
    planes = t.model_planes()
    for first, count in rows:
        assert fm.row_verdict(first, 1, count, t.n, planes) == fm.OK
        for base in (None, t.base):
            out = np.full(count * e + 3, 0xA5, dtype=np.uint8)
            fm.expected_rows(planes, t.n, base, [first], 1, count, [fm.OK], out, count * e + 3)
            assert np.array_equal(out[: count * e], t.rows([first], 1, count, base is not None)[0]), (first, count)
            assert np.all(out[count * e :] == 0xA5)
        for p in t.planes:
            if p.kind != "sparse":
                continue
            st, v0, nv = fm.sparse_verdict(p.model()[1], t.n, first, count)
            assert st == fm.OK and v0 == fp.rank_in(p, first) and nv == int(np.count_nonzero(p.data[first : first + count]))
            got = srm.sparse_range(p.mask, p.vals, p.rank, t.n, first, count)
            assert np.array_equal(got["out"], p.data[first : first + count])
            b0, run0, runs, decoded = fm.mask_runs(t.n, first, count)
            assert b0 == got["b0"] and run0 * 512 == got["m_lo"] and got["v_lo"] <= v0 and v0 + nv <= got["v_hi"]
            assert decoded <= got["m_hi"] - got["m_lo"] and decoded >= -(-(first + count) // 8) - got["m_lo"]
            if nv:
                r0, nr = fm.value_runs(v0, nv)
                assert r0 * 512 <= v0 and v0 + nv <= (r0 + nr) * 512 and (nr - 1) * 512 < v0 % 512 + nv


def test_rows_cross_the_edges_of_the_values_stream():
    """inside the run of non-zero bytes: rows whose first value stands three in front of a 512 edge and of a 4096 edge"""
    t = fp.tensor(2)
    p = t.planes[0]
    seen = set()
    for first, count in _all_rows(t):
        st, v0, nv = fm.sparse_verdict(p.model()[1], t.n, first, count)
        for edge in (512, 4096):
            if nv > 3 and v0 % edge == edge - 3:
                seen.add(edge)
    assert seen == {512, 4096}
    assert max(fm.value_runs(*fm.sparse_verdict(p.model()[1], t.n, f, c)[1:])[1] for f, c in _all_rows(t) if c == 8192) == 17


def test_verdicts_of_the_model():
    t = fp.tensor(4)
    n, planes = t.n, t.model_planes()
    p = t.planes[0]
    assert fm.row_verdict(n - 6, 1, 7, n, planes) == fm.E_INVAL and fm.row_verdict(1 << 63, 4, 7, n, planes) == fm.E_INVAL
    cum = srm.cum_in(p.rank).copy()
    cum[1] += 1  # raised by one: seen where a decoded block ends at the entry, on either side
    bad = [p.model(cum=cum)] + planes[1:]
    assert [fm.row_verdict(f, 1, 513, n, bad) for f in (100, 32768 - 513, 32768 - 100, 65536 - 513, 65536 + 10)] == \
        [fm.OK, fm.E_CORRUPT, fm.E_CORRUPT, fm.E_CORRUPT, fm.OK]
    cum = srm.cum_in(p.rank).copy()
    cum[1], cum[2] = cum[2], cum[1]
    bad = [p.model(cum=cum)] + planes[1:]
    assert [fm.row_verdict(f, 1, 7, n, bad) for f in (40000, 100, 65536 + 10)] == [fm.E_CORRUPT, fm.OK, fm.OK]
    mask = p.mask.copy()
    mask[-1] |= 1 << 6
    padded = fp.Plane("s", p.data, mask=mask)
    bad = [padded.model()] + planes[1:]
    assert [fm.row_verdict(f, 1, 7, n, bad) for f in (n - 7, n - 8 - 7, 0)] == [fm.E_CORRUPT, fm.OK, fm.OK]


# ---------------------------------------------------------------- the listing
def _kernel_asm(name):
    """gfx950 ISA text of golden-huffman_amd/csrc/<name>.hip, built with the Makefile's own flags"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "golden-huffman_amd", "csrc", name + ".hip")
    mk = open(os.path.join(ROOT, "golden-huffman_amd", "Makefile")).read()
    assert re.search(r"^NAMES := .*\b%s\b" % name, mk, flags=re.M), "the unit is built into libghf.so"
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, flags=re.M).group(1)
    flags = flags.replace("$(ARCH)", "gfx950").replace("$(ROOT)", ROOT).replace("$(HERE)", os.path.join(ROOT, "golden-huffman_amd") + "/")
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        r = subprocess.run([hipcc] + flags.split() + ["--cuda-device-only", "-S", "-o", os.path.join(td, "k.s"), src],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(os.path.join(td, "k.s")).read()


def test_forms_gather_kernels_use_no_scratch_no_spills_and_keep_the_lds_budget(ghf):
    text = _kernel_asm("ghf_planes_gather_forms")
    src = open(os.path.join(ROOT, "golden-huffman_amd", "csrc", "ghf_planes_gather_forms.hip")).read()
    stage_max = eval(re.search(r"constexpr uint32_t kFormsStageMax = ([0-9 *]+);", src).group(1))  # the most a launch asks for
    assert 65 * 512 <= stage_max and 17 * 512 + 11 * 512 <= stage_max  # one plane at either row cap fits
    for sym in KERNELS:
        meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
        assert meta, sym
        head = text[: meta.start()]
        blk = head[head.rindex("- .agpr_count") :] + meta.group(1)  # this kernel's metadata block: the fields in front of .name too
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))  # the tables; the stage is the launch's dynamic LDS
        assert "hidden_dynamic_lds_size" in blk, sym
        assert 0 < lds and lds + stage_max <= LDS_BUDGET, (sym, lds)  # two workgroups per CU at the longest rows
        body = text[text.index(sym + ":") :]
        body = body[: body.index(".Lfunc_end")]
        assert "scratch_" not in body and "v_writelane" not in body, sym
        assert "ds_write_b128" in body and "global_store_byte" in body, sym  # the stage's stores and the way out of it
        assert "flat_load" not in body and "flat_store" not in body, sym  # the pointers that went through LDS are device memory again
