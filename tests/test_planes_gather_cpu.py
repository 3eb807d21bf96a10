"""CPU (-m "not gpu"): ghf_decode_planes_gather is exported, bound and declared, a null context is refused without a device,
the numpy model of the call (tests/gather_model.py) agrees with the oracle on where every covered run starts and on what a
row is made of, and an ISA guard keeps the three instantiations of k_decode_planes_gather free of spills, scratch and a
private segment and, with the largest stage a launch asks for, within 64 KiB of LDS.  In the style of tests/test_planes_range_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import gather_model as gm
import gather_planes as gp
import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
NAME, ARGC = "ghf_decode_planes_gather", 17
LDS_BUDGET = 64 * 1024
KERNELS = ["_ZN3ghf22k_decode_planes_gatherILi%dEEEvNS_18PlanesGatherParamsEj" % e for e in (2, 4, 8)]


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_gather_entry_point(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    block = hdr[hdr.index("/* ---- byte planes in three forms") : hdr.index(" * SURVEY 8(e): one stream sharded")]
    assert NAME in ghf.EXPORTS
    assert getattr(L, NAME) is not None
    assert len(getattr(L, NAME).argtypes) == ARGC
    decl = re.search(r"^int %s\(([^;]*)\);" % NAME, block, flags=re.M | re.S)  # in the byte-planes block, behind the forms family
    assert decl
    assert block.index("int ghf_decode_planes_forms_range(") < decl.start()
    assert len(decl.group(1).split(",")) == ARGC
    comment = block[: decl.start()].rstrip()  # the comment that ends right in front of the declaration
    assert comment.endswith("*/")
    comment = comment[comment.rindex("/*") :]
    assert "No reference counterpart" in comment and "include/compressor.h:87-92" in comment
    assert "READ:" in comment and "WRITTEN:" in comment
    assert re.search(r"^#define GHF_GATHER_MAX_ROW_ELEMS 32768u\b", block, flags=re.M)
    assert ghf.GATHER_MAX_ROW_ELEMS == gm.MAX_ROW_ELEMS == 32768
    assert hasattr(ghf.Context, "decode_planes_gather")


def test_a_null_context_is_refused_without_a_device(ghf):
    """the call-level checks come before anything touches HIP; with no device the null context answers for every width"""
    L = ghf.lib()
    infos = (ghf.SeekInfo * 8)()
    ptrs = (ghf.C.c_void_p * 8)(*[4096] * 8)
    sizes = (ghf.C.c_size_t * 8)(*[2048] * 8)
    for e in (2, 4, 8, 0, 1, 3, 16):
        assert L.ghf_decode_planes_gather(None, ptrs, sizes, 1 << 20, infos, ptrs, sizes, 0, 2048, e, 4096, 1, 16, 4, 8192, 16 * 16,
                                          16384) == E_INVAL, e
        assert L.ghf_decode_planes_gather(None, ptrs, sizes, 1 << 20, infos, ptrs, sizes, 0, 2048, e, 4096, 1, 16, 0, 8192, 16 * 16,
                                          16384) == E_INVAL, e
    assert L.ghf_decode_planes_gather(None, None, None, None, None, None, None, 0, 0, 2, None, 0, 0, 0, None, 0, None) == E_INVAL


# ---------------------------------------------------------------- the model against the oracle
def _rows(n):
    """(first, count) of every row of the GPU test's shapes, and the row at the cap"""
    out = [(i * stride, re_) for re_, stride, ids in gp.row_cases(n) for i in ids]
    return out + ([(700, gm.MAX_ROW_ELEMS)] if n == gp.N_CAP else [])


@pytest.mark.parametrize("n", [gp.N_SMALL, gp.N_CAP])
def test_covered_runs_start_where_the_oracle_puts_them_and_make_up_the_row(n):
    t = gp.tensor(8, n)
    rows = _rows(n)
    assert {c for _, c in rows} >= set(gm.ROW_ELEMS)
    assert n != gp.N_CAP or len(gm.covered(700, gm.MAX_ROW_ELEMS, n)) == 65  # every lane of the run round
    for pl in t.planes:
        cum = np.zeros(n + 1, dtype=np.int64)  # the oracle's cumulative code lengths
        np.cumsum(np.asarray(pl.length, dtype=np.int64)[pl.data], out=cum[1:])
        for first, count in rows:
            runs = gm.covered(first, count, n)
            pieces = []
            for g, k, in_run, skip, take in runs:
                sym0 = g * gm.BLOCK + k * gm.RUN
                assert in_run == min(gm.RUN, n - sym0) and 0 <= skip and 1 <= take and skip + take <= in_run
                assert gm.run_start(pl.table, g, k) == pl.first_bit + int(cum[sym0]), (pl.cls, g, k)
                assert int(gm.records(pl.table)[g]["run"][k]) == int(cum[sym0 + in_run] - cum[sym0])
                pieces.append(pl.data[sym0 + skip : sym0 + skip + take])
            assert len(runs) <= gm.MAX_ROW_ELEMS // gm.RUN + 1
            assert np.array_equal(np.concatenate(pieces), pl.data[first : first + count]), (pl.cls, first, count)
            assert all(gm.block_ok(pl.table, g, pl.stream_bytes) for g in {r[0] for r in runs})


def test_the_planes_come_from_the_code_classes_the_gpu_test_names():
    t = gp.tensor(8)
    by = {p.cls: p for p in t.planes}
    assert t.planes[0].cls == "len12" and by["len12"].max_len > 12 and by["len14"].max_len > 12  # the miss path of the small decoder
    assert by["short"].min_len == 1 and by["short"].max_len <= 4
    assert by["len9"].min_len >= 7 and by["len9"].stream_bytes >= t.n  # near-uniform: what GHF_RAW_AUTO stores raw
    assert by["long"].max_len >= 16
    assert gp.tensor(2).raw_auto == 0 and gp.tensor(4).raw_auto == 0b0100


def test_the_model_decodes_what_the_oracle_wrote_and_sees_a_shifted_run():
    """the model's own decoder, which judges the runs of a damaged table: a true run lands, and in plane 0 -- the plane whose
    table the GPU test damages -- run 4 of block 1 entered one bit late does not (in other planes it does: gather_planes.py)"""
    pl = gp.tensor(2).planes[0]
    dec = gm.Decoder(pl.length, pl.codeword)
    rec = gm.records(pl.table)
    for g, k in ((0, 0), (1, 3), (3, 0)):
        cnt = min(gm.RUN, pl.n - (g * gm.BLOCK + k * gm.RUN))
        start = gm.run_start(pl.table, g, k)
        assert dec.run_bits(pl.stream, pl.stream_bytes, start, cnt) == int(rec[g]["run"][k])
    assert dec.run_bits(pl.stream, pl.stream_bytes, gm.run_start(pl.table, 1, 4) + 1, gm.RUN) != int(rec[1]["run"][4]) - 1
    late = gp.tensor(8).planes[4]  # the len14 slice: the same damage lands there, and the model says so
    assert gm.Decoder(late.length, late.codeword).run_bits(late.stream, late.stream_bytes, gm.run_start(late.table, 1, 4) + 1,
                                                           gm.RUN) == int(gm.records(late.table)[1]["run"][4]) - 1


def test_row_verdicts_of_the_model():
    t = gp.tensor(2)
    n = t.n
    planes = t.model_planes(0)
    assert gm.row_verdict(0, 1, 7, n, planes) == gm.OK
    assert gm.row_verdict(n - 7, 1, 7, n, planes) == gm.OK
    assert gm.row_verdict(n - 6, 1, 7, n, planes) == gm.E_INVAL
    assert gm.row_verdict(n + 1, 1, 7, n, planes) == gm.E_INVAL
    assert gm.row_verdict(1 << 63, 4, 7, n, planes) == gm.E_INVAL
    bad_code = [t.planes[0].model(code_ok=False), planes[1]]
    assert gm.row_verdict(n + 1, 1, 7, n, bad_code) == gm.E_FORMAT  # on every row
    assert gm.row_verdict(n + 1, 1, 7, n, [None, None]) == gm.E_INVAL and gm.row_verdict(5, 1, 7, n, [None, None]) == gm.OK


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


def test_gather_kernels_use_no_scratch_no_spills_and_keep_the_lds_budget(ghf):
    text = _kernel_asm("ghf_planes_gather")
    src = open(os.path.join(ROOT, "golden-huffman_amd", "csrc", "ghf_planes_gather.hip")).read()
    stage_max = eval(re.search(r"constexpr uint32_t kGatherStageMax = ([0-9 *]+);", src).group(1))  # the most a launch asks for
    assert 65 * 512 <= stage_max  # the runs of one plane at the row cap fit
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
