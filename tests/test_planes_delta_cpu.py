"""CPU (-m "not gpu"): the byte-plane calls against a base tensor (ghf_histogram_planes_delta, ghf_planes_split_delta,
ghf_planes_merge_delta, ghf_planes_merge_range_delta, ghf_compress_planes_delta, ghf_decode_planes_delta,
ghf_decode_planes_range_delta) are exported, bound and declared where the header keeps the
byte-plane calls, a null context is refused without a device, and an ISA guard keeps the twelve new kernels free of spills
and scratch and at the LDS of their parents.  In the style of tests/test_planes_coded_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
ARGC = {"ghf_histogram_planes_delta": 7, "ghf_planes_split_delta": 7, "ghf_planes_merge_delta": 7,
        "ghf_planes_merge_range_delta": 8, "ghf_compress_planes_delta": 11, "ghf_decode_planes_delta": 11,
        "ghf_decode_planes_range_delta": 14}
PLAIN_ARGC = {"ghf_histogram_planes": 6, "ghf_planes_split": 6, "ghf_planes_merge": 6, "ghf_planes_merge_range": 7,
              "ghf_compress_planes_coded": 10, "ghf_decode_planes": 10, "ghf_decode_planes_range": 13}
METHODS = ("histogram_planes_delta", "planes_split_delta", "planes_merge_delta", "planes_merge_range_delta",
           "compress_planes_delta", "decode_planes_delta", "decode_planes_range_delta")
WIDTHS = (2, 4, 8)
HIST_LDS = 32768  # bins[256][32] u32, the parent's
HIST_KERNELS = {e: "_ZN3ghf24k_histogram_planes_deltaILi%dEEEvPKhS2_mPy" % e for e in WIDTHS}
TILE_KERNELS = {e: ["_ZN3ghf20k_planes_split_deltaILi%dEEEvPKhS2_mPhm" % e,
                    "_ZN3ghf20k_planes_merge_deltaILi%dEEEvPKhmS2_mPhPKi" % e,
                    "_ZN3ghf26k_planes_merge_range_deltaILi%dEEEvPKhmjS2_mPhPKi" % e] for e in WIDTHS}


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_delta_entry_points(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    for (name, argc), (plain, plain_argc) in zip(ARGC.items(), PLAIN_ARGC.items()):
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert len(getattr(L, name).argtypes) == argc, name
        decl = re.search(r"^int %s\(([^;]*)\);" % name, hdr, flags=re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == argc, name
        assert "const uint8_t* d_base" in decl.group(1), name
        # the plain call it mirrors, with d_base added
        assert argc == plain_argc + 1 and len(getattr(L, plain).argtypes) == plain_argc, (name, plain)
    for m in METHODS:
        assert hasattr(ghf.Context, m), m


def test_the_declarations_sit_in_the_byte_plane_part_of_the_header(ghf):
    """behind "byte planes: an element range", in front of the multi-GPU calls, and not inside "byte planes in stages",
    whose comments tests/test_planes_coded_cpu.py counts; the comment directly in front of every declaration says that the
    reference has nothing like it and names the lines it generalises"""
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    lo, hi = hdr.index("/* ---- byte planes: an element range"), hdr.index("/* Multi-GPU decode of a stream")
    sec = hdr.index("/* ---- byte planes against a base tensor")
    assert hdr.index("/* ---- byte planes: typed elements") < hdr.index("/* ---- byte planes in stages") < lo < sec < hi
    assert hdr.index("int ghf_decode_planes_range(") < sec
    stages = hdr[hdr.index("/* ---- byte planes in stages") : hdr.index("/* ---- shared-code batches of typed elements")]
    block = hdr[sec:hi]
    for name in ARGC:
        assert name + "(" not in stages, name
        at = block.index("int %s(" % name)
        comment = block[:at].rstrip()
        assert comment.endswith("*/"), name
        comment = comment[comment.rindex("/*") :]
        assert "No reference counterpart" in comment, name
        assert re.search(r"include/(compressor|encoder)\.h:\d+-\d+", comment), name
    assert block.count("No reference counterpart") == len(ARGC)
    intro = block[: block.index("int ghf_histogram_planes_delta(")]
    assert "d_base == d_out is allowed" in intro and "undefined" in intro  # the one overlap that is defined
    assert "16-byte aligned" in intro and "GHF_E_INVAL" in intro
    assert "SYNCHRONISES" in block and "UNSPECIFIED" in block


def test_a_null_context_is_refused_without_a_device(ghf):
    """The call-level checks come before anything touches HIP.  With no device there is no context, so the null context is
    what answers here for every width, good or bad; the other refusals are exercised on a live context in
    tests/test_gpu_planes_delta.py."""
    L = ghf.lib()
    idx = (ghf.Index * 8)()
    vp8, sz8 = (ghf.C.c_void_p * 8)(*[4096] * 8), (ghf.C.c_size_t * 8)(*[64] * 8)
    infos = (ghf.SeekInfo * 8)()
    slot = ghf.planes_slot_bytes(64)
    d_in, d_base, d_out, d_codes, d_bytes = 4096, 8192, 1 << 20, 1 << 21, 1 << 22
    for e in (2, 4, 8, 0, 1, 3, 16):
        for flags in (0, ghf.HIST_COVER_ALL, 2):
            assert L.ghf_histogram_planes_delta(None, d_in, d_base, 64, e, flags, d_out) == E_INVAL, e
        assert L.ghf_planes_split_delta(None, d_in, d_base, 64, e, d_out, 64) == E_INVAL, e
        assert L.ghf_planes_merge_delta(None, d_in, 64, d_base, 64, e, d_out) == E_INVAL, e
        assert L.ghf_planes_merge_delta(None, d_in, 64, d_out, 64, e, d_out) == E_INVAL, e
        assert L.ghf_planes_merge_range_delta(None, d_in, 64, d_base, 5, 32, e, d_out) == E_INVAL, e
        for flags in (0, ghf.PLANES_BUILD_CODES, 2):
            for ix in (None, idx):
                assert L.ghf_compress_planes_delta(None, d_in, d_base, 64, e, d_codes, flags, d_out, slot, d_bytes, ix) == E_INVAL, e
        for ix in (None, idx):
            assert L.ghf_decode_planes_delta(None, vp8, sz8, d_codes, ix, d_base, 64, e, d_out, 64 * 8, d_bytes) == E_INVAL, e
        assert L.ghf_decode_planes_range_delta(None, vp8, sz8, d_codes, idx, None, None, None, d_base, e, 5, 32, d_out, 64 * 8) == E_INVAL, e
        assert L.ghf_decode_planes_range_delta(None, vp8, sz8, d_codes, None, infos, vp8, sz8, d_base, e, 5, 32, d_out, 64 * 8) == E_INVAL, e
    assert L.ghf_histogram_planes_delta(None, None, None, 0, 2, 0, None) == E_INVAL
    assert L.ghf_planes_split_delta(None, None, None, 0, 2, None, 0) == E_INVAL
    assert L.ghf_planes_merge_delta(None, None, 0, None, 0, 2, None) == E_INVAL
    assert L.ghf_planes_merge_range_delta(None, None, 0, None, 0, 0, 2, None) == E_INVAL
    assert L.ghf_compress_planes_delta(None, None, None, 0, 2, None, 0, None, 0, None, None) == E_INVAL
    assert L.ghf_decode_planes_delta(None, None, None, None, None, None, 0, 2, None, 0, None) == E_INVAL
    assert L.ghf_decode_planes_range_delta(None, None, None, None, None, None, None, None, None, 2, 0, 0, None, 0) == E_INVAL


_asm = {}


def _kernel_asm(name):
    """gfx950 ISA text of golden-huffman_amd/csrc/<name>.hip, built with the Makefile's own flags (once per unit)"""
    if name in _asm:
        return _asm[name]
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
        _asm[name] = open(os.path.join(td, "k.s")).read()
    return _asm[name]


def _resources(text, sym):
    """(metadata fields of the kernel, its body)"""
    meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
    assert meta, sym
    head = text[: meta.start()]
    head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
    blk = head + meta.group(1)
    body = text[text.index(sym + ":") :]
    body = body[: body.index(".Lfunc_end")]
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
            for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")}, body


def _no_spills_no_scratch(sym, res, body):
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (sym, res)
    assert res["private_segment_fixed_size"] == 0, (sym, res)
    assert "scratch_" not in body, sym


@pytest.mark.parametrize("e", WIDTHS)
def test_delta_histogram_kernel_keeps_the_resources_of_its_parent(ghf, e):
    """no spills, no scratch, the parent's 32 KiB of LDS and at most 128 registers: four workgroups of four waves on a CU"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%d" % HIST_LDS in design[design.index("## 19.") :], "DESIGN.md section 19 states the LDS the kernel is held to"
    text = _kernel_asm("ghf_planes_hist")
    sym = HIST_KERNELS[e]
    res, body = _resources(text, sym)
    _no_spills_no_scratch(sym, res, body)
    assert res["group_segment_fixed_size"] == HIST_LDS, (sym, res)
    assert res["vgpr_count"] <= 128, (sym, res)
    parent, _ = _resources(text, "_ZN3ghf18k_histogram_planesILi%dEEEvPKhmPy" % e)
    assert parent["group_segment_fixed_size"] == res["group_segment_fixed_size"]
    # both streams carry the non-temporal hint in the tile loop: 4 + 4 loads per step, two steps unrolled, and the first tile
    assert len(re.findall(r"global_load_dwordx4 .* nt\b", body)) >= 24, sym


@pytest.mark.parametrize("e", WIDTHS)
def test_delta_split_and_merge_kernels_keep_the_resources_of_their_parents(ghf, e):
    """no spills, no scratch, the parents' LDS tile: 64 * max(E, 4) / E rows of (E + 1) vectors"""
    text = _kernel_asm("ghf_planes")
    lds = ghf.PLANES_TILE[e] // 16 * (e + 1) * 16
    parents = ["_ZN3ghf14k_planes_splitILi%dEEEvPKhmPhm" % e, "_ZN3ghf14k_planes_mergeILi%dEEEvPKhmmPhPKi" % e,
               "_ZN3ghf20k_planes_merge_rangeILi%dEEEvPKhmjmPhPKi" % e]
    vec = max(e, 4)
    for sym, parent in zip(TILE_KERNELS[e], parents):
        res, body = _resources(text, sym)
        _no_spills_no_scratch(sym, res, body)
        assert res["group_segment_fixed_size"] == lds, (sym, res)
        assert _resources(text, parent)[0]["group_segment_fixed_size"] == lds, parent
        # the access shape of the tile loop: every 16-byte access carries the non-temporal hint, and the base adds max(E, 4)
        # loads per tile to the parent's
        loads = len(re.findall(r"global_load_dwordx4 .* nt\b", body))
        parent_loads = len(re.findall(r"global_load_dwordx4 .* nt\b", _resources(text, parent)[1]))
        assert loads == parent_loads + vec, (sym, loads, parent_loads)
        assert len(re.findall(r"global_load_dwordx4 ", body)) == loads, sym
        stores = re.findall(r"global_store_dwordx4 .*", body)
        assert len(stores) == vec and all(re.search(r" nt\b", s) for s in stores), (sym, stores)
        # the base loads of a tile are issued before its first LDS instruction
        first_lds = re.search(r"\bds_(write|read)", body).start()
        assert len(re.findall(r"global_load_dwordx4 ", body[:first_lds])) == loads, sym
