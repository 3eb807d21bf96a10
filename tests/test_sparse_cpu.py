"""CPU (-m "not gpu"): the zero-suppressed byte-plane calls (ghf_sparse_mask_bytes, ghf_sparse_split, ghf_sparse_merge,
ghf_compress_planes_sparse[_delta], ghf_decode_planes_sparse[_delta]) are exported, bound and declared
at the end of the header, a null context is refused without a device, the host-only size is right, and a resource guard
keeps the five kernels of ghf_sparse.hip free of spills and scratch and at the LDS that DESIGN.md states.  In the style of
tests/test_planes_delta_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
ARGC = {"ghf_sparse_split": 7, "ghf_sparse_merge": 6, "ghf_compress_planes_sparse": 12, "ghf_compress_planes_sparse_delta": 13,
        "ghf_decode_planes_sparse": 12, "ghf_decode_planes_sparse_delta": 13}
METHODS = ("sparse_split", "sparse_merge", "compress_planes_sparse", "compress_planes_sparse_delta", "decode_planes_sparse",
           "decode_planes_sparse_delta", "sparse_mask_bytes")
# kernel -> its static LDS in bytes, as DESIGN.md section 20 states it
KERNELS = {"_ZN3ghf20k_sparse_split_countEPKhmPhPm": 512, "_ZN3ghf20k_sparse_merge_countEPKhmPmPi": 512,
           "_ZN3ghf13k_sparse_scanEPKmjPmmS2_Pi": 2048, "_ZN3ghf19k_sparse_split_moveEPKhmPhmPKm": 4128,
           "_ZN3ghf19k_sparse_merge_moveEPKhS1_mPhPKmPKi": 4128}
SHORT = {"k_sparse_split_count": 512, "k_sparse_merge_count": 512, "k_sparse_scan": 2048, "k_sparse_split_move": 4128,
         "k_sparse_merge_move": 4128}


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def header():
    return open(os.path.join(ROOT, "include", "ghf.h")).read()


def declaration(hdr, name, ret="int"):
    """the argument list of a declaration, comments removed"""
    decl = re.search(r"^%s %s\(([^;]*)\);" % (ret, name), hdr, flags=re.M | re.S)
    assert decl, name
    return re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)


def test_library_exports_the_sparse_entry_points(ghf):
    L = ghf.lib()
    hdr = header()
    for name, argc in ARGC.items():
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert len(getattr(L, name).argtypes) == argc, name
        assert len(declaration(hdr, name).split(",")) == argc, name
    for plain in ("ghf_compress_planes_sparse", "ghf_decode_planes_sparse"):
        # the _delta form is the plain form with d_base added
        assert ARGC[plain + "_delta"] == ARGC[plain] + 1
        assert "const uint8_t* d_base" in declaration(hdr, plain + "_delta") and "d_base" not in declaration(hdr, plain)
    assert "ghf_sparse_mask_bytes" in ghf.EXPORTS and len(L.ghf_sparse_mask_bytes.argtypes) == 1
    assert len(declaration(hdr, "ghf_sparse_mask_bytes", ret="size_t").split(",")) == 1
    for m in METHODS:
        assert hasattr(ghf.Context, m), m
    assert ghf.SPARSE_AUTO == 0x80000000 and re.search(r"^#define GHF_SPARSE_AUTO 0x80000000u$", hdr, flags=re.M)


def test_the_declarations_sit_at_the_end_of_the_header(ghf):
    """behind ghf_crs_sync_piece, the last declaration the header had, and so outside every byte-plane section whose comments
    other tests count; the comment directly in front of every declaration says that the reference has nothing like it and
    names the lines it generalises"""
    hdr = header()
    sec = hdr.index("/* ---- zero-suppressed byte planes")
    assert hdr.index("int ghf_crs_sync_piece(") < sec
    assert hdr.index("/* ---- byte planes against a base tensor") < hdr.index("/* Multi-GPU decode of a stream") < sec
    block = hdr[sec : hdr.index("#ifdef __cplusplus", sec)]
    for name in list(ARGC) + ["ghf_sparse_mask_bytes"]:
        assert hdr.count(name + "(") == block.count(name + "("), name  # declared, and spoken of, nowhere else
        at = block.index("%s %s(" % ("size_t" if name == "ghf_sparse_mask_bytes" else "int", name))
        comment = block[:at].rstrip()
        assert comment.endswith("*/"), name
        comment = comment[comment.rindex("/*") :]
        assert comment.startswith("/* No reference counterpart"), name
        assert re.search(r"include/(compressor|encoder)\.h:\d+-\d+", comment), name
    assert block.count("No reference counterpart") == len(ARGC) + 1
    intro = block[: block.index("#define GHF_SPARSE_AUTO")]
    assert "LSB first" in intro and "the bits behind n in the last mask byte are 0" in intro
    assert "16-byte aligned" in intro and "GHF_E_INVAL" in intro and "GHF_E_EMPTY" in intro and "GHF_E_CAP" in intro
    assert "d_base == d_out is allowed" in intro
    assert "SYNCHRONISES with the host ONCE" in block and "a rule, not a minimum" in block


def test_a_null_context_is_refused_without_a_device(ghf):
    """The call-level checks come before anything touches HIP.  With no device there is no context, so the null context is
    what answers here for every width and every mask, good or bad; the other refusals are exercised on a live context in
    tests/test_gpu_sparse.py."""
    L = ghf.lib()
    C = ghf.C
    idx = (ghf.Index * 16)()
    vp16, sz16 = (C.c_void_p * 16)(*[4096] * 16), (C.c_size_t * 16)(*[64] * 16)
    n_vals = (C.c_size_t * 8)(*[3] * 8)
    chosen = C.c_uint(0)
    slot = ghf.planes_slot_bytes(64)
    d_in, d_base, d_out, d_codes, d_bytes = 4096, 8192, 1 << 20, 1 << 21, 1 << 22
    for e in (2, 4, 8, 0, 1, 3, 16):
        for mask in (0, 1, 2, 3, 0xFF, 1 << 8, ghf.SPARSE_AUTO, ghf.SPARSE_AUTO | 1):
            for ix in (None, idx):
                assert L.ghf_compress_planes_sparse(None, d_in, 64, e, mask, d_out, slot, d_bytes, d_codes, ix, C.byref(chosen),
                                                    n_vals) == E_INVAL, (e, mask)
                assert L.ghf_compress_planes_sparse_delta(None, d_in, d_base, 64, e, mask, d_out, slot, d_bytes, d_codes, ix,
                                                          C.byref(chosen), n_vals) == E_INVAL, (e, mask)
                assert L.ghf_decode_planes_sparse(None, vp16, sz16, d_codes, ix, mask, n_vals, 64, e, d_out, 64 * 8, d_bytes) == E_INVAL
                assert L.ghf_decode_planes_sparse_delta(None, vp16, sz16, d_codes, ix, d_base, mask, n_vals, 64, e, d_out, 64 * 8,
                                                        d_bytes) == E_INVAL, (e, mask)
    for n in (0, 1, 64, 4097):
        assert L.ghf_sparse_split(None, d_in, n, d_out, d_base, n, d_bytes) == E_INVAL, n
        assert L.ghf_sparse_merge(None, d_in, d_base, 3, n, d_out) == E_INVAL, n
    assert L.ghf_sparse_split(None, None, 0, None, None, 0, None) == E_INVAL
    assert L.ghf_sparse_merge(None, None, None, 0, 0, None) == E_INVAL
    assert L.ghf_compress_planes_sparse(None, None, 0, 2, 0, None, 0, None, None, None, None, None) == E_INVAL
    assert L.ghf_compress_planes_sparse_delta(None, None, None, 0, 2, 0, None, 0, None, None, None, None, None) == E_INVAL
    assert L.ghf_decode_planes_sparse(None, None, None, None, None, 0, None, 0, 2, None, 0, None) == E_INVAL
    assert L.ghf_decode_planes_sparse_delta(None, None, None, None, None, None, 0, None, 0, 2, None, 0, None) == E_INVAL


def test_sparse_mask_bytes(ghf):
    want = {0: 0, 1: 1, 8: 1, 9: 2, (1 << 40) + 1: (1 << 37) + 1}
    for n, b in want.items():
        assert ghf.sparse_mask_bytes(n) == b == (n + 7) // 8, n
    assert ghf.Context.sparse_mask_bytes(9) == 2


def test_the_exported_geometry_is_the_source_s(ghf):
    src = open(os.path.join(ROOT, "golden-huffman_amd", "csrc", "ghf_internal.h")).read()
    assert re.search(r"constexpr uint32_t kSparseTile = (\d+);", src).group(1) == str(ghf.SPARSE_TILE)
    assert re.search(r"constexpr uint32_t kSparseGroups = 256 \* 16;", src) and ghf.SPARSE_GROUPS == 256 * 16
    assert ghf.SPARSE_SCAN == ghf.SPARSE_GROUPS  # one count per workgroup: the scan takes them in one step
    assert ghf.SPARSE_GROUPS == ghf.PLANES_GROUPS


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
    """the metadata fields of the kernel"""
    meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
    assert meta, sym
    head = text[: meta.start()]
    head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
    blk = head + meta.group(1)
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
            for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_count")}


def test_design_states_the_lds_of_every_kernel():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 20.") :]
    for name, lds in SHORT.items():
        row = re.search(r"^\| `%s` \|[^\n]*$" % name, sec, flags=re.M)
        assert row, name
        assert re.search(r"\| %d \|" % lds, row.group(0)), (name, row.group(0))


@pytest.mark.parametrize("sym", list(KERNELS))
def test_sparse_kernels_have_no_spills_no_scratch_and_the_stated_lds(ghf, sym):
    """from the kernel metadata alone: nothing spilled, no private segment, and the static LDS of DESIGN.md section 20 (which
    test_design_states_the_lds_of_every_kernel holds against the same numbers); at most 128 registers: a resident round of
    sixteen one-wave workgroups per CU"""
    res = _resources(_kernel_asm("ghf_sparse"), sym)
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (sym, res)
    assert res["private_segment_fixed_size"] == 0, (sym, res)
    assert res["group_segment_fixed_size"] == KERNELS[sym], (sym, res)
    assert res["vgpr_count"] <= 128, (sym, res)
