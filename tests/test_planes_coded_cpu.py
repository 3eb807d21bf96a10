"""CPU (-m "not gpu"): the staged byte-plane calls (ghf_histogram_planes, ghf_planes_image_bytes,
ghf_compress_planes_coded) are exported, bound and declared, a null context is refused without a device, the constants the
binding names are the source's, and an ISA guard keeps every k_histogram_planes<E> free of spills and scratch and at the
32 KiB of LDS DESIGN.md section 18 states.  In the style of tests/test_planes_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
ARGC = {"ghf_histogram_planes": 6, "ghf_planes_image_bytes": 5, "ghf_compress_planes_coded": 10}
LDS_BYTES = 32768      # bins[256][32] u32 for every E
LDS_TWO_PER_CU = 80 * 1024
KERNELS = ["_ZN3ghf18k_histogram_planesILi%dEEEvPKhmPy" % e for e in (2, 4, 8)]


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_three_staged_entry_points(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    for name, argc in ARGC.items():
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert len(getattr(L, name).argtypes) == argc, name
        decl = re.search(r"^int %s\(([^;]*)\);" % name, hdr, flags=re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == argc, name
    assert re.search(r"^#define GHF_PLANES_BUILD_CODES 1u$", hdr, flags=re.M) and ghf.PLANES_BUILD_CODES == 1
    for m in ("histogram_planes", "planes_image_bytes", "compress_planes_coded"):
        assert hasattr(ghf.Context, m), m
    # the declarations live in the byte-plane part of the header; every comment says that the reference has nothing like it
    # and which lines it generalises
    block = hdr[hdr.index("/* ---- byte planes in stages") : hdr.index("/* ---- shared-code batches of typed elements")]
    assert hdr.index("/* ---- byte planes: typed elements") < hdr.index("/* ---- byte planes in stages") < hdr.index("/* Multi-GPU decode of a stream")
    assert block.count("No reference counterpart") == 3
    assert block.count("include/compressor.h:62-73") >= 3 and block.count("include/encoder.h:123-150") >= 3
    assert "UNSPECIFIED" in block  # d_out_bytes behind a latched status
    nocode = hdr[hdr.index("GHF_E_NOCODE = 10") :][:400]
    assert "ghf_compress_planes_coded" in nocode


def test_the_constants_the_binding_names_are_the_sources(ghf):
    src = open(os.path.join(ROOT, "golden-huffman_amd", "csrc", "ghf_internal.h")).read()

    def const(name):
        m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src)
        assert m, name
        expr = re.sub(r"\bk[A-Z]\w+", lambda k: str(const(k.group(0))), m.group(1))  # products of literals and other constants
        assert re.fullmatch(r"[\d\s*]+", expr), (name, expr)
        return eval(expr)

    assert const("kPlanesHistThreads") == 256
    assert ghf.PLANES_HIST_GROUPS == const("kPlanesHistGroups")
    assert ghf.PLANES_HIST_TILE_BYTES == const("kPlanesHistTileVecs") * 16
    assert ghf.PLANES_HIST_FLUSH_TILES == const("kPlanesHistFlushTiles")
    assert const("kPlanesHistCols") * 256 * 4 == LDS_BYTES


def test_a_null_context_is_refused_without_a_device(ghf):
    """The call-level checks come before anything touches HIP.  With no device there is no context, so the null context is
    what answers here for every width, good or bad; the other refusals are exercised on a live context in
    tests/test_gpu_planes_coded.py."""
    L = ghf.lib()
    idx = (ghf.Index * 8)()
    slot = ghf.planes_slot_bytes(64)
    for e in (2, 4, 8, 0, 1, 3, 16):
        for flags in (0, ghf.HIST_COVER_ALL, 2):
            assert L.ghf_histogram_planes(None, 4096, 64, e, flags, 8192) == E_INVAL, e
        assert L.ghf_planes_image_bytes(None, 4096, 1 << 20, e, 8192) == E_INVAL, e
        for flags in (0, ghf.PLANES_BUILD_CODES, 2):
            assert L.ghf_compress_planes_coded(None, 4096, 64, e, 1 << 20, flags, 8192, slot, 1 << 21, None) == E_INVAL, e
            assert L.ghf_compress_planes_coded(None, 4096, 64, e, 1 << 20, flags, 8192, slot, 1 << 21, idx) == E_INVAL, e
    assert L.ghf_histogram_planes(None, None, 0, 2, 0, None) == E_INVAL
    assert L.ghf_planes_image_bytes(None, None, None, 2, None) == E_INVAL
    assert L.ghf_compress_planes_coded(None, None, 0, 2, None, 0, None, 0, None, None) == E_INVAL


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


def test_histogram_kernels_use_no_scratch_and_the_lds_the_design_states(ghf):
    """metadata only: spill counts, private segment, LDS bytes; and no scratch access in the body"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 18.") :]
    assert "%d" % LDS_BYTES in sec, "DESIGN.md section 18 states the LDS bytes the kernels are held to"
    assert LDS_BYTES <= LDS_TWO_PER_CU
    text = _kernel_asm("ghf_planes_hist")
    for sym in KERNELS:
        meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
        assert meta, sym
        head = text[: meta.start()]
        head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
        blk = head + meta.group(1)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert lds == LDS_BYTES, (sym, lds)
        # four workgroups of four waves on a CU need at most 128 registers per lane
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 128, sym
        body = text[text.index(sym + ":") :]
        body = body[: body.index(".Lfunc_end")]
        assert "scratch_" not in body, sym
