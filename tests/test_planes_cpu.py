"""CPU (-m "not gpu"): the byte-plane calls (ghf_planes_slot_bytes, ghf_planes_split, ghf_planes_merge,
ghf_compress_planes, ghf_decode_planes) are exported, bound and declared, their call-level refusals come back without a
device, and an ISA guard keeps all six instantiations of k_planes_split / k_planes_merge free of spills and scratch and
within the 9 KiB of LDS per workgroup DESIGN.md section 14 states.  In the style of tests/test_batch_bodies_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
ARGC = {"ghf_planes_slot_bytes": 1, "ghf_planes_split": 6, "ghf_planes_merge": 6, "ghf_compress_planes": 9, "ghf_decode_planes": 10}
LDS_BUDGET = 9 * 1024  # 64 rows of (8 + 1) vectors at E = 8
KERNELS = ["_ZN3ghf14k_planes_splitILi%dEEEvPKhmPhm" % e for e in (2, 4, 8)] + \
          ["_ZN3ghf14k_planes_mergeILi%dEEEvPKhmmPhPKi" % e for e in (2, 4, 8)]


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_five_plane_entry_points(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    for name, argc in ARGC.items():
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert len(getattr(L, name).argtypes) == argc, name
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, hdr, flags=re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == argc, name
    assert re.search(r"^#define GHF_PLANES_MAX 8$", hdr, flags=re.M) and ghf.PLANES_MAX == 8
    for m in ("planes_split", "planes_merge", "compress_planes", "decode_planes"):
        assert hasattr(ghf.Context, m), m
    # every declaration's comment says that the reference has nothing like it and which lines it generalises
    block = hdr[hdr.index("/* ---- byte planes") : hdr.index("/* Multi-GPU decode of a stream")]
    assert block.count("No reference counterpart") >= 6
    assert "include/compressor.h:62-73" in block and "include/compressor.h:87-92" in block
    assert "SYNCHRONISES" in block  # ghf_decode_planes(indexes = NULL) says that it waits for the stream


def test_slot_bytes_is_the_compress_bound_rounded_to_16(ghf):
    L = ghf.lib()
    for n in (0, 1, 15, 16, 17, 4097, 65536, 65539, (1 << 30) + 7):
        want = (L.ghf_compress_bound(n) + 15) & ~15
        assert L.ghf_planes_slot_bytes(n) == want == ghf.planes_slot_bytes(n), n
        assert want % 16 == 0 and want >= L.ghf_compress_bound(n)


def test_a_null_context_is_refused_without_a_device(ghf):
    """The call-level checks come before anything touches HIP.  With no device there is no context, so the null context is
    what answers here for every width, good or bad; the refusal of elem_bytes 0, 1, 3 and 16 as such is exercised on a live
    context in tests/test_gpu_planes.py."""
    L = ghf.lib()
    idx = (ghf.Index * 8)()
    ptrs = (ghf.C.c_void_p * 8)(*[4096] * 8)
    sizes = (ghf.C.c_size_t * 8)(*[2048] * 8)
    for e in (2, 4, 8, 0, 1, 3, 16):  # no width excuses the missing context
        assert L.ghf_planes_split(None, 4096, 64, e, 8192, 64) == E_INVAL, e
        assert L.ghf_planes_merge(None, 8192, 64, 64, e, 4096) == E_INVAL, e
        assert L.ghf_compress_planes(None, 4096, 64, e, 8192, ghf.planes_slot_bytes(64), 1 << 20, None, None) == E_INVAL, e
        assert L.ghf_compress_planes(None, 4096, 64, e, 8192, ghf.planes_slot_bytes(64), 1 << 20, 1 << 21, idx) == E_INVAL, e
        assert L.ghf_decode_planes(None, ptrs, sizes, 1 << 20, None, 64, e, 4096, 64 * 16, None) == E_INVAL, e
        assert L.ghf_decode_planes(None, ptrs, sizes, 1 << 20, idx, 64, e, 4096, 64 * 16, 1 << 21) == E_INVAL, e
    assert L.ghf_planes_split(None, None, 0, 2, None, 0) == E_INVAL
    assert L.ghf_decode_planes(None, None, None, None, None, 0, 2, None, 0, None) == E_INVAL


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


def test_plane_kernels_use_no_scratch_and_keep_their_lds_budget(ghf):
    text = _kernel_asm("ghf_planes")
    for sym, e in zip(KERNELS, (2, 4, 8, 2, 4, 8)):
        meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
        assert meta, sym
        head = text[: meta.start()]
        head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
        blk = head + meta.group(1)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert 0 < lds <= LDS_BUDGET, (sym, lds)
        # the kernel's LDS tile holds tile / 16 rows of (E + 1) vectors: the tile the binding names is the kernel's own
        assert lds == ghf.PLANES_TILE[e] // 16 * (e + 1) * 16, (sym, lds)
        body = text[text.index(sym + ":") :]
        body = body[: body.index(".Lfunc_end")]
        assert "scratch_" not in body, sym
