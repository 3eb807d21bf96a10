"""CPU (-m "not gpu"): ghf_decode_images_batch is exported, bound and declared, and an ISA guard keeps both
instantiations of its one-workgroup-per-item kernel scratch-free and within 40 KiB of LDS -- four workgroups per CU, the
budget of k_decode_batch (DESIGN.md sections 9 and 10).  In the style of tests/test_batch_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
IMAGES_SYMBOLS = ["ghf_decode_images_batch", "ghf_decode_images_batch_stats"]
KERNELS = ["_ZN3ghf21k_decode_images_batchILb1EEEvNS_17BatchImagesParamsE",  # kWrite: decode
           "_ZN3ghf21k_decode_images_batchILb0EEEvNS_17BatchImagesParamsE"]  # sizes only


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_images_entry_points(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    for name in IMAGES_SYMBOLS:
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert re.search(r"^int %s\(ghf_ctx\* ctx," % name, hdr, flags=re.M), name
    assert hasattr(ghf.Context, "decode_images_batch")


def test_null_arguments_are_refused_without_a_device(ghf):
    """the call-level checks come before anything touches HIP"""
    L = ghf.lib()
    assert L.ghf_decode_images_batch(None, None, None, 0, None, None, None, None, None) == E_INVAL
    assert L.ghf_decode_images_batch_stats(None, None) == E_INVAL


def _kernel_asm(name):
    """gfx950 ISA text of golden-huffman_amd/csrc/<name>.hip, built with the Makefile's own flags"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "golden-huffman_amd", "csrc", name + ".hip")
    mk = open(os.path.join(ROOT, "golden-huffman_amd", "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, flags=re.M).group(1)
    flags = flags.replace("$(ARCH)", "gfx950").replace("$(ROOT)", ROOT).replace("$(HERE)", os.path.join(ROOT, "golden-huffman_amd") + "/")
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        r = subprocess.run([hipcc] + flags.split() + ["--cuda-device-only", "-S", "-o", os.path.join(td, "k.s"), src],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(os.path.join(td, "k.s")).read()


def test_images_kernel_uses_no_scratch_and_keeps_its_lds_budget():
    text = _kernel_asm("ghf_batch")
    for sym in KERNELS:
        meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
        assert meta, sym
        head = text[: meta.start()]
        head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
        blk = head + meta.group(1)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 40 * 1024, sym
        body = text[text.index(sym + ":") :]
        body = body[: body.index(".Lfunc_end")]
        assert "scratch_" not in body, sym
