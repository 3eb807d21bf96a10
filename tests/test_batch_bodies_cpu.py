"""CPU (-m "not gpu"): ghf_decode_bodies_batch_shared is exported, bound and declared, its call-level refusals come back
without a device, and an ISA guard keeps both instantiations of k_decode_bodies_batch_shared scratch-free and within
40 KiB of LDS -- four workgroups per CU, the budget of its siblings (DESIGN.md sections 10, 12 and 13).  In the style of
tests/test_batch_shared_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
NAME = "ghf_decode_bodies_batch_shared"
KERNELS = ["_ZN3ghf28k_decode_bodies_batch_sharedILb1EEEvNS_23BatchSharedBodiesParamsE",  # kWrite: decode
           "_ZN3ghf28k_decode_bodies_batch_sharedILb0EEEvNS_23BatchSharedBodiesParamsE"]  # sizes only


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_bodies_entry_point(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    assert NAME in ghf.EXPORTS
    assert getattr(L, NAME) is not None
    assert len(getattr(L, NAME).argtypes) == 9
    assert re.search(r"^int %s\(ghf_ctx\* ctx," % NAME, hdr, flags=re.M)
    assert hasattr(ghf.Context, "decode_bodies_batch_shared")
    # the old advice (prepend the header to every body) is gone from the header; the stats comment names the new call
    assert "prepend the header" not in hdr
    stats = hdr[hdr.index("d_stats (device u64[2]") : hdr.index("int ghf_decode_images_batch_stats(")]
    assert NAME in stats


def test_null_arguments_are_refused_without_a_device(ghf):
    """the call-level checks come before anything touches HIP: no context, and the count of 0 does not excuse them"""
    L = ghf.lib()
    fn = getattr(L, NAME)
    assert fn(None, None, None, None, 0, None, None, None, None) == E_INVAL
    assert fn(None, 16, 16, 16, 1, None, None, 16, 16) == E_INVAL  # every array named, still no context


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


def test_bodies_kernel_uses_no_scratch_and_keeps_its_lds_budget():
    text = _kernel_asm("ghf_batch_shared")
    for sym in KERNELS:
        meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
        assert meta, sym
        head = text[: meta.start()]
        head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
        blk = head + meta.group(1)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 40 * 1024, sym
        body = text[text.index(sym + ":") :]
        body = body[: body.index(".Lfunc_end")]
        assert "scratch_" not in body, sym
