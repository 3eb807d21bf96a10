"""CPU (-m "not gpu"): the host-only half of the shared-code batch calls (the four exports, ghf_compress_batch_shared_bound,
GHF_E_NOCODE's text) and an ISA guard that keeps k_compress_batch_shared and k_decode_batch_shared scratch-free and inside
the LDS budgets DESIGN.md section 12 argues from: 20 KiB (eight workgroups per CU) and 40 KiB (four).  In the style of
tests/test_batch_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHARED_SYMBOLS = ["ghf_histogram_batch", "ghf_compress_batch_shared_bound", "ghf_compress_batch_shared", "ghf_decode_batch_shared"]


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_shared_batch_entry_points(ghf):
    L = ghf.lib()
    for name in SHARED_SYMBOLS:
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    assert re.search(r"GHF_E_NOCODE = 10\b", hdr)
    assert re.search(r"#define GHF_HIST_COVER_ALL 1u\b", hdr)
    assert ghf.HIST_COVER_ALL == 1
    assert L.ghf_status_string(10) not in (None, b"unknown status")
    assert 10 in ghf.STATUS


@pytest.mark.parametrize("n", [1, 4096, 1 << 20])
def test_shared_bound_is_four_bytes_per_symbol_and_the_end_mark(ghf, n):
    assert ghf.compress_batch_shared_bound(n) == (4 * n + 4 + 15) & ~15


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


def test_shared_batch_kernels_use_no_scratch_and_keep_their_lds_budget():
    """Without the code build a compress workgroup is short-lived, so what hides one item's latency is its neighbours on
    the CU: at most 20 KiB of LDS lets eight workgroups share a CU's 160 KiB (the decode kernel: 40 KiB, four), and none
    of the three kernels may spill."""
    text = _kernel_asm("ghf_batch_shared")
    for sym, lds in (("_ZN3ghf23k_compress_batch_sharedENS_25BatchSharedCompressParamsE", 20 * 1024),
                     ("_ZN3ghf21k_decode_batch_sharedENS_23BatchSharedDecodeParamsE", 40 * 1024),
                     ("_ZN3ghf17k_histogram_batchENS_15BatchHistParamsE", 4 * 1024)):
        meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
        assert meta, sym
        head = text[: meta.start()]
        head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
        blk = head + meta.group(1)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= lds, sym
        body = text[text.index(sym + ":") :]
        body = body[: body.index(".Lfunc_end")]
        assert "scratch_" not in body, sym
