"""CPU (-m "not gpu"): the host-only half of the seek table (ghf_seek_bytes, ghf_seek_parse) and an ISA guard that keeps
the two new LDS-heavy kernels scratch-free, in the style of test_k6_kernels_use_no_scratch."""
import os
import re
import struct

import numpy as np
import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_FORMAT = 6


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def table_image(n, flags=0, magic=b"GHFSEEK1", version=1, block=4096, run=512, n_blocks=None, records=None):
    """header + zeroed records, built here from the format's description (DESIGN.md "Seekable .crs2")"""
    nb = -(-n // 4096) if n_blocks is None else n_blocks
    hdr = magic + struct.pack("<IIQIIQ", version, flags, n, block, run, nb)
    hdr += bytes(64 - len(hdr))
    body = bytes(24 * nb) if records is None else records
    return np.frombuffer(hdr + body, dtype=np.uint8).copy()


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 1 << 28, 1 << 32])
def test_seek_bytes(ghf, n):
    assert ghf.seek_bytes(n) == 64 + 24 * (-(-n // 4096))


@pytest.mark.parametrize("n,flags", [(0, 0), (1, 0), (4096, 1), (4097, 0), (100000, 1)])
def test_seek_parse_returns_the_header_fields(ghf, n, flags):
    img = table_image(n, flags=flags)
    assert img.size == ghf.seek_bytes(n)
    info = ghf.seek_parse(img)
    assert (info.n_symbols, info.n_blocks, info.flags, info.version) == (n, -(-n // 4096), flags, 1)


def test_seek_parse_needs_only_the_header_and_the_size(ghf):
    """the records are not looked at on the host: a 2^32-symbol table's header parses against its size alone"""
    import ctypes as C

    n = 1 << 32
    img = table_image(n, records=b"")
    info = ghf.SeekInfo()
    assert ghf.lib().ghf_seek_parse(img.ctypes.data, ghf.seek_bytes(n), C.byref(info)) == 0
    assert info.n_symbols == n and info.n_blocks == 1 << 20


@pytest.mark.parametrize("what", ["magic", "version", "block_symbols", "run_symbols", "n_blocks", "size_short", "size_long",
                                  "truncated_header", "truncated_records", "unknown_flag", "reserved"])
def test_seek_parse_rejects(ghf, what):
    n = 10000  # 3 blocks
    img = {
        "magic": lambda: table_image(n, magic=b"GHFSEEK2"),
        "version": lambda: table_image(n, version=2),
        "block_symbols": lambda: table_image(n, block=8192),
        "run_symbols": lambda: table_image(n, run=256),
        "n_blocks": lambda: table_image(n, n_blocks=4),
        "size_short": lambda: table_image(n)[:-24],
        "size_long": lambda: np.concatenate([table_image(n), np.zeros(24, np.uint8)]),
        "truncated_header": lambda: table_image(n)[:40],
        "truncated_records": lambda: table_image(n)[:64 + 30],
        "unknown_flag": lambda: table_image(n, flags=2),
        "reserved": lambda: _poke(table_image(n), 50, 1),
    }[what]()
    with pytest.raises(ghf.GhfError) as e:
        ghf.seek_parse(img)
    assert e.value.status == E_FORMAT


def _poke(a, pos, val):
    a[pos] = val
    return a


def _kernel_asm(name):
    """gfx950 ISA text of golden-huffman_amd/csrc/<name>.hip, built with the Makefile's own flags"""
    import shutil
    import subprocess
    import tempfile

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


def test_seek_kernels_use_no_scratch_and_fit_two_workgroups_per_cu():
    """k_seek_expand and k_decode_head keep K7's 68 KiB table image in LDS and a per-lane stream cursor in registers; a
    build that spills is refused here (spilled builds of such kernels have misbehaved on the GPU).  The
    expand kernel's occupancy is an LDS question: at most 80 KiB, so that two 16-wave workgroups share a CU."""
    text = _kernel_asm("ghf_seek")
    for sym in ("_ZN3ghf13k_seek_expandENS_16SeekExpandParamsE", "_ZN3ghf13k_decode_headENS_13DecHeadParamsE",
                "_ZN3ghf11k_seek_packENS_14SeekPackParamsE"):
        meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
        assert meta, sym
        head = text[: meta.start()]
        head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
        blk = head + meta.group(1)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 80 * 1024, sym
    body = text[text.index("_ZN3ghf13k_seek_expandENS_16SeekExpandParamsE:") :]
    body = body[: body.index(".Lfunc_end")]
    assert "scratch_" not in body
