"""CPU (-m "not gpu"): the host-only half of the batch calls (ghf_compress_batch_bound, ghf_batch_index_item, the
struct layout) and an ISA guard that keeps the two fused one-workgroup-per-item kernels scratch-free and small enough in
LDS for five (compress) / four (decode) workgroups per CU -- the conditions their occupancy argument rests on
(DESIGN.md section 9).  In the style of tests/test_seek_cpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
# the entry points include/ghf.h declares for batches (GHF_BATCH_MAX_ITEM is a macro, mirrored as ghf.BATCH_MAX_ITEM)
BATCH_SYMBOLS = ["ghf_compress_batch_bound", "ghf_batch_index_alloc", "ghf_batch_index_free", "ghf_batch_index_item",
                 "ghf_compress_batch", "ghf_decode_batch"]


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_batch_entry_points(ghf):
    L = ghf.lib()
    for name in BATCH_SYMBOLS:
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    assert int(re.search(r"#define GHF_BATCH_MAX_ITEM \(1u << (\d+)\)", hdr).group(1)) == 20
    assert ghf.BATCH_MAX_ITEM == 1 << 20


@pytest.mark.parametrize("n", [1, 15, 16, 4096, 65536, 100000, 1 << 20])
def test_batch_bound_is_the_single_stream_bound(ghf, n):
    assert ghf.compress_batch_bound(n) == ghf.compress_bound(n)


def test_batch_index_struct_matches_the_header(ghf):
    """u32 count, u32 reserved, three u64, two pointers: 48 bytes, pointers at 32 and 40 (what include/ghf.h declares)"""
    B = ghf.BatchIndex
    assert C.sizeof(B) == 48
    assert (B.count.offset, B.reserved.offset, B.max_item_bytes.offset, B.blocks_per_item.offset, B.segs_per_item.offset,
            B.d_chunk_bit.offset, B.d_seg_bit.offset) == (0, 4, 8, 16, 24, 32, 40)
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    body = re.search(r"typedef struct ghf_batch_index \{(.*?)\} ghf_batch_index;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t count, reserved", "uint64_t max_item_bytes", "uint64_t blocks_per_item", "uint64_t segs_per_item",
                      "uint64_t* d_chunk_bit", "uint32_t* d_seg_bit"]


def _fake_batch_index(ghf, count, max_item):
    """a BatchIndex with made-up device addresses: ghf_batch_index_item is host-only pointer arithmetic"""
    b = ghf.BatchIndex()
    b.count = count
    b.max_item_bytes = max_item
    b.blocks_per_item = -(-max_item // 4096)
    b.segs_per_item = -(-max_item // 64)
    b.d_chunk_bit = 0x10000000
    b.d_seg_bit = 0x20000000
    return b


@pytest.mark.parametrize("max_item", [1, 64, 4096, 4097, 70000, 1 << 20])
def test_batch_index_item_geometry(ghf, max_item):
    count = 5
    b = _fake_batch_index(ghf, count, max_item)
    for i in range(count):
        for n_i in sorted({1, min(63, max_item), min(64, max_item), min(65, max_item), min(4096, max_item), max_item}):
            v = ghf.batch_index_item(b, i, n_i)
            assert v.n_symbols == n_i
            assert (v.chunk_symbols, v.seg_symbols) == (4096, 64)
            assert v.n_chunks == -(-n_i // 4096)
            assert v.n_segs == -(-n_i // 64)
            assert v.flags == 0
            assert v.d_chunk_bit == 0x10000000 + 8 * i * b.blocks_per_item
            assert v.d_seg_bit == 0x20000000 + 4 * i * b.segs_per_item


def test_batch_index_item_rejects_bad_arguments(ghf):
    b = _fake_batch_index(ghf, 3, 5000)
    view = ghf.Index()
    L = ghf.lib()
    assert L.ghf_batch_index_item(C.byref(b), 3, 1, C.byref(view)) == E_INVAL       # i >= count
    assert L.ghf_batch_index_item(C.byref(b), 0, 5001, C.byref(view)) == E_INVAL    # n_i > max_item_bytes
    assert L.ghf_batch_index_item(None, 0, 1, C.byref(view)) == E_INVAL
    assert L.ghf_batch_index_item(C.byref(b), 0, 1, None) == E_INVAL
    assert L.ghf_batch_index_item(C.byref(b), 2, 5000, C.byref(view)) == 0


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


def test_batch_kernels_use_no_scratch_and_keep_their_lds_budget():
    """One workgroup per item only pays when many workgroups share a CU (the one-wavefront code build of one item is hidden
    by the others): the compress kernel keeps at most 32 KiB of LDS (five workgroups in a CU's 160 KiB), the decode kernel
    at most 40 KiB, and neither may spill."""
    text = _kernel_asm("ghf_batch")
    for sym, lds in (("_ZN3ghf16k_compress_batchENS_19BatchCompressParamsE", 32 * 1024),
                     ("_ZN3ghf14k_decode_batchENS_17BatchDecodeParamsE", 40 * 1024)):
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
