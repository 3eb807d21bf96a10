"""CPU (-m "not gpu"): byte planes in three forms (ghf_planes_split_to, ghf_planes_merge_from, ghf_planes_merge_range_from,
ghf_compress_planes_forms, ghf_decode_planes_forms, ghf_decode_planes_forms_range) are exported, bound and
declared in a section of their own, a null context is refused without a device, the choice rule restated in numpy plus the
oracle gives the raw masks and stored sizes the design states, and a resource guard keeps the eighteen pointer kernels free
of spills and scratch, at their parents' LDS and within the kernel-argument segment.  In the style of tests/test_sparse_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import forms_model as model
import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
ARGC = {"ghf_planes_split_to": 6, "ghf_planes_merge_from": 6, "ghf_planes_merge_range_from": 6, "ghf_compress_planes_forms": 17,
        "ghf_decode_planes_forms": 14, "ghf_decode_planes_forms_range": 19}
METHODS = ("planes_split_to", "planes_merge_from", "planes_merge_range_from", "compress_planes_forms", "decode_planes_forms",
           "decode_planes_forms_range")
WIDTHS = (2, 4, 8)
# the parents' static LDS (tests/test_planes_cpu.py): tile / 16 rows of (E + 1) vectors
LDS = {2: 6144, 4: 5120, 8: 9216}
KERNELS = [("_ZN3ghf17k_planes_split_toILi%dELb%dEEEvPKhS2_mNS_9PlaneDstsIXT_EEE" % (e, d), e) for e in WIDTHS for d in (0, 1)] + \
          [("_ZN3ghf19k_planes_merge_fromILi%dELb%dEEEvNS_9PlaneSrcsIXT_EEEPKhmPhPKi" % (e, d), e) for e in WIDTHS for d in (0, 1)] + \
          [("_ZN3ghf25k_planes_merge_range_fromILi%dELb%dEEEvNS_9PlaneSrcsIXT_EEEjPKhmPhPKi" % (e, d), e) for e in WIDTHS for d in (0, 1)]


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


def test_library_exports_the_forms_entry_points(ghf):
    L = ghf.lib()
    hdr = header()
    for name, argc in ARGC.items():
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert len(getattr(L, name).argtypes) == argc, name
        args = declaration(hdr, name)
        assert len(args.split(",")) == argc, name
        assert "d_base" in args, name  # the whole family takes the optional base
    for m in METHODS:
        assert hasattr(ghf.Context, m), m
    assert ghf.RAW_AUTO == 0x80000000 and re.search(r"^#define GHF_RAW_AUTO 0x80000000u$", hdr, flags=re.M)


def test_the_section_stands_between_the_sharded_decode_and_the_crs_part(ghf):
    """behind ghf_sync_piece, the declaration that follows "Multi-GPU decode of a stream", and in front of everything the
    header says about .crs; the comment directly in front of every declaration says that the reference has nothing like it
    and names the lines it generalises"""
    hdr = header()
    sec = hdr.index("/* ---- byte planes in three forms (DESIGN.md section 23)")
    sync_piece = hdr.index("int ghf_sync_piece(")
    assert hdr.index("/* Multi-GPU decode of a stream") < sync_piece < sec < hdr.index("int ghf_crs_build_code(")
    assert hdr[hdr.index(");", sync_piece) + 2 : sec].strip() == ""  # directly behind that declaration
    block = hdr[sec : hdr.index("/* ----", sec + 10)]
    for name in ARGC:
        assert hdr.count(name + "(") == block.count(name + "(") == 1, name  # declared here, and spoken of as a call nowhere else
        at = block.index("int %s(" % name)
        comment = block[:at].rstrip()
        assert comment.endswith("*/"), name
        comment = comment[comment.rindex("/*") :]
        assert comment.startswith("/* No reference counterpart"), name
        assert re.search(r"include/compressor\.h:\d+-\d+", comment), name
    assert block.count("No reference counterpart") == len(ARGC)
    flat = re.sub(r"\s*\n \*\s*", " ", block)  # the comments as running text
    intro = flat[: flat.index("#define GHF_RAW_AUTO")]
    assert "no container, no magic, no header" in intro and "d_out_bytes[p] = n_elems" in intro
    assert "d_base IS OPTIONAL" in intro and "GHF_E_INVAL" in intro
    assert "AT MOST ONCE" in flat and "NEVER synchronises" in flat and "EXACTLY when" in flat


def test_a_null_context_is_refused_without_a_device(ghf):
    """The call-level checks come before anything touches HIP.  With no device there is no context, so the null context is
    what answers here for every width and every mask, good or bad, with and without a base; the other refusals are exercised
    on a live context in tests/test_gpu_planes_forms.py."""
    L = ghf.lib()
    C = ghf.C
    idx = (ghf.Index * 16)()
    vp8 = (C.c_void_p * 8)(*[4096 + 256 * p for p in range(8)])
    vp16, sz16 = (C.c_void_p * 16)(*[4096] * 16), (C.c_size_t * 16)(*[64] * 16)
    infos = (ghf.SeekInfo * 16)()
    r_infos, r_ptrs = (ghf.SparseRankInfo * 8)(), (C.c_void_p * 8)()
    n_vals = (C.c_size_t * 8)(*[3] * 8)
    raw, chosen = C.c_uint(0), C.c_uint(0)
    slot = ghf.planes_slot_bytes(64)
    d_in, d_out, d_codes, d_bytes, d_ranks = 4096, 1 << 20, 1 << 21, 1 << 22, 1 << 23
    masks = (0, 1, 2, 3, 0xFF, 1 << 8, ghf.RAW_AUTO, ghf.RAW_AUTO | 1)
    for e in (2, 4, 8, 0, 1, 3, 16):
        for d_base in (None, 8192, 8193):
            assert L.ghf_planes_split_to(None, d_in, d_base, 64, e, vp8) == E_INVAL, e
            assert L.ghf_planes_merge_from(None, vp8, d_base, 64, e, d_out) == E_INVAL, e
            assert L.ghf_planes_merge_range_from(None, vp8, d_base, 64, e, d_out) == E_INVAL, e
            for rm in masks:
                for sm in (0, 1, ghf.SPARSE_AUTO, ghf.SPARSE_AUTO | 2):
                    for ix in (None, idx):
                        assert L.ghf_compress_planes_forms(None, d_in, d_base, 64, e, rm, sm, d_out, slot, d_bytes, d_codes, ix, d_ranks, 128,
                                                           C.byref(raw), C.byref(chosen), n_vals) == E_INVAL, (e, rm, sm)
                        assert L.ghf_decode_planes_forms(None, vp16, sz16, d_codes, ix, d_base, rm, sm, n_vals, 64, e, d_out, 64 * 8,
                                                         d_bytes) == E_INVAL, (e, rm, sm)
                    assert L.ghf_decode_planes_forms_range(None, vp16, sz16, d_codes, idx, None, None, None, r_infos, r_ptrs, d_base, rm, sm,
                                                           64, e, 3, 9, d_out, 64 * 8) == E_INVAL, (e, rm, sm)
                    assert L.ghf_decode_planes_forms_range(None, vp16, sz16, d_codes, None, infos, vp16, sz16, r_infos, r_ptrs, d_base, rm,
                                                           sm, 64, e, 3, 9, d_out, 64 * 8) == E_INVAL, (e, rm, sm)
    assert L.ghf_planes_split_to(None, None, None, 0, 2, None) == E_INVAL
    assert L.ghf_planes_merge_from(None, None, None, 0, 2, None) == E_INVAL
    assert L.ghf_planes_merge_range_from(None, None, None, 0, 2, None) == E_INVAL
    assert L.ghf_compress_planes_forms(None, None, None, 0, 2, 0, 0, None, 0, None, None, None, None, 0, None, None, None) == E_INVAL
    assert L.ghf_decode_planes_forms(None, None, None, None, None, None, 0, 0, None, 0, 2, None, 0, None) == E_INVAL
    assert L.ghf_decode_planes_forms_range(None, None, None, None, None, None, None, None, None, None, None, 0, 0, 0, 2, 0, 0, None,
                                           0) == E_INVAL


# the choice rule on default_rng(7).standard_normal(n) as bf16 / fp32 / fp64: the raw masks and the stored totals
RAW_MASKS = {65536: {2: 0b01, 4: 0b0111, 8: 0b00111111}, 4097: {2: 0b01, 4: 0b0111, 8: 0b01111111},
             64: {2: 0b11, 4: 0b1111, 8: 0xFF}, 1: {2: 0b11, 4: 0b1111, 8: 0xFF}}
TOTALS = {65536: {2: 88620, 4: 219692, 8: 461747}, 4097: {2: 6608, 4: 14802, 8: 30561}}


@pytest.mark.parametrize("n", list(RAW_MASKS))
@pytest.mark.parametrize("e", WIDTHS)
def test_the_restated_rule_gives_the_pinned_masks_and_sizes(e, n):
    """GHF_RAW_AUTO with nothing sparse, and both masks automatic: a standard-normal tensor has no plane with 3/4 zeros, so
    both requests store the same"""
    x = model.normal_elems(n, e)
    for sparse in (0, model.AUTO):
        s = model.Stored(x, e, raw=model.AUTO, sparse=sparse, tables=False)
        assert s.raw == RAW_MASKS[n][e] and s.sparse == 0, (sparse, bin(s.raw))
        for p in range(e):  # raw exactly when the image would be no smaller than the plane; nothing stores more than n bytes
            assert ((s.raw >> p) & 1) == (model.image(s.planes[p]).size >= n), p
            assert s.sizes[p] <= n and s.sizes[e + p] == 0, p
        if n in TOTALS:
            assert s.total == TOTALS[n][e]
        else:
            assert s.total == n * e  # all raw: the tensor's own size
        assert s.total <= n * e


def test_the_two_header_rule():
    """an all-zero tensor: up to 2 * ghf_header_bytes(1) elements both automatic masks store no plane sparse -- raw while the
    dense image (a header and a bit per byte) would be no smaller than the plane, dense from there on --, above that size
    sparse; with an explicit raw mask GHF_SPARSE_AUTO is the rule of DESIGN.md section 20 at every size"""
    import numpy as np

    assert model.TWO_HEADERS == 2096
    for n, want in ((64, (0b11, 0)), (1024, (0b11, 0)), (2096, (0, 0)), (2097, (0, 0b11)), (65536, (0, 0b11))):
        z = np.zeros(2 * n, dtype=np.uint8)
        s = model.Stored(z, 2, raw=model.AUTO, sparse=model.AUTO, tables=False)
        assert (s.raw, s.sparse) == want, n
        assert model.Stored(z, 2, raw=0, sparse=model.AUTO, tables=False).sparse == 0b11, n
        assert model.Stored(z, 2, raw=0b01, sparse=model.AUTO, tables=False).sparse == 0b10, n


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
            for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
                      "kernarg_segment_size", "vgpr_count")}


def test_design_states_the_lds_of_the_pointer_kernels():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 23.") :]
    for e in WIDTHS:
        assert re.search(r"\| %d \|[^\n]*\| %d \|" % (e, LDS[e]), sec), e


@pytest.mark.parametrize("sym,e", KERNELS)
def test_pointer_kernels_have_no_spills_no_scratch_and_the_parents_lds(ghf, sym, e):
    """from the kernel metadata alone: nothing spilled, no private segment, the static LDS of the parent kernels, and the E
    plane addresses inside a kernel-argument segment of at most 4096 bytes; at most 128 registers: a resident round of sixteen
    one-wave workgroups per CU, as the parents have it"""
    text = _kernel_asm("ghf_planes")
    res = _resources(text, sym)
    assert res["vgpr_spill_count"] == 0 and res["sgpr_spill_count"] == 0, (sym, res)
    assert res["private_segment_fixed_size"] == 0, (sym, res)
    assert res["group_segment_fixed_size"] == LDS[e] == ghf.PLANES_TILE[e] // 16 * (e + 1) * 16, (sym, res)
    assert 8 * e < res["kernarg_segment_size"] <= 4096, (sym, res)
    assert res["vgpr_count"] <= 128, (sym, res)
    body = text[text.index(sym + ":") :]
    assert "scratch_" not in body[: body.index(".Lfunc_end")], sym
