"""CPU (-m "not gpu"): the host-only half of the plane batch calls with raw planes -- the rule of
ghf_batch_planes_raw_auto in numpy over the oracle's histograms and codes, with the masks and stored sizes it gives
pinned (tests/batch_forms_model.py); the entries are exported, bound and declared; the call-level refusals that come back
without a device; and an ISA guard over the new kernels of ghf_batch_planes.hip and ghf_batch_seek.hip: LDS of at most
20 KiB for the packer and 40 KiB for the decoders (the run-record decoder: its parent's 41 840 bytes), no spills, no private
segment, no scratch instruction, 16-byte global loads and slot stores on the raw path.  In the style of
tests/test_batch_planes_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import batch_forms_model as model
import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
ARGC = {"ghf_batch_planes_raw_auto": 5, "ghf_compress_batch_planes_forms": 13, "ghf_decode_batch_planes_forms": 13,
        "ghf_decode_bodies_batch_planes_forms": 11, "ghf_decode_bodies_batch_planes_forms_seek": 13}
METHODS = ["batch_planes_raw_auto", "compress_batch_planes_forms", "decode_batch_planes_forms", "decode_bodies_batch_planes_forms",
           "decode_bodies_batch_planes_forms_seek"]


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


# ------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("e", [2, 4, 8])
def test_rule_on_the_normal_batch_gives_the_pinned_mask_and_sizes(e):
    datas = model.normal_batch(e)
    hists = model.plane_hists(datas, e, cover=True)
    codes = model.build_codes(hists)
    mask = model.raw_mask(hists, codes)
    dense, forms = model.stored_bytes(datas, e, codes, 0), model.stored_bytes(datas, e, codes, mask)
    print("E %d: mask %s, %d bytes all dense, %d with raw planes" % (e, bin(mask), dense, forms))
    assert (mask, forms, dense) == model.PINNED_NORMAL[e]
    # what the rule promises with exact counts: no raw plane stores more than its bodies would
    for p in range(e):
        if mask >> p & 1:
            assert sum(d.size // e for d in datas) <= sum(model.body_bytes(d[p::e], codes[p]) for d in datas), p


@pytest.mark.parametrize("e", [2, 4, 8])
def test_rule_on_three_tiny_items(e):
    rng = np.random.default_rng(7)
    datas = [model.normal_elems(rng, 17, e) for _ in range(3)]
    plain = model.plane_hists(datas, e)
    assert model.raw_mask(plain, model.build_codes(plain)) == 0
    cover = model.plane_hists(datas, e, cover=True)
    assert model.raw_mask(cover, model.build_codes(cover)) == model.PINNED_TINY_COVER[e]


def test_rule_leaves_a_plane_with_a_code_out_of_bounds_or_without_bytes_dense():
    datas = model.normal_batch(2)
    hists = model.plane_hists(datas, 2, cover=True)
    codes = model.build_codes(hists)
    assert model.raw_mask(hists, codes) == 0b01
    codes[0].max_len = 33
    assert model.raw_mask(hists, codes) == 0
    codes = model.build_codes(hists)
    hists[0, :256] = 0
    assert model.raw_mask(hists, codes) == 0


# ------------------------------------------------------------------------------ 2. exports
def test_library_exports_the_forms_entry_points(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    for name, argc in ARGC.items():
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert len(getattr(L, name).argtypes) == argc, name
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, hdr, flags=re.M | re.S)
        assert decl, name
        assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == argc, name
        comment = hdr[: decl.start()].rstrip()
        comment = comment[comment.rindex("/*") :]
        assert comment.startswith("/* No reference counterpart"), name
        assert "include/compressor.h:62-73" in comment and "87-92" in comment, name
    assert "ghf_batch_seek_pack does not change" in hdr and "NOT SPECIFIED" in hdr  # what the header says about a raw slot's record
    for m in METHODS:
        assert hasattr(ghf.Context, m), m


# ------------------------------------------------------------------------------ 3. call-level refusals
def test_call_level_refusals_come_back_without_a_device(ghf):
    """As in tests/test_batch_planes_cpu.py this shows only that every call answers GHF_E_INVAL before anything touches
    HIP when there is no context -- whatever the mask.  Each refusal as such, a mask bit at or above elem_bytes among
    them, is exercised on a live context in tests/test_gpu_batch_forms.py::test_call_level_argument_errors."""
    L = ghf.lib()
    bidx = ghf.BatchIndex()
    A = 4096  # any non-null, 16-byte aligned value: nothing is dereferenced
    auto = lambda e=2, h=A, cd=A, out=A: L.ghf_batch_planes_raw_auto(None, h, cd, e, out)
    comp = lambda e=2, raw=0, codes=A, st=A: L.ghf_compress_batch_planes_forms(None, A, A, 4096, 4, e, codes, raw, A, A, A, None, st)
    dec = lambda e=2, raw=0, codes=A, st=A: L.ghf_decode_batch_planes_forms(None, A, A, codes, ghf.C.byref(bidx), A, 4, e, raw, A, A, A, st)
    bod = lambda e=2, raw=0, codes=A, st=A: L.ghf_decode_bodies_batch_planes_forms(None, A, A, codes, 4, e, raw, A, A, A, st)
    seek = lambda e=2, raw=0, codes=A, st=A: L.ghf_decode_bodies_batch_planes_forms_seek(None, A, A, A, A, codes, 4, e, raw, A, A, A, st)
    for e in (2, 4, 8, 3):
        assert auto(e=e) == E_INVAL
        for f in (comp, dec, bod, seek):
            for raw in (0, 1, 1 << e, 0xFFFFFFFF):
                assert f(e=e, raw=raw) == E_INVAL, (e, raw)
    assert auto(h=None) == E_INVAL and auto(cd=None) == E_INVAL and auto(cd=A + 8) == E_INVAL and auto(out=None) == E_INVAL
    for f in (comp, dec, bod, seek):
        assert f(codes=None) == E_INVAL and f(codes=A + 8) == E_INVAL and f(st=None) == E_INVAL


# ------------------------------------------------------------------------------ 4. budgets
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


LOAD16 = re.compile(r"\b(?:global|flat)_load_dwordx4\b")
STORE16 = re.compile(r"\b(?:global|flat)_store_dwordx4\b")


def _check(text, sym, lds, lds_min=1):
    meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
    assert meta, sym
    head = text[: meta.start()]
    head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
    blk = head + meta.group(1)
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
    assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, sym
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, sym
    got = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert lds_min <= got <= lds, (sym, got)
    body = text[text.index(sym + ":") :]
    body = body[: body.index(".Lfunc_end")]
    assert "scratch_" not in body, sym
    return body


def test_forms_kernels_of_the_planes_unit_keep_their_budgets():
    text = _kernel_asm("ghf_batch_planes")
    _check(text, "_ZN3ghf23k_batch_planes_raw_autoEPKyPK8ghf_codejPj", 1024)
    for e in (2, 4, 8):
        body = _check(text, "_ZN3ghf29k_compress_batch_planes_formsILi%dEEEvNS_25BatchPlanesCompressParamsEj" % e, 20 * 1024)
        # the raw path's loads of the item and its slot stores are 16-byte accesses (flat_: the slot's pointer comes out of an
        # array in memory, as in the parent)
        assert LOAD16.search(body) and STORE16.search(body), e
        body = _check(text, "_ZN3ghf27k_decode_batch_planes_formsILi%dEEEvNS_23BatchPlanesDecodeParamsEj" % e, 40 * 1024)
        assert LOAD16.search(body), e
        for w in (0, 1):
            body = _check(text, "_ZN3ghf34k_decode_bodies_batch_planes_formsILi%dELb%dEEEvNS_23BatchPlanesBodiesParamsEj" % (e, w), 40 * 1024)
            assert bool(LOAD16.search(body)) == bool(w), (e, w)  # the sizes pass reads no raw plane


def test_forms_kernels_of_the_seek_unit_keep_their_budgets():
    text = _kernel_asm("ghf_batch_seek")
    for e in (2, 4, 8):
        for w in (0, 1):
            # (at most the parent's: k_decode_bodies_batch_planes_shared_seek stages 32 KiB rounds, 41 840 bytes in all)
            body = _check(text, "_ZN3ghf39k_decode_bodies_batch_planes_forms_seekILi%dELb%dEEEvNS_21BatchSeekDecodeParamsEj" % (e, w), 41840)
            assert bool(LOAD16.search(body)) == bool(w), (e, w)
