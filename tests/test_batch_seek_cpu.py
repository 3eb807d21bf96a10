"""CPU (-m "not gpu"): the run record of stored shared-code bodies -- ghf_batch_seek_bytes,
ghf_batch_seek_bound, ghf_batch_seek_pack, ghf_decode_bodies_batch_shared_seek and
ghf_decode_bodies_batch_planes_shared_seek are exported, bound and declared; the two size functions give the format's
sizes; the call-level refusals come back without a device; and an ISA guard keeps every instantiation of the decode
kernels scratch-free and within 52 KiB of LDS (three workgroups per CU), the pack kernel scratch-free.  In the style of
tests/test_batch_bodies_cpu.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import pkgload

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL = 1
ARGS = {"ghf_batch_seek_bytes": 1, "ghf_batch_seek_bound": 1, "ghf_batch_seek_pack": 9, "ghf_decode_bodies_batch_shared_seek": 11,
        "ghf_decode_bodies_batch_planes_shared_seek": 12}
METHODS = ["batch_seek_pack", "decode_bodies_batch_shared_seek", "decode_bodies_batch_planes_shared_seek"]
PACK = "_ZN3ghf17k_batch_seek_packENS_19BatchSeekPackParamsE"
DECODE = ["_ZN3ghf33k_decode_bodies_batch_shared_seekILb%dEEEvNS_21BatchSeekDecodeParamsE" % w for w in (1, 0)] + [
    "_ZN3ghf40k_decode_bodies_batch_planes_shared_seekILi%dELb%dEEEvNS_21BatchSeekDecodeParamsE" % (e, w) for e in (2, 4, 8) for w in (1, 0)]


@pytest.fixture(scope="module")
def ghf():
    pkg = pkgload.load()
    if not os.path.exists(pkg.ghf.LIB_PATH):
        pkg.build()
    return pkg.ghf


def test_library_exports_the_five_entry_points(ghf):
    L = ghf.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf.h")).read()
    for name, nargs in ARGS.items():
        assert name in ghf.EXPORTS, name
        assert getattr(L, name) is not None, name
        assert len(getattr(L, name).argtypes) == nargs, name
        m = re.search(r"^(int|size_t) %s\((.*?)\);" % name, hdr, flags=re.M | re.S)
        assert m, name
        decl = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        assert decl.count(",") + 1 == nargs, (name, decl)
        assert m.group(1) == ("size_t" if nargs == 1 else "int"), name
    for meth in METHODS:
        assert hasattr(ghf.Context, meth), meth


def test_record_sizes(ghf):
    L = ghf.lib()
    assert [L.ghf_batch_seek_bytes(n) for n in (1, 128, 129, 512, 32768, 1 << 20)] == [16, 16, 16, 16, 520, 16392]
    assert L.ghf_batch_seek_bound(4096) == 80
    assert ghf.batch_seek_bytes(4096) == 72 and ghf.batch_seek_bytes(65536) == 1032  # 1.8 % and 1.6 % of the item
    for n in (1, 127, 128, 129, 4095, 4096, 4097, 65536 + 77, 1 << 20):
        assert L.ghf_batch_seek_bytes(n) == (8 + 2 * -(-n // 128) + 7) // 8 * 8, n
        assert L.ghf_batch_seek_bound(n) == (L.ghf_batch_seek_bytes(n) + 15) // 16 * 16, n


def test_call_level_refusals_come_back_without_a_device(ghf):
    """the call-level checks come before anything touches HIP: no context, and a count of 0 does not excuse them"""
    L = ghf.lib()
    bidx = ghf.BatchIndex()
    pack, flat, planes = L.ghf_batch_seek_pack, L.ghf_decode_bodies_batch_shared_seek, L.ghf_decode_bodies_batch_planes_shared_seek
    assert pack(None, None, None, 0, 1, None, None, None, None) == E_INVAL
    assert pack(None, bidx, 16, 1, 1, 16, 16, 16, 16) == E_INVAL  # every array named, still no context
    assert pack(None, bidx, 16, 1, 3, 16, 16, 16, 16) == E_INVAL  # elem_bytes of 3
    assert flat(None, None, None, None, None, None, 0, None, None, None, None) == E_INVAL
    assert flat(None, 16, 16, 16, 16, 16, 1, 16, 16, 16, 16) == E_INVAL
    assert planes(None, None, None, None, None, None, 0, 2, None, None, None, None) == E_INVAL
    assert planes(None, 16, 16, 16, 16, 16, 1, 2, 16, 16, 16, 16) == E_INVAL
    assert planes(None, 16, 16, 16, 16, 16, 1, 3, 16, 16, 16, 16) == E_INVAL  # elem_bytes of 3


def _kernel_asm(name):
    """gfx950 ISA text of golden-huffman_amd/csrc/<name>.hip, built with the Makefile's own flags"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "golden-huffman_amd", "csrc", name + ".hip")
    mk = open(os.path.join(ROOT, "golden-huffman_amd", "Makefile")).read()
    assert re.search(r"^NAMES := .*\b%s\b" % name, mk, flags=re.M)  # the library is built from it
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, flags=re.M).group(1)
    flags = flags.replace("$(ARCH)", "gfx950").replace("$(ROOT)", ROOT).replace("$(HERE)", os.path.join(ROOT, "golden-huffman_amd") + "/")
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        r = subprocess.run([hipcc] + flags.split() + ["--cuda-device-only", "-S", "-o", os.path.join(td, "k.s"), src],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(os.path.join(td, "k.s")).read()


def _meta(text, sym):
    meta = re.search(r"\.name:\s+%s\b(.*?)\.wavefront_size" % re.escape(sym), text, flags=re.S)
    assert meta, sym
    head = text[: meta.start()]
    head = head[head.rindex("- .agpr_count") :]  # this kernel's metadata block: the fields in front of .name
    blk = head + meta.group(1)
    body = text[text.index(sym + ":") :]
    body = body[: body.index(".Lfunc_end")]
    return (lambda field: int(re.search(r"\.%s:\s+(\d+)" % field, blk).group(1))), body


def test_kernels_use_no_scratch_and_keep_their_lds_budget():
    text = _kernel_asm("ghf_batch_seek")
    for sym in DECODE:
        field, body = _meta(text, sym)
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, sym
        assert field("private_segment_fixed_size") == 0, sym
        assert field("group_segment_fixed_size") <= 52 * 1024, sym
        assert "scratch_" not in body, sym
    field, body = _meta(text, PACK)
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("private_segment_fixed_size") == 0
    assert "scratch_" not in body
