"""CPU (-m "not gpu"): the container calls (include/ghf_tensor.h) are exported, declared with the
comment of their neighbours and bound by a module of their own that leaves ghf.py's recorded surface alone;
ghf_tensor_bound covers every model container; ghf_tensor_parse accepts every model container and returns its fields, and
refuses one damaged head per rule; a null context is refused without a device.  The model is tests/tensor_model.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import pkgload
import tensor_model as tm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
E_INVAL, E_FORMAT = 1, 6
ARGC = {"ghf_tensor_bound": 2, "ghf_tensor_pack": 14, "ghf_compress_tensor": 10, "ghf_tensor_workspace_release": 1,
        "ghf_tensor_parse": 4, "ghf_tensor_open": 6, "ghf_tensor_close": 1, "ghf_tensor_describe": 2, "ghf_tensor_decode": 6, "ghf_tensor_decode_range": 7, "ghf_tensor_gather": 10}
RAW_SIZES = range(1, 49)


@pytest.fixture(scope="module")
def pkg():
    p = pkgload.load()
    if not os.path.exists(p.ghf.LIB_PATH):
        p.build()
    return p


@pytest.fixture(scope="module")
def gt(pkg):
    import importlib

    return importlib.import_module("golden_huffman_amd.ghf_tensor")


def models():
    return [tm.case(k)[2] for k in tm.CASES] + [tm.all_raw(n)[1] for n in RAW_SIZES]


def test_the_model_answers_the_pinned_masks_and_value_counts():
    for key, (e, n, rel, raw, sparse, want_raw, want_sparse) in tm.CASES.items():
        c = tm.case(key)[2]
        assert (c.raw, c.sparse) == (want_raw, want_sparse), key
        assert c.n == n and c.e == e and c.total == c.bytes.size
    for key, want in tm.N_VALS.items():
        assert tm.case(key)[2].stored.n_vals == want, key
    d4 = tm.case("d4")[2]  # raw + dense + sparse + a sparse plane with an empty values slot; 3 rank blocks, 18 seek blocks
    assert d4.stored.kind[0] == "raw" and d4.stored.kind[1] == "image" and d4.stored.kind[7] is None and d4.n_vals == [0, 0, 93, 0]
    assert (d4.ranks[2].size - 64) // 8 - 1 == 3 and (d4.tables[1].size - 64) // 24 == 18
    d8 = tm.case("d8")[2]
    assert d8.stored.n_vals[6:] == [0, 0] and d8.stored.kind[8 + 6] is None and d8.stored.kind[8 + 7] is None


def test_exports_and_declarations(pkg, gt):
    ghf, L = pkg.ghf, gt.lib()
    hdr = open(os.path.join(ROOT, "include", "ghf_tensor.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(ghf_[a-z0-9_]+)\s*\(", code))) == sorted(ARGC) == sorted(gt.EXPORTS)
    for name, argc in ARGC.items():
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == argc, name
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, code, flags=re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == argc, name
        comment = hdr[: hdr.index(" %s(" % name)].rstrip()
        comment = comment[: comment.rindex("*/") + 2]
        assert comment[comment.rindex("/*") :].startswith("/* No reference counterpart"), name
        assert name not in ghf.EXPORTS, name  # the recorded binding is not touched
    assert hdr.count("No reference counterpart") == len(ARGC)
    assert len(ghf.EXPORTS) == 133
    main = open(os.path.join(ROOT, "include", "ghf.h")).read()
    tail = main[main.rindex("/* ----") :]
    assert "DESIGN.md section 27" in tail and '#include "ghf_tensor.h"' in tail and tail.rstrip().endswith("#endif /* GHF_H_ */")
    assert re.search(r"^#define GHF_TENSOR_HEAD_BYTES 768$", hdr, flags=re.M) and gt.HEAD_BYTES == tm.HEAD_BYTES == 768
    assert re.search(r"^#define GHF_TENSOR_DELTA 1u", hdr, flags=re.M) and gt.DELTA == tm.DELTA == 1
    assert C.sizeof(gt.TensorInfo) == 8 + 8 + 16 + 8 + 64 + 16 * 40 and gt.DIR_ENTRIES == tm.DIR_ENTRIES == 40
    for m in ("compress_tensor", "pack", "parse", "open", "bound", "release_workspace", "Tensor"):
        assert hasattr(gt, m), m
    for m in ("decode", "decode_range", "gather", "close"):
        assert hasattr(gt.Tensor, m), m


def test_the_units_are_built_into_the_library():
    mk = open(os.path.join(ROOT, "golden-huffman_amd", "Makefile")).read()
    names = re.search(r"^NAMES := (.*)$", mk, flags=re.M).group(1).split()
    assert "ghf_tensor" in names and "ghf_api_tensor" in names


def test_bound_covers_every_model_container(gt):
    for c in models():
        assert gt.bound(c.n, c.e) >= c.total, (c.e, c.n)
        assert gt.bound(c.n, c.e) % 16 == 0
    assert gt.bound(100, 3) == 0


def test_parse_accepts_every_model_container(gt):
    for c in models():
        info = gt.parse(c.head, c.total)
        assert (info.version, info.elem_bytes, info.n_elems, info.raw_planes, info.sparse_planes, info.flags, info.reserved,
                info.total_bytes) == (1, c.e, c.n, c.raw, c.sparse, c.flags, 0, c.total)
        assert list(info.n_vals) == c.n_vals + [0] * (8 - c.e)
        assert info.sections() == c.dir
        gt.parse(c.bytes, c.total + 4096)  # a container may stand in a larger buffer


def _poke(head, at, fmt, value):
    bad = head.copy()
    bad[at : at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
    return bad


def _entry(k, field):
    return 128 + 16 * k + 8 * field


def damaged_heads():
    """(what, head, container_bytes): one damaged head per parse rule, from the delta fp32 container (raw plane 0, dense
    plane 1, sparse planes 2 and 3, plane 3 without values)"""
    c = tm.case("d4")[2]
    h, total, n, e = c.head, c.total, c.n, c.e
    off = lambda k: c.dir[k][0]  # noqa: E731
    size = lambda k: c.dir[k][1]  # noqa: E731
    yield "magic", _poke(h, 7, "<B", ord("2")), total
    yield "version", _poke(h, 8, "<I", 2), total
    yield "elem_bytes", _poke(h, 12, "<I", 3), total
    yield "raw bit at elem_bytes", _poke(h, 24, "<I", c.raw | 1 << e), total
    yield "sparse bit above elem_bytes", _poke(h, 28, "<I", c.sparse | 1 << 9), total
    yield "a plane in both masks", _poke(h, 24, "<I", c.raw | 0b0100), total
    yield "unknown flags", _poke(h, 32, "<I", c.flags | 2), total
    yield "reserved word", _poke(h, 36, "<I", 1), total
    yield "reserved bytes", _poke(h, 63, "<B", 1), total
    yield "offset not a multiple of 16", _poke(h, _entry(tm.STREAMS + 0, 0), "<Q", off(tm.STREAMS + 0) + 8), total
    swapped = _poke(_poke(h, _entry(tm.TABLES + 1, 0), "<Q", off(tm.TABLES + 2)), _entry(tm.TABLES + 2, 0), "<Q", off(tm.TABLES + 1))
    yield "sections out of order", swapped, total
    yield "sections overlap", _poke(h, _entry(tm.TABLES + 2, 0), "<Q", off(tm.TABLES + 1)), total
    yield "streams in front of the tables", _poke(h, _entry(tm.STREAMS + 0, 0), "<Q", 768), total
    yield "a section beyond the container", h, total - 16
    yield "total_bytes beyond the container", _poke(h, 40, "<Q", total + 16), total
    yield "total_bytes is not the end", _poke(h, 40, "<Q", total - 16), total
    yield "a dense plane without its table", _poke(_poke(h, _entry(tm.TABLES + 1, 0), "<Q", 0), _entry(tm.TABLES + 1, 1), "<Q", 0), total
    yield "a sparse plane without its rank table", _poke(_poke(h, _entry(tm.RANKS + 2, 0), "<Q", 0), _entry(tm.RANKS + 2, 1), "<Q", 0), total
    yield "a stream missing", _poke(_poke(h, _entry(tm.STREAMS + 1, 0), "<Q", 0), _entry(tm.STREAMS + 1, 1), "<Q", 0), total
    yield "a values stream without values", _poke(_poke(h, _entry(tm.STREAMS + 7, 0), "<Q", total), _entry(tm.STREAMS + 7, 1), "<Q", 16), total + 16
    yield "a table of a raw plane", _poke(_poke(h, _entry(tm.TABLES + 0, 0), "<Q", 0), _entry(tm.TABLES + 0, 1), "<Q", 88), total
    yield "a rank table of a dense plane", _poke(h, _entry(tm.RANKS + 1, 1), "<Q", 96), total
    yield "a raw stream of another size", _poke(h, _entry(tm.STREAMS + 0, 1), "<Q", n + 1), total
    yield "a seek table of another size", _poke(h, _entry(tm.TABLES + 1, 1), "<Q", size(tm.TABLES + 1) - 24), total
    yield "a values table of another size", _poke(h, _entry(tm.TABLES + 6, 1), "<Q", size(tm.TABLES + 6) + 24), total
    yield "a rank table of another size", _poke(h, _entry(tm.RANKS + 3, 1), "<Q", size(tm.RANKS + 3) - 8), total
    yield "n_vals above n_elems", _poke(h, 64 + 8 * 2, "<Q", n + 1), total
    yield "n_vals of a plane that is not sparse", _poke(h, 64 + 8 * 1, "<Q", 5), total
    yield "n_elems of zero", _poke(h, 16, "<Q", 0), total
    yield "a head cut short", h[:767], total


def test_parse_refuses_one_damaged_head_per_rule(pkg, gt):
    L = gt.lib()
    seen = 0
    for what, head, container_bytes in damaged_heads():
        buf = (C.c_uint8 * head.size).from_buffer_copy(head.tobytes())
        info = gt.TensorInfo()
        info.version = 77
        assert L.ghf_tensor_parse(buf, head.size, container_bytes, C.byref(info)) == E_FORMAT, what
        assert info.version == 0, what  # zeroed on failure
        with pytest.raises(pkg.ghf.GhfError) as err:
            gt.parse(head, container_bytes)
        assert err.value.status == E_FORMAT, what
        seen += 1
    assert seen == 30
    info = gt.TensorInfo()
    assert L.ghf_tensor_parse(None, 768, 4096, C.byref(info)) == E_INVAL
    good = tm.case("d4")[2].head
    assert L.ghf_tensor_parse((C.c_uint8 * 768).from_buffer_copy(good.tobytes()), 768, 4096, None) == E_INVAL


def test_a_null_context_is_refused_without_a_device(pkg, gt):
    """the call-level checks come before anything touches HIP; the other refusals run on a live context in
    tests/test_gpu_tensor.py"""
    ghf, L = pkg.ghf, gt.lib()
    idx = (ghf.Index * 16)()
    vp16, vp8, n_vals = (C.c_void_p * 16)(*[4096] * 16), (C.c_void_p * 8)(*[8192] * 8), (C.c_size_t * 8)()
    head = tm.case("p4")[2].head
    buf = (C.c_uint8 * 768).from_buffer_copy(head.tobytes())
    for e in (2, 4, 8, 0, 3):
        assert L.ghf_tensor_pack(None, vp16, 4096, idx, vp8, 0, 0, n_vals, 64, e, 0, 1 << 20, 1 << 16, 1 << 21) == E_INVAL, e
        assert L.ghf_compress_tensor(None, 4096, None, 64, e, ghf.RAW_AUTO, 0, 1 << 20, 1 << 16, 1 << 21) == E_INVAL, e
    h = C.c_void_p(1234)
    assert L.ghf_tensor_open(None, buf, 768, 1 << 20, 15728, C.byref(h)) == E_INVAL and not h.value
    assert L.ghf_tensor_decode(None, None, None, 1 << 20, 1 << 16, None) == E_INVAL
    assert L.ghf_tensor_decode_range(None, None, None, 0, 1, 1 << 20, 1 << 16) == E_INVAL
    assert L.ghf_tensor_gather(None, None, None, 4096, 1, 1, 1, 1 << 20, 16, 8192) == E_INVAL
    assert L.ghf_tensor_describe(None, C.byref(gt.TensorInfo())) == E_INVAL
    assert L.ghf_tensor_workspace_release(None) == E_INVAL
    assert L.ghf_tensor_close(None) == 0
