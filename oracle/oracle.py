"""oracle/oracle.py -- TEST INFRASTRUCTURE ONLY.

ctypes binding of oracle/_build/liboracle.so (the plain-C CPU restatement of the reference's
canonical-Huffman path, oracle/huff_oracle.c) plus a thin runner for oracle/_ref/ref_glzip (the
reference's own headers compiled in the build container, when present).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module --
as the checker, never as the product.  The product (golden-huffman_amd) never imports it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "liboracle.so")
REF_BIN = os.path.join(HERE, "_ref", "ref_glzip")
NSYM = 257


class OrcCode(C.Structure):
    """mirror of orc_code (include/canonical_huff_encoder.h:107-120 of the reference)."""

    _fields_ = [
        ("length", C.c_uint32 * NSYM),
        ("codeword", C.c_uint32 * NSYM),
        ("symbol", C.c_uint32 * NSYM),
        ("first_code", C.c_uint32 * 64),
        ("start_pos", C.c_uint32 * 64),
        ("min_len", C.c_int32),
        ("max_len", C.c_int32),
    ]

    def as_dict(self):
        ml = self.max_len
        return {
            "length": list(self.length),
            "codeword": list(self.codeword),
            "symbol": list(self.symbol),
            "first_code": list(self.first_code)[1 : ml + 1],
            "start_pos": list(self.start_pos)[1 : ml + 1],
            "min_len": self.min_len,
            "max_len": ml,
        }


class OrcTree(C.Structure):
    """mirror of orc_tree: the reference's HuffTree (include/huff_tree.h:41-98), leaves = node ids 0..255."""

    _fields_ = [("left", C.c_int * 512), ("right", C.c_int * 512), ("root", C.c_int), ("n_leaves", C.c_int), ("n_nodes", C.c_int)]


class OrcCrsCode(C.Structure):
    _fields_ = [("len", C.c_uint16 * 256), ("bits", (C.c_uint8 * 256) * 256)]


def build():
    """(re)build liboracle.so -- and the reference driver when /root/reference is present."""
    subprocess.run(["make", "-s", "-C", HERE, "all"], check=True)
    if os.path.isdir("/root/reference/include"):
        subprocess.run(["make", "-s", "-C", HERE, "ref"], check=True)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        u8p = C.c_void_p
        L.orc_histogram.argtypes = [u8p, C.c_size_t, C.POINTER(C.c_int64)]
        L.orc_histogram.restype = None
        L.orc_build_code.argtypes = [C.POINTER(C.c_int64), C.POINTER(OrcCode)]
        L.orc_build_code.restype = C.c_int
        L.orc_header_size.argtypes = [C.POINTER(OrcCode)]
        L.orc_header_size.restype = C.c_size_t
        L.orc_write_header.argtypes = [C.POINTER(OrcCode), u8p]
        L.orc_write_header.restype = C.c_size_t
        L.orc_encode_body.argtypes = [u8p, C.c_size_t, C.POINTER(OrcCode), u8p, C.c_size_t]
        L.orc_encode_body.restype = C.c_size_t
        L.orc_compress.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.orc_compress.restype = C.c_int
        L.orc_compress_bound.argtypes = [C.c_size_t]
        L.orc_compress_bound.restype = C.c_size_t
        L.orc_parse_header.argtypes = [u8p, C.c_size_t, C.POINTER(OrcCode)]
        L.orc_parse_header.restype = C.c_size_t
        L.orc_decode_body.argtypes = [u8p, C.c_size_t, C.POINTER(OrcCode), u8p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.orc_decode_body.restype = C.c_int
        L.orc_decompress.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.orc_decompress.restype = C.c_int
        L.orc_pack_at.argtypes = [u8p, C.c_size_t, C.POINTER(OrcCode), C.c_uint, C.c_int, u8p, C.c_size_t]
        L.orc_pack_at.restype = C.c_uint64
        L.orc_body_bits.argtypes = [C.POINTER(C.c_int64), C.POINTER(OrcCode)]
        L.orc_body_bits.restype = C.c_uint64
        L.orc_build_code_limited.argtypes = [C.POINTER(C.c_int64), C.POINTER(OrcCode), C.c_int]
        L.orc_build_code_limited.restype = C.c_int
        L.orc_compress_limited.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, C.POINTER(C.c_size_t), C.c_int]
        L.orc_compress_limited.restype = C.c_int
        L.orc_crs_build_tree.argtypes = [C.POINTER(C.c_int64), C.POINTER(OrcTree)]
        L.orc_crs_build_tree.restype = C.c_int
        L.orc_crs_codes.argtypes = [C.POINTER(OrcTree), C.POINTER(OrcCrsCode)]
        L.orc_crs_codes.restype = None
        L.orc_crs_write_tree.argtypes = [C.POINTER(OrcTree), u8p]
        L.orc_crs_write_tree.restype = C.c_size_t
        L.orc_crs_parse_tree.argtypes = [u8p, C.c_size_t, C.POINTER(OrcTree)]
        L.orc_crs_parse_tree.restype = C.c_size_t
        L.orc_crs_bound.argtypes = [C.c_size_t]
        L.orc_crs_bound.restype = C.c_size_t
        L.orc_crs_compress.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.orc_crs_compress.restype = C.c_int
        L.orc_crs_decompress.argtypes = [u8p, C.c_size_t, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.orc_crs_decompress.restype = C.c_int
        L.orc_crs_walk.argtypes = [C.POINTER(OrcTree), u8p, C.c_uint64, C.c_uint64, C.c_uint64, u8p, C.c_size_t, C.POINTER(C.c_uint64)]
        L.orc_crs_walk.restype = C.c_long
        _lib = L
    return _lib


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data


def histogram(data):
    a, p = _u8(data)
    h = np.zeros(NSYM, dtype=np.int64)
    lib().orc_histogram(p, a.size, h.ctypes.data_as(C.POINTER(C.c_int64)))
    return h


def build_code(hist):
    h = np.ascontiguousarray(hist, dtype=np.int64)
    c = OrcCode()
    rc = lib().orc_build_code(h.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(c))
    if rc:
        raise ValueError("orc_build_code rc=%d" % rc)
    return c


def header_bytes(code):
    n = lib().orc_header_size(C.byref(code))
    out = np.zeros(n, dtype=np.uint8)
    w = lib().orc_write_header(C.byref(code), out.ctypes.data)
    assert w == n
    return out


def body_bits(hist, code):
    h = np.ascontiguousarray(hist, dtype=np.int64)
    return int(lib().orc_body_bits(h.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(code)))


def compress(data):
    a, p = _u8(data)
    cap = lib().orc_compress_bound(a.size)
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().orc_compress(p, a.size, out.ctypes.data, cap, C.byref(n))
    if rc:
        raise ValueError("orc_compress rc=%d" % rc)
    return out[: n.value].copy()


def decompress(crs2, cap=None):
    a, p = _u8(crs2)
    if cap is None:
        cap = a.size * 8 + 64  # min code length is 1 bit
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().orc_decompress(p, a.size, out.ctypes.data, cap, C.byref(n))
    if rc:
        raise ValueError("orc_decompress rc=%d" % rc)
    return out[: n.value].copy()


def parse_header(crs2):
    a, p = _u8(crs2)
    c = OrcCode()
    hs = lib().orc_parse_header(p, a.size, C.byref(c))
    if not hs:
        raise ValueError("bad .crs2 header")
    return c, hs


# ------------------------------------------------------------------ opt-in length limit
def build_code_limited(hist, limit=32):
    h = np.ascontiguousarray(hist, dtype=np.int64)
    c = OrcCode()
    rc = lib().orc_build_code_limited(h.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(c), limit)
    if rc:
        raise ValueError("orc_build_code_limited rc=%d" % rc)
    return c


def compress_limited(data, limit=32):
    a, p = _u8(data)
    cap = lib().orc_compress_bound(a.size) + a.size * 3  # limited codes may be longer than 9 bits on average
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().orc_compress_limited(p, a.size, out.ctypes.data, cap, C.byref(n), limit)
    if rc:
        raise ValueError("orc_compress_limited rc=%d" % rc)
    return out[: n.value].copy()


def compress_empty():
    """SURVEY 8(f) N4, second half: the opt-in definition of the EMPTY input (GHF_EMPTY_OK, include/ghf.h).  PARITY
    UNPINNED -- the reference is undefined at n == 0 (include/canonical_huff_encoder.cc:309-343: no merge happens, every
    length stays 0), so this restates the builder's own definition, not the reference: the end mark alone with the
    one-bit code "0", its header as write_encode_info (canonical_huff_encoder.cc:210-242) would lay it out, then the
    byte 0x7F = the end mark followed by the 1-bits flush_bits pads with (utils/include/buffer.h:290-295)."""
    c = OrcCode()
    for i in range(NSYM):
        c.symbol[i] = 0xFFFFFFFF
    c.symbol[0] = NSYM - 1
    c.length[NSYM - 1] = 1
    c.min_len = c.max_len = 1
    c.first_code[1] = 0
    c.start_pos[1] = 0
    return np.concatenate([header_bytes(c), np.array([0x7F], dtype=np.uint8)])


# ------------------------------------------------------------------ .crs (NormalHuffEncoder)
def crs_tree(hist256):
    h = np.ascontiguousarray(hist256[:256], dtype=np.int64)
    t = OrcTree()
    rc = lib().orc_crs_build_tree(h.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(t))
    if rc:
        raise ValueError("orc_crs_build_tree rc=%d" % rc)
    return t


def crs_code_strings(tree):
    """the 256 code strings ('0'/'1'), '' for absent symbols -- what NormalHuffEncoder::encode_map_ holds."""
    c = OrcCrsCode()
    lib().orc_crs_codes(C.byref(tree), C.byref(c))
    return ["".join("01"[b] for b in c.bits[s][: c.len[s]]) for s in range(256)]


def crs_tree_bytes(tree):
    out = np.zeros(2 * 511, dtype=np.uint8)
    n = lib().orc_crs_write_tree(C.byref(tree), out.ctypes.data)
    return out[:n].copy()


def crs_compress(data):
    a, p = _u8(data)
    cap = lib().orc_crs_bound(a.size)
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().orc_crs_compress(p, a.size, out.ctypes.data, cap, C.byref(n))
    if rc:
        raise ValueError("orc_crs_compress rc=%d" % rc)
    return out[: n.value].copy()


def crs_decompress(crs, cap=None):
    a, p = _u8(crs)
    if cap is None:
        cap = a.size * 8 + 64
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().orc_crs_decompress(p, a.size, out.ctypes.data, cap, C.byref(n))
    if rc:
        raise ValueError("orc_crs_decompress rc=%d" % rc)
    return out[: n.value].copy()


def crs_parse_tree(header):
    """the tree of a preorder header (the restatement of DecodeHuffTree::do_build_tree) -> OrcTree"""
    a, p = _u8(header)
    t = OrcTree()
    if lib().orc_crs_parse_tree(p, a.size, C.byref(t)) != a.size:
        raise ValueError("bad .crs tree")
    return t


def crs_walk(tree, body, nbits, start, end, out):
    """the codes that start in bits [start, end) of `body` under `tree`, written to `out` -> (their number, the bit behind
    the last one); raises if a code runs past nbits"""
    nxt = C.c_uint64(0)
    n = lib().orc_crs_walk(C.byref(tree), body.ctypes.data, nbits, start, end, out.ctypes.data, out.size, C.byref(nxt))
    if n < 0:
        raise ValueError("orc_crs_walk rc=%d" % n)
    return n, nxt.value


# ------------------------------------------------------------------ the compiled reference (build container only)
def have_ref():
    return os.path.exists(REF_BIN)


def ref_run(args, timeout=120, cpu=None):
    """run oracle/_ref/ref_glzip under a timeout and an output-size limit (a runaway
    reference decoder fills the disk); cpu = pin the process to that one core (the reference is single-threaded)."""
    cmd = "ulimit -f 16777216; exec '%s' %s" % (REF_BIN, " ".join("'%s'" % a for a in args))
    pin = (lambda: os.sched_setaffinity(0, {cpu})) if cpu is not None else None
    return subprocess.run(["bash", "-c", cmd], check=True, timeout=timeout, capture_output=True, text=True, preexec_fn=pin).stdout
