"""A numpy model of the container GHFTENS1, written from the format alone: the bytes of the container of
one typed tensor, built from forms_model.Stored (the slots and the masks), range_worlds.expected_table (the seek tables) and
sparse_range_model.table_of (the rank tables).  Nothing here touches the library.  Shared by tests/test_tensor_cpu.py and
tests/test_gpu_tensor.py, which also pin the inputs below and the masks the choice rule gives for them."""
import functools
import struct

import numpy as np

import forms_model
import range_worlds
import sparse_range_model

HEAD_BYTES = 768
DIR_ENTRIES = 40
STREAMS, TABLES, RANKS = 0, 16, 32  # where the three groups begin in the directory
DELTA = 1
MAGIC = b"GHFTENS1"
AUTO = forms_model.AUTO


def pad16(x):
    return (x + 15) & ~15


def new_of(base, e, rel):
    """base * (1 + rel * standard_normal), computed in the element type (bf16: through fp32, upper half), as bytes"""
    n = base.size // e
    g = np.random.default_rng(11).standard_normal(n)
    if e == 8:
        return (base.view(np.float64) * (1 + rel * g)).view(np.uint8).copy()
    # the product is rounded once, into the element type (N_VALS below pins which rounding this is)
    if e == 4:
        return (base.view(np.float32) * (1 + rel * g)).astype(np.float32).view(np.uint8).copy()
    b32 = (base.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    v = (b32 * (1 + rel * g)).astype(np.float32)
    return (v.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()


# the inputs: (key) -> (e, n, rel or None for a plain tensor, raw request, sparse request) and what the choice rule must answer
DELTA_CASES = {
    "d4": (4, 70001, 1e-5, AUTO, AUTO, 0b0001, 0b1100),
    "d2": (2, 70001, 1e-3, AUTO, AUTO, 0, 0b10),
    "d8": (8, 4097, 1e-5, AUTO, AUTO, 0b11111, 0b11100000),
}
PLAIN_CASES = {
    "p4": (4, 4097, None, AUTO, 0, 0b0111, 0),
    "p2_1": (2, 1, None, AUTO, 0, 0b11, 0),
    "p2_9": (2, 9, None, AUTO, 0, 0b11, 0),
}
CASES = dict(DELTA_CASES, **PLAIN_CASES)
N_VALS = {"d4": [69733, 25804, 93, 0], "d2": [35072, 204]}  # the non-zero bytes per plane of new ^ base


class Container:
    """the expected container of the tensor whose stored bytes are `src` (for a delta: new ^ base)"""

    def __init__(self, src, e, raw=AUTO, sparse=0, flags=0):
        self.e, self.n, self.flags = e, src.size // e, flags
        self.stored = st = forms_model.Stored(src, e, raw, sparse)
        self.raw, self.sparse = st.raw, st.sparse
        self.n_vals = [st.n_vals[p] if (st.sparse >> p) & 1 else 0 for p in range(e)]
        dirs = [(0, 0)] * DIR_ENTRIES
        parts, at = [], HEAD_BYTES

        def place(k, blob):
            nonlocal at
            dirs[k] = (at, int(blob.size))
            parts.append(blob)
            parts.append(np.zeros(pad16(blob.size) - blob.size, dtype=np.uint8))
            at += pad16(blob.size)

        self.tables, self.ranks = {}, {}
        for j in range(2 * e):  # the seek tables, j ascending: of every stream that has a code
            if st.kind[j] != "image":
                continue
            t = st.tables[j]
            self.tables[j] = range_worlds.expected_table(self._symbols(j), t["length"], 8 * (1040 + 8 * t["max_len"]))
            place(TABLES + j, self.tables[j])
        for p in range(e):  # the rank tables, p ascending: of every sparse plane
            if (st.sparse >> p) & 1:
                self.ranks[p] = sparse_range_model.table_of(st.planes[p])
                place(RANKS + p, self.ranks[p])
        self.streams_off = at
        for j in range(2 * e):  # the streams, j ascending
            if st.kind[j] is not None:
                place(STREAMS + j, st.data[j])
        self.total = at
        self.dir = dirs
        head = MAGIC + struct.pack("<IIQIIIIQ", 1, e, self.n, self.raw, self.sparse, flags, 0, self.total) + bytes(16) + \
            struct.pack("<8Q", *(self.n_vals + [0] * (8 - e)))
        assert len(head) == 128
        head += b"".join(struct.pack("<QQ", o, b) for o, b in dirs)
        assert len(head) == HEAD_BYTES
        self.bytes = np.concatenate([np.frombuffer(head, dtype=np.uint8)] + parts)
        assert self.bytes.size == self.total and self.total % 16 == 0

    def _symbols(self, j):
        """the byte string the stream of slot j decodes to"""
        st, e = self.stored, self.e
        pl = st.planes[j % e]
        if not (st.sparse >> (j % e)) & 1:
            return pl
        m, v = forms_model.sparse_form(pl)
        return m if j < e else v

    @property
    def head(self):
        return self.bytes[:HEAD_BYTES]


@functools.lru_cache(maxsize=None)
def case(key):
    """-> (base bytes or None, new bytes, Container) of a pinned input"""
    e, n, rel, raw, sparse, _, _ = CASES[key]
    base = forms_model.normal_elems(n, e, seed=7)
    if rel is None:
        return None, base, Container(base, e, raw, sparse, 0)
    new = new_of(base, e, rel)
    return base, new, Container(new ^ base, e, raw, sparse, DELTA)


def all_raw(n, e=2, seed=5):
    """an all-raw tensor of n elements (explicit masks): -> (bytes, Container); the smallest container there is"""
    src = np.random.default_rng(seed + n).integers(0, 256, size=n * e, dtype=np.uint8)
    return src, Container(src, e, (1 << e) - 1, 0, 0)
