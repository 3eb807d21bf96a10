"""The tensors of the forms gather tests (tests/test_planes_gather_forms_cpu.py, tests/test_gpu_planes_gather_forms.py), built
with the oracle only: every stored stream -- a dense plane, a sparse plane's mask, its values -- is the oracle's .crs2 image,
its seek table is range_worlds.expected_table's and a rank table is sparse_range_model.table_of's.  No GPU is needed here.

A tensor has n = 2 * 32768 + 4096 + 517 elements: three rank blocks, the last one ragged, and a last mask byte with three pad
bits.  Its planes are the XOR-DELTA of `new` against `base`, in these forms (a letter per plane):

  s  sparse, 1 % non-zero
  z  sparse, all zero: n_vals == 0, no values stream
  r  sparse, 1 % non-zero and a run of 8192 consecutive non-zero bytes from element RUN_AT on: a row inside it has
     nv == row_elems, the run crosses the edge of rank blocks 0 and 1, and the ranks inside it take every value modulo 4096
  d  dense, codes of 1 to 4 bits
  w  raw: uniform bytes"""
import functools

import numpy as np

import datagen as dg
import gather_forms_model as fm
import gather_model as gm
import range_worlds as rw
import sparse_range_model as srm
from oracle import oracle as orc

N = 2 * 32768 + 4096 + 517
RUN_AT, RUN_LEN = 32768 - 3000, 8192
FORMS = {2: "rd", 4: "swzd", 8: "rdwzsdws"}


def _sparse_bytes(n, seed, run):
    keep = dg.uniform_bytes(n, seed=seed) < 3  # about 1 %
    x = np.where(keep, dg.uniform_bytes(n, seed=seed + 1) | 1, 0).astype(np.uint8)
    if run:
        x[RUN_AT : RUN_AT + RUN_LEN] = dg.uniform_bytes(RUN_LEN, seed=seed + 2) | 1
    return x


def plane_bytes(form, n, seed):
    if form == "z":
        return np.zeros(n, dtype=np.uint8)
    if form in "sr":
        return _sparse_bytes(n, seed, form == "r")
    if form == "d":
        return np.ascontiguousarray(dg.weighted_bytes(n, dg.thresholds_from_probs([8, 4, 2, 1]), seed=seed, values=[3, 200, 17, 99]))
    return np.ascontiguousarray(dg.uniform_bytes(n, seed=seed))


class Stream:
    """a byte string as a stored stream: the oracle's image and code, expected_table's seek table"""

    def __init__(self, data):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.n = int(self.data.size)
        self.code = orc.build_code(orc.histogram(self.data))
        self.length = [int(v) for v in self.code.length]
        self.codeword = [int(v) for v in self.code.codeword]
        self.stream = orc.compress(self.data)
        self.stream_bytes = int(self.stream.size)
        self.first_bit = 8 * int(orc.header_bytes(self.code).size)
        self.table = rw.expected_table(self.data, self.length, self.first_bit)

    def model(self, table=None, stream_bytes=None, code_ok=True):
        return {"table": self.table if table is None else table, "true_table": self.table, "stream": self.stream,
                "stream_bytes": self.stream_bytes if stream_bytes is None else stream_bytes, "length": self.length,
                "codeword": self.codeword, "code_ok": code_ok, "data": self.data}


class Plane:
    """one plane in its form: `streams` are its stored streams in slot order (the plane or its mask; a sparse plane's values)"""

    def __init__(self, form, data, mask=None):
        self.form, self.data, self.n = form, data, int(data.size)
        self.kind = {"w": "raw", "d": "dense"}.get(form, "sparse")
        self.mask = self.vals = self.rank = self.main = self.values = None
        if self.kind == "dense":
            self.main = Stream(data)
        elif self.kind == "sparse":
            true_mask, self.vals = srm.sparse_form(data)
            self.mask = true_mask if mask is None else mask  # (a damaged mask: the stream holds it, the rank table the truth)
            self.rank = srm.table_of(data)
            self.n_vals = int(self.vals.size)
            self.main = Stream(self.mask)
            self.values = Stream(self.vals) if self.n_vals else None

    def model(self, cum=None, mask_stream=None, vals_stream=None):
        """the plane as gather_forms_model takes it, with damaged parts in place of the true ones"""
        if self.kind == "raw":
            return "raw", self.data
        if self.kind == "dense":
            return "dense", self.main.model()
        return "sparse", {"mask": self.mask, "vals": self.vals, "cum": srm.cum_in(self.rank) if cum is None else cum, "n_vals": self.n_vals,
                          "mask_stream": self.main.model() if mask_stream is None else mask_stream,
                          "vals_stream": (self.values.model() if self.values else None) if vals_stream is None else vals_stream}

    def stored_bytes(self):
        if self.kind == "raw":
            return self.n
        return self.main.stream_bytes + (self.values.stream_bytes if self.values else 0)


class Tensor:
    def __init__(self, e, n=N):
        self.e, self.n, self.forms = e, n, FORMS[e]
        self.planes = [Plane(f, plane_bytes(f, n, 100 + 10 * i)) for i, f in enumerate(self.forms)]
        self.delta = np.ascontiguousarray(np.stack([p.data for p in self.planes], axis=1)).reshape(-1)  # element k: bytes k*e ..
        self.base = np.ascontiguousarray(dg.uniform_bytes(n * e, seed=9))
        self.new = self.delta ^ self.base
        self.raw = sum(1 << i for i, p in enumerate(self.planes) if p.kind == "raw")
        self.sparse = sum(1 << i for i, p in enumerate(self.planes) if p.kind == "sparse")

    def model_planes(self):
        return [p.model() for p in self.planes]

    def rows(self, indices, index_stride, row_elems, with_base):
        src = self.new if with_base else self.delta
        return [src[int(i) * index_stride * self.e : (int(i) * index_stride + row_elems) * self.e] for i in indices]


@functools.lru_cache(maxsize=None)
def tensor(e):
    return Tensor(e)


def rank_in(plane, first):
    """the number of the first value at or behind element `first` of a sparse plane"""
    return int(np.count_nonzero(plane.data[:first]))


def row_firsts(t, row_elems):
    """the first elements the GPU test asks for at this row length: the tensor's start, both sides of the first rank-block edge, a
    row across it, a row across the second edge, the row that ends at n (its last mask byte has pad bits), and -- inside the run
    of the `r` plane -- rows whose first value stands just in front of a 512 edge and of a 4096 edge of the values stream"""
    n = t.n
    out = [0, 32767, 32768, 32768 - (row_elems + 1) // 2, 65536 - 1, n - row_elems]
    runs = [p for p in t.planes if p.form == "r"]
    if runs:
        r_at = rank_in(runs[0], RUN_AT)
        for edge in (512, 4096):
            k = (edge - 3 - r_at) % edge  # value r_at + k stands three in front of an edge
            if k + row_elems <= RUN_LEN or row_elems >= 4096:
                out.append(RUN_AT + k)
    return [f for f in dict.fromkeys(out) if 0 <= f and f + row_elems <= n]


def row_cases(t):
    """-> [(row_elems, indices)] by element offset (stride 1), in descending order, the first of them repeated"""
    out = []
    for re_ in fm.ROW_ELEMS:
        firsts = sorted(row_firsts(t, re_), reverse=True)
        out.append((re_, firsts + firsts[:1]))
    return out
