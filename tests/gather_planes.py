"""The tensors of the gather tests (tests/test_planes_gather_cpu.py, tests/test_gpu_planes_gather.py), built with the oracle
only: every byte plane of a tensor comes from another code class, and its stream, code and seek table are the oracle's and
range_worlds.expected_table's.  No GPU is needed here.

  len12    a slice of the range_worlds world of that name; the slice's own code has max_len 14: the miss path of the small
           decoder (the whole world stops at 12 bits, its first 12805 bytes do not)
  short    codes of 1 to 4 bits
  len9     near-uniform bytes: 8- and 9-bit codes, an image larger than the plane (what GHF_RAW_AUTO stores raw)
  long     Fibonacci-like counts: codes of 16 bits and more
  len14, len8, pair5, nonstat   slices of the other worlds (len14: the world whose max_len exceeds 12, 13 bits in the slice)

A tensor of E planes takes the first E classes, so bf16 (E = 2) holds the miss path and the short codes and fp32 (E = 4) all
four classes the tests name.  Plane 0 is the one whose table the GPU test damages: Huffman codes self-synchronise, and a run
entered one bit late CAN land on its recorded end with the right number of symbols (in the len14 and long slices run 4 of
block 1 does) -- no check on lengths can see that.  tests/test_planes_gather_cpu.py holds plane 0 to not being such a case."""
import functools

import numpy as np

import datagen as dg
import gather_model as gm
import range_worlds as rw
from oracle import oracle as orc

N_SMALL = 3 * 4096 + 517  # a ragged last block, and a last run of 5 symbols
# room for one row of GHF_GATHER_MAX_ROW_ELEMS from element 700 on, 65 runs, in front of a ragged last block (eight blocks and
# 517 elements would end 183 elements short of such a row)
N_CAP = 9 * 4096 + 517
CLASSES = ["len12", "short", "len9", "long", "len14", "len8", "pair5", "nonstat"]


def _long(n):
    counts = dg.fib_counts(18)
    counts[-1] += n - sum(counts)
    return dg.counts_to_bytes(counts, seed=31)


def plane_bytes(cls, n):
    if cls == "short":
        return dg.weighted_bytes(n, dg.thresholds_from_probs([8, 4, 2, 1]), seed=7, values=[3, 200, 17, 99])
    if cls == "long":
        return _long(n)
    return rw.world(cls).data[:n]


class Plane:
    """one byte plane and what the oracle says about it"""

    def __init__(self, cls, n):
        self.cls, self.n = cls, n
        self.data = np.ascontiguousarray(plane_bytes(cls, n), dtype=np.uint8)
        assert self.data.size == n
        self.code = orc.build_code(orc.histogram(self.data))
        self.length = [int(v) for v in self.code.length]
        self.codeword = [int(v) for v in self.code.codeword]
        self.min_len, self.max_len = int(self.code.min_len), int(self.code.max_len)
        self.stream = orc.compress(self.data)
        self.stream_bytes = int(self.stream.size)
        self.first_bit = 8 * int(orc.header_bytes(self.code).size)
        self.table = rw.expected_table(self.data, self.length, self.first_bit)

    def model(self, table=None, stream_bytes=None, code_ok=True):
        """the plane as gather_model.row_verdict takes it, with a damaged table or a cut stream in place of the true one"""
        return {"table": self.table if table is None else table, "true_table": self.table, "stream": self.stream,
                "stream_bytes": self.stream_bytes if stream_bytes is None else stream_bytes, "length": self.length,
                "codeword": self.codeword, "code_ok": code_ok}


class Tensor:
    def __init__(self, e, n):
        self.e, self.n = e, n
        self.planes = [Plane(c, n) for c in CLASSES[:e]]
        self.bytes = np.ascontiguousarray(np.stack([p.data for p in self.planes], axis=1)).reshape(-1)  # element k: bytes k*e ..
        # what GHF_RAW_AUTO chooses: a plane whose image would be at least n bytes
        self.raw_auto = sum(1 << i for i, p in enumerate(self.planes) if p.stream_bytes >= n)

    def rows(self, indices, index_stride, row_elems):
        return [self.bytes[int(i) * index_stride * self.e : (int(i) * index_stride + row_elems) * self.e] for i in indices]

    def model_planes(self, raw):
        return [None if raw >> i & 1 else p.model() for i, p in enumerate(self.planes)]


@functools.lru_cache(maxsize=None)
def tensor(e, n=N_SMALL):
    return Tensor(e, n)


def row_cases(n):
    """-> [(row_elems, index_stride, indices)]: every row length of the model's list, by element offset (stride 1: the model's
    firsts, in descending order, the first of them repeated) and by row id (stride = row_elems: rows 0, 1, 2 and the last whole
    one, descending, one repeated)"""
    out = []
    for re_ in gm.ROW_ELEMS:
        firsts = sorted(gm.row_firsts(n, re_), reverse=True)
        out.append((re_, 1, firsts + firsts[:1]))
        ids = sorted({0, 1, 2, n // re_ - 1} & set(range(n // re_)), reverse=True)
        out.append((re_, re_, ids + ids[-1:]))
    return out
