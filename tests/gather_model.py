"""ghf_decode_planes_gather restated in numpy: which runs a row covers, where a run starts, and what every row's verdict is.

Nothing here is imported from the library.  The row rule, the order of the verdicts and the checks on tables and streams
are written down from the call's specification (include/ghf.h):

  row r        elements [index[r] * index_stride, + row_elems) of a tensor of n elements
  GHF_E_FORMAT on every row when the code of a dense plane is not a complete prefix code
  GHF_E_INVAL  index[r] * index_stride overflows 64 bits, or the row passes n
  GHF_E_CORRUPT for any dense plane: a covered block's start_bit + sum(run_bits) lies beyond bit 8 * stream_bytes or is not
               the next block's start_bit; a covered run does not land exactly on its recorded end after its symbols, meets
               an end mark, or meets bits that start no code
  a failed row stores nothing; the other rows are unaffected

A seek table is 64 header bytes, then per block of 4096 symbols {u64 start_bit, u16 run_bits[8]}: the bit lengths of the
block's eight runs of 512 symbols."""
import numpy as np

OK, E_INVAL, E_FORMAT, E_CORRUPT = 0, 1, 6, 7
BLOCK, RUN, RUNS_PER_BLOCK = 4096, 512, 8
HEADER = 64
MAX_ROW_ELEMS = 32768
END_MARK = 256
REC = np.dtype([("start", "<u8"), ("run", "<u2", (RUNS_PER_BLOCK,))])

# the row shapes of tests/test_gpu_planes_gather.py: one symbol, a few, a whole run, a run and a symbol, a block, a block
# and a symbol
ROW_ELEMS = (1, 7, 512, 513, 4096, 4097)


def row_firsts(n, row_elems):
    """the first elements the GPU test asks for at this row length, inside a tensor of n elements: the tensor's start, both
    sides of a run edge and of a block edge, the row that ends exactly at n, and (row_elems == 1) the last element"""
    out = [0, 511, 512, 513, 4095, 4096, 4097, n - row_elems]
    return [f for f in dict.fromkeys(out) if 0 <= f and f + row_elems <= n]


def covered(first, count, n):
    """-> [(block, run, symbols in the run, symbols to skip, symbols to take)] for the runs that elements [first, first +
    count) of n touch, in order; the takes add up to count"""
    assert count >= 1 and first + count <= n
    out = []
    for r in range(first // RUN, (first + count - 1) // RUN + 1):
        lo, hi = r * RUN, min(r * RUN + RUN, n)
        a, b = max(first, lo), min(first + count, hi)
        out.append((r // RUNS_PER_BLOCK, r % RUNS_PER_BLOCK, hi - lo, a - lo, b - a))
    return out


def records(table):
    t = np.ascontiguousarray(table, dtype=np.uint8)
    return np.frombuffer(t[HEADER:].tobytes(), dtype=REC)


def run_start(table, block, run):
    """the bit a run starts at: its block's start_bit plus the lengths of the runs in front of it"""
    rec = records(table)[block]
    return int(rec["start"]) + int(rec["run"][:run].astype(np.int64).sum())


def block_ok(table, block, stream_bytes):
    """the record lies inside the stream, and the block ends where the next one starts"""
    rec = records(table)
    end = int(rec[block]["start"]) + int(rec[block]["run"].astype(np.int64).sum())
    if end > 8 * stream_bytes:
        return False
    return block + 1 >= rec.size or end == int(rec[block + 1]["start"])


class Decoder:
    """a prefix code as (length, codeword) -> symbol, read MSB first from a byte string; zeros behind the string"""

    def __init__(self, length, codeword):
        self.by_len = {}
        for s in range(257):
            if length[s]:
                self.by_len.setdefault(int(length[s]), {})[int(codeword[s])] = s
        self.lens = sorted(self.by_len)

    def run_bits(self, stream, stream_bytes, bit, cnt):
        """bits that `cnt` codes from `bit` on take, or None: bits that start no code, or an end mark among them"""
        s = np.ascontiguousarray(stream, dtype=np.uint8)[:stream_bytes]
        need = cnt * 32 + 64
        b0 = bit // 8
        chunk = np.zeros(need // 8 + 9, dtype=np.uint8)
        have = s[b0 : b0 + chunk.size]
        chunk[: have.size] = have
        bits = np.unpackbits(chunk)
        pos = bit - 8 * b0
        start = pos
        for _ in range(cnt):
            acc, l, sym = 0, 0, None
            for want in self.lens:
                while l < want:
                    acc = acc << 1 | int(bits[pos + l])
                    l += 1
                sym = self.by_len[want].get(acc)
                if sym is not None:
                    break
            if sym is None or sym == END_MARK:
                return None
            pos += l
        return pos - start


def row_verdict(index, index_stride, row_elems, n, planes):
    """planes: per plane None (raw) or a dict {table, stream, stream_bytes, length, codeword, code_ok, true_table}: true_table is
    the table the stream was written with, and stream[:stream_bytes] a prefix of what was written -- a run whose record equals
    the true one and lies inside the prefix is known to land, the others are decoded here"""
    if any(p is not None and not p["code_ok"] for p in planes):
        return E_FORMAT
    first = int(index) * int(index_stride)
    if first >= 1 << 64 or first > n or row_elems > n - first:
        return E_INVAL
    for p in planes:
        if p is None:
            continue
        runs = covered(first, row_elems, n)
        for g in dict.fromkeys(b for b, *_ in runs):
            if not block_ok(p["table"], g, p["stream_bytes"]):
                return E_CORRUPT
        rec, true = records(p["table"]), records(p["true_table"])
        dec = None
        for g, k, cnt, _, _ in runs:
            start, bits = run_start(p["table"], g, k), int(rec[g]["run"][k])
            if start == run_start(p["true_table"], g, k) and bits == int(true[g]["run"][k]) and start + bits <= 8 * p["stream_bytes"]:
                continue
            dec = dec or Decoder(p["length"], p["codeword"])
            if dec.run_bits(p["stream"], p["stream_bytes"], start, cnt) != bits:
                return E_CORRUPT
    return OK


def gather_rows(tensor_bytes, elem_bytes, indices, index_stride, row_elems, statuses, out, out_stride):
    """what the call leaves in `out` (a uint8 array holding the fill pattern): the rows whose status is OK"""
    t = np.ascontiguousarray(tensor_bytes, dtype=np.uint8)
    for r, (i, st) in enumerate(zip(indices, statuses)):
        if st == OK:
            first = int(i) * int(index_stride)
            out[r * out_stride : r * out_stride + row_elems * elem_bytes] = t[first * elem_bytes : (first + row_elems) * elem_bytes]
    return out
