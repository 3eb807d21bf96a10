"""A numpy model of the rank table of a sparse byte string and of the plan of ghf_decode_planes_sparse_range (DESIGN.md
section 21): the table's bytes, and -- for one string and one range -- the origin, the rank blocks, the two cum entries, the
sub-string's mask bytes and values, the merge of the sub-string and the lead that the final merge skips.  Nothing here
touches the library; tests/test_sparse_range_cpu.py holds the model against x[first : first + count] and the library's
host-side parse against the model's tables, tests/test_gpu_sparse_range.py holds the kernels against both."""
import numpy as np

RANK_ELEMS = 32768            # GHF_SPARSE_RANK_ELEMS
RANK_MASK_BYTES = RANK_ELEMS // 8   # 4096: one seek block of the mask's stream
SEEK_BLOCK = 4096
HEADER_BYTES = 64
MAGIC = b"GHFRANK1"


def rank_blocks(n):
    return -(-n // RANK_ELEMS)


def rank_bytes(n):
    return HEADER_BYTES + 8 * (rank_blocks(n) + 1)


def sparse_form(x):
    """(mask, vals): bit k & 7 of mask[k >> 3] = (x[k] != 0), pad bits 0; vals = x[x != 0] in order"""
    nz = x != 0
    return np.packbits(nz, bitorder="little"), np.ascontiguousarray(x[nz])


def cum_of(x):
    """cum[j] = the non-zero bytes of x[0 : 32768 j), j = 0 .. blocks"""
    n, nb = x.size, rank_blocks(x.size)
    return np.array([int(np.count_nonzero(x[: min(j * RANK_ELEMS, n)])) for j in range(nb + 1)], dtype=np.uint64)


def table_of(x):
    """the rank table of the byte string x as uint8[rank_bytes(n)], little-endian"""
    cum = cum_of(x)
    head = MAGIC + (1).to_bytes(4, "little") + RANK_ELEMS.to_bytes(4, "little") + x.size.to_bytes(8, "little") + \
        int(cum[-1]).to_bytes(8, "little") + rank_blocks(x.size).to_bytes(8, "little") + bytes(24)
    assert len(head) == HEADER_BYTES
    return np.frombuffer(head + cum.astype("<u8").tobytes(), dtype=np.uint8).copy()


def cum_in(table):
    return np.frombuffer(table.tobytes()[HEADER_BYTES:], dtype="<u8")


def merge(mask, vals, n):
    """the sparse merge: the string of n bytes whose mask and values these are; the set bits must number the values and the
    pad bits must be clear (what the kernel latches GHF_E_CORRUPT for is an assertion here)"""
    bits = np.unpackbits(mask, bitorder="little")
    assert not bits[n:].any() and int(bits[:n].sum()) == vals.size
    out = np.zeros(n, dtype=np.uint8)
    out[bits[:n].astype(bool)] = vals
    return out


def plan(n, first, count):
    """what depends on the range alone"""
    assert count > 0 and first + count <= n
    origin = first - first % RANK_ELEMS
    end = first + count
    b0, b1 = origin // RANK_ELEMS, -(-end // RANK_ELEMS)
    mask_bytes = (n + 7) // 8
    return {"from": origin, "end": end, "b0": b0, "b1": b1, "lead": first - origin, "sub_n": min(RANK_ELEMS * b1, n) - origin,
            "m_lo": RANK_MASK_BYTES * b0, "m_hi": min(RANK_MASK_BYTES * b1, mask_bytes)}


def sparse_range(mask, vals, table, n, first, count):
    """elements [first, first + count) of the string, the way the range call gets them: from the covered mask bytes, the
    values between the two cum entries (read from where their seek block starts, like the decode) and the table"""
    p = plan(n, first, count)
    cum = cum_in(table)
    v_lo, v_hi = int(cum[p["b0"]]), int(cum[p["b1"]])
    assert v_lo <= v_hi <= vals.size and v_hi - v_lo <= p["sub_n"]
    sub_mask = mask[p["m_lo"] : p["m_hi"]]
    assert sub_mask.size == (p["sub_n"] + 7) // 8
    v_start = v_lo - v_lo % SEEK_BLOCK
    decoded = vals[v_start:v_hi] if v_hi > v_lo else vals[:0]   # nothing is decoded when the sub-string has no value
    skip = v_lo % SEEK_BLOCK
    sub = merge(sub_mask, decoded[skip : skip + (v_hi - v_lo)], p["sub_n"])
    assert p["lead"] < RANK_ELEMS and p["sub_n"] - p["lead"] - count < RANK_ELEMS   # the over-decode bound, on both sides
    p.update(v_lo=v_lo, v_hi=v_hi, vals_skip=skip, out=sub[p["lead"] : p["lead"] + count])
    return p
