"""ghf_decode_planes_gather_forms restated in numpy (include/ghf.h): which runs of a sparse plane's mask
and values streams a row covers, the rank of its first element, the checks on rank entries and pad bits, the order of the
verdicts, and the bytes of every row.  Builds on tests/gather_model.py (rows, runs, blocks, the stream checks) and
tests/sparse_range_model.py (the sparse form and its rank table); nothing here is imported from the library.

  row r        elements [index[r] * index_stride, + row_elems) of a tensor of n elements, E planes
  plane p      raw: the plane's bytes; dense: a .crs2 stream with a seek table; sparse: a mask stream (bit k & 7 of byte k >> 3
               says byte k is non-zero; 4096 mask bytes per rank block of 32768 elements), a values stream and cum[]
  GHF_E_FORMAT on every row when the code of a stored stream is not a complete prefix code
  GHF_E_INVAL  the row passes n, or its start overflows 64 bits
  GHF_E_CORRUPT for a dense plane what gather_model says; for a sparse plane, with b0 = first // 32768:
      1  cum[b0] <= cum[b0 + 1] (<= cum[b0 + 2] where the row crosses into block b0 + 1) <= n_vals, and no step exceeds the
         elements of its block
      2  the mask stream's runs of 512 bytes [8 b0, ceil(mend / 512)) pass gather_model's block and run checks, mend = the mask
         bytes up to the row's end
      3  r0 = the set bits of [32768 b0, first), nv = the row's own; where the decoded runs hold a rank block to its end (or
         the tensor's) the block's set bits (of elements below n) equal the difference of its two entries; where the row touches
         the last mask byte its pad bits are 0; cum[b0] + r0 + nv <= n_vals
      4  nv > 0: the values stream's runs [v0 // 512, ceil((v0 + nv) / 512)), v0 = cum[b0] + r0, pass the same checks
  element k of the row gets value number v0 + (set bits of the row in front of k) where its bit is set, else 0; XOR the base"""
import numpy as np

import gather_model as gm
import sparse_range_model as srm

OK, E_INVAL, E_FORMAT, E_CORRUPT = gm.OK, gm.E_INVAL, gm.E_FORMAT, gm.E_CORRUPT
RANK, RANK_MASK, RUN = srm.RANK_ELEMS, srm.RANK_MASK_BYTES, gm.RUN
SPARSE_MAX_ROW_ELEMS = 8192
ROW_ELEMS = (1, 7, 513, 4096, 8192)


def mask_runs(n, first, count):
    """-> (b0, first run, runs, decoded mask bytes counted from the start of rank block b0): whole runs of 512 mask bytes from
    the block's start to the row's end, cut where the mask ends"""
    assert 1 <= count <= SPARSE_MAX_ROW_ELEMS and first + count <= n
    b0 = first // RANK
    mend = -(-(first + count) // 8) - RANK_MASK * b0
    runs = -(-mend // RUN)
    decoded = min(runs * RUN, (n + 7) // 8 - RANK_MASK * b0)
    assert runs <= 11
    return b0, 8 * b0, runs, decoded


def value_runs(v0, nv):
    """-> (first run, runs) of the values stream that hold values [v0, v0 + nv)"""
    assert nv >= 1 and nv <= SPARSE_MAX_ROW_ELEMS
    runs = -(-(v0 % RUN + nv) // RUN)
    assert runs <= 17
    return v0 // RUN, runs


def ranks_of(mask, n, first, count):
    """(r0, nv) from the mask's bits"""
    bits = np.unpackbits(np.ascontiguousarray(mask, dtype=np.uint8), bitorder="little")
    lo = first - first % RANK
    return int(bits[lo:first].sum()), int(bits[first : first + count].sum())


def stream_ok(stream_plane, first_sym, n_syms, total):
    """gather_model's verdict on symbols [first_sym, first_sym + n_syms) of one stored stream of `total` symbols"""
    return gm.row_verdict(first_sym, 1, n_syms, total, [stream_plane]) == OK


def sparse_verdict(sp, n, first, count):
    """sp: {mask, vals: the bytes the two streams hold; cum: the table's entries as they lie on the device; n_vals: what the rank
    info counts; mask_stream, vals_stream: gather_model plane dicts (vals_stream None when n_vals == 0)} -> (verdict, v0, nv)"""
    b0, run0, runs, decoded = mask_runs(n, first, count)
    cum = [int(v) for v in sp["cum"]]
    crosses = first % RANK + count > RANK
    len0 = min(RANK, n - RANK * b0)
    len1 = min(RANK, n - RANK * (b0 + 1)) if crosses else 0
    c0, c1 = cum[b0], cum[b0 + 1]
    c2 = cum[b0 + 2] if crosses else c1
    if not (c0 <= c1 <= c2 <= sp["n_vals"]) or c1 - c0 > len0 or c2 - c1 > len1:
        return E_CORRUPT, None, None
    mask_total = (n + 7) // 8
    mend = -(-(first + count) // 8)
    if not stream_ok(sp["mask_stream"], RANK_MASK * b0, mend - RANK_MASK * b0, mask_total):
        return E_CORRUPT, None, None
    bits = np.unpackbits(np.ascontiguousarray(sp["mask"], dtype=np.uint8), bitorder="little")
    r0, nv = ranks_of(sp["mask"], n, first, count)
    lo = RANK * b0
    if decoded >= (len0 + 7) // 8 and int(bits[lo : lo + len0].sum()) != c1 - c0:
        return E_CORRUPT, None, None
    if len1 and decoded >= RANK_MASK + (len1 + 7) // 8 and int(bits[lo + RANK : lo + RANK + len1].sum()) != c2 - c1:
        return E_CORRUPT, None, None
    if mend == mask_total and n % 8 and bits[n : 8 * mask_total].any():
        return E_CORRUPT, None, None
    if c0 + r0 + nv > sp["n_vals"]:
        return E_CORRUPT, None, None
    v0 = c0 + r0
    if nv and not stream_ok(sp["vals_stream"], v0, nv, sp["n_vals"]):
        return E_CORRUPT, None, None
    return OK, v0, nv


def row_verdict(index, index_stride, row_elems, n, planes):
    """planes: per plane ("raw", bytes), ("dense", gather_model plane dict) or ("sparse", sp).  The verdicts in the call's
    order: the codes, the row's place, then every plane"""
    for kind, pl in planes:
        if kind == "dense" and not pl["code_ok"]:
            return E_FORMAT
        if kind == "sparse" and not (pl["mask_stream"]["code_ok"] and (pl["vals_stream"] is None or pl["vals_stream"]["code_ok"])):
            return E_FORMAT
    first = int(index) * int(index_stride)
    if first >= 1 << 64 or first > n or row_elems > n - first:
        return E_INVAL
    for kind, pl in planes:
        if kind == "dense" and gm.row_verdict(first, 1, row_elems, n, [pl]) != OK:
            return E_CORRUPT
        if kind == "sparse" and sparse_verdict(pl, n, first, row_elems)[0] != OK:
            return E_CORRUPT
    return OK


def plane_row(kind, pl, n, first, count):
    """the bytes plane `pl` gives elements [first, first + count), the way the call gets them (the row's verdict is OK)"""
    if kind == "raw":
        return np.asarray(pl, dtype=np.uint8)[first : first + count]
    if kind == "dense":
        return np.asarray(pl["data"], dtype=np.uint8)[first : first + count]
    st, v0, nv = sparse_verdict(pl, n, first, count)
    assert st == OK
    bits = np.unpackbits(np.ascontiguousarray(pl["mask"], dtype=np.uint8), bitorder="little")[first : first + count].astype(bool)
    out = np.zeros(count, dtype=np.uint8)
    out[bits] = np.asarray(pl["vals"], dtype=np.uint8)[v0 : v0 + nv]
    return out


def expected_rows(planes, n, base, indices, index_stride, row_elems, statuses, out, out_stride):
    """what the call leaves in `out` (a uint8 array holding the fill pattern): the rows whose status is OK, XOR the base's"""
    e = len(planes)
    for r, (i, st) in enumerate(zip(indices, statuses)):
        if st != OK:
            continue
        first = int(i) * int(index_stride)
        row = np.stack([plane_row(k, pl, n, first, row_elems) for k, pl in planes], axis=1).reshape(-1)
        if base is not None:
            row = row ^ np.asarray(base, dtype=np.uint8)[first * e : (first + row_elems) * e]
        out[r * out_stride : r * out_stride + row_elems * e] = row
    return out
