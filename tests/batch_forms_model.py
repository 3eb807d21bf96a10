"""The host model of the plane batch calls with raw planes (include/ghf.h), in numpy over the CPU
oracle's histograms and codes: which planes the rule of ghf_batch_planes_raw_auto stores raw, and what a batch stores under
a mask.  Shared by tests/test_batch_forms_cpu.py (which pins the numbers) and tests/test_gpu_batch_forms.py (which holds the
device against them)."""
import numpy as np

from oracle import oracle as orc

# 64 items of 2048 standard-normal values from default_rng(7) under GHF_HIST_COVER_ALL codes: E -> (mask, stored bytes
# with that mask, stored bytes all dense), computed with the oracle
PINNED_NORMAL = {2: (0b01, 175120, 175235), 4: (0b0111, 437264, 437691), 8: (0b00111111, 919378, 920295)}
# 3 items of 17 elements: E -> mask under GHF_HIST_COVER_ALL codes (without: 0 for every E)
PINNED_TINY_COVER = {2: 0b1, 4: 0b0111, 8: 0b01111111}


def normal_elems(rng, n, e):
    """n standard-normal values as bf16 (the high half of the fp32), fp32 or fp64 -> uint8[n * e]"""
    x = rng.standard_normal(n)
    if e == 2:
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()
    return x.astype(np.float32 if e == 4 else np.float64).view(np.uint8).copy()


def normal_batch(e, items=64, n=2048, seed=7):
    rng = np.random.default_rng(seed)
    return [normal_elems(rng, n, e) for _ in range(items)]


def plane_hists(datas, e, cover=False):
    """what ghf_histogram_batch_planes leaves: int64[e, 257], slot 256 = 1"""
    h = np.zeros((e, 257), dtype=np.int64)
    for d in datas:
        for p in range(e):
            h[p, :256] += orc.histogram(np.ascontiguousarray(d[p::e]))[:256]
    if cover:
        h[h == 0] = 1
    h[:, 256] = 1
    return h


def build_codes(hists):
    return [orc.build_code(np.ascontiguousarray(hists[p])) for p in range(hists.shape[0])]


def lengths(code):
    return np.asarray(list(code.length), dtype=np.int64)


def raw_mask(hists, codes):
    """the rule, on the arrays as given: plane p is raw exactly when sum hist * length >= 8 * sum hist over the 256 byte
    values and the right side is not 0; a code whose min_len / max_len fail the length bounds leaves its plane dense.
    Python integers: the sums are exact."""
    mask = 0
    for p, code in enumerate(codes):
        if not (1 <= code.min_len <= code.max_len <= 32):
            continue
        h = [int(x) for x in hists[p][:256]]
        ln = [int(x) for x in lengths(code)[:256]]
        bits, syms = sum(a * b for a, b in zip(h, ln)), sum(h)
        if syms != 0 and bits >= 8 * syms:
            mask |= 1 << p
    return mask


def body_bytes(plane, code):
    """the size of the body ghf_compress_batch_shared writes for these bytes: the codes, the end mark, rounded up"""
    ln = lengths(code)
    return (int(ln[plane].sum()) + int(ln[256]) + 7) // 8


def stored_bytes(datas, e, codes, mask):
    """the sum over all slots of what the forms packer reports: n for a raw slot, the body's size for a dense one"""
    total = 0
    for d in datas:
        for p in range(e):
            total += d.size // e if mask >> p & 1 else body_bytes(d[p::e], codes[p])
    return total
