"""Synthesised histograms for the code builders (numpy only; no GPU, no numpy RNG: the family must never change).

The builders take a histogram, not data, so regimes that no file of testable size reaches are one microsecond-long launch
away: heap entries that differ only above or only below bit 32, every heap length with every sibling tied, exact
leaf-versus-merged ties, 257 live symbols in the package-merge, totals up to the edge of the heap word's domain (2^55,
include/ghf.h at ghf_build_code) and beyond it.

family()      -> [(label, int64[257], kind)], [256] == 1 always (the end mark); the .crs builder is fed [:256].
                 kind = what the CANONICAL builder (ghf_build_code) must do with the entry:
                   "fits"           the reference-exact code has at most 32 bits
                   "deep"           it has more: GHF_E_CODELEN by default, the package-merge tables under GHF_CODE_LIMIT
                   "out_of_domain"  the 257 counts sum to 2^55 or more: refused.  These entries hold uint64 counts; the
                                    array is their int64 bit pattern (h.view(np.uint64) are the counts).
                 Ordered so that entries with many and with few live symbols alternate: a small heap then runs right
                 after a large one has left stale slots below it.
crs_extras()  -> [(label, int64[256], expect)] for ghf_crs_build_code alone (no end mark): expect = the tree depth the
                 reference gives (63, 64; 65 is refused), or "empty" / "single".
family_sha256() -> one digest over every array of both lists, pinned in tests/golden/golden_hists.json.

Where k live symbols "sit at" positions: "first" = indices 0..k-1, "drawn" = k indices drawn by splitmix64 (values in
list order at ascending indices), "reversed" = the same indices with the values in reversed order.  The builders push
in ascending index order, so the placement changes the heap the same counts build.
"""
import hashlib

import numpy as np

import datagen as dg

NSYM = 257
DOMAIN_BITS = 55           # GHF_HIST_TOTAL_BITS
PIN_TOTAL = 65536          # entries up to this total are materialised as bytes and pinned to the compiled reference
PLACEMENTS = ("first", "drawn", "reversed")


def words(seed, n):
    """n splitmix64 words of stream `seed` (datagen's counter-based generator)."""
    k = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return dg.splitmix64(np.uint64(seed) + k * dg.GOLDEN)


def drawn_indices(k, seed):
    """k distinct byte values, ascending: the k smallest keys among 256 splitmix64 words."""
    return np.sort(np.argsort(words(seed, 256), kind="stable")[:k])


def place(values, placement, seed):
    values = [int(v) for v in values]
    k = len(values)
    assert 0 <= k <= 256
    h = np.zeros(NSYM, dtype=np.int64)
    if placement == "first":
        h[:k] = values
    elif placement == "drawn":
        h[drawn_indices(k, seed)] = values
    elif placement == "reversed":
        h[drawn_indices(k, seed)] = values[::-1]
    else:
        raise ValueError(placement)
    h[256] = 1
    return h


def fib(k):
    return dg.fib_counts(k)


def _ties():
    out = []
    for k in range(1, 257):  # all k symbols tie, at every heap length; reversed == drawn when all counts are equal
        for pl in ("first", "drawn"):
            out.append(("ties/c1/k%d/%s" % (k, pl), place([1] * k, pl, 1000 + k), "fits"))
    for k in range(8, 257, 8):
        for e in (32, 45):
            pl = ("first", "drawn")[(k // 8 + e) & 1]
            out.append(("ties/c2^%d/k%d/%s" % (e, k, pl), place([1 << e] * k, pl, 2000 + k), "fits"))
    return out


def _near_ties():
    out = []
    ks = list(range(1, 257, 5))  # 1, 6, .., 256
    for i, k in enumerate(ks):
        w = words(3000 + k, k)
        v123 = [1 + int(x % np.uint64(3)) for x in w]
        for pl in PLACEMENTS:  # (small totals: all three placements are pinned to the compiled reference)
            out.append(("near/123/k%d/%s" % (k, pl), place(v123, pl, 3000 + k), "fits"))
        for j, (name, c) in enumerate((("1000", 1000), ("2^33", 1 << 33))):
            v = [c + int((x >> np.uint64(17 + j)) & np.uint64(1)) for x in w]
            pl = PLACEMENTS[(i + j) % 3]
            out.append(("near/%s/k%d/%s" % (name, k, pl), place(v, pl, 3100 + k), "fits"))
    return out


CHAINS = {
    "fib": lambda k: fib(k),
    "fib2x": lambda k: [x for x in fib(k) for _ in (0, 1)],  # every term twice: 2k symbols
    "pow2": lambda k: [1 << i for i in range(k)],             # exact leaf-versus-merged ties
    "pow3": lambda k: [3 ** i for i in range(k)],
}
FILL_COUNT = 2  # the flat block that fills the remaining byte values of a "filled" chain
# A filled chain is the chain standing on a 7..8 level subtree of the flat block, so the longest ones no longer fit
# 32 bits.  Which ones is the reference heap's verdict, written down here and checked against the oracle by
# tests/test_hist_families_cpu.py.
DEEP_FILLED = {("pow3", k) for k in range(29, 33)} | {("pow2", 32)}


def _chains():
    out = []
    for ci, (name, gen) in enumerate(CHAINS.items()):
        for k in range(2, 33):
            v = gen(k)
            pls = PLACEMENTS if k % 4 == 0 else (PLACEMENTS[(k + ci) % 3],)
            for pl in pls:
                out.append(("chain/%s/k%d/%s" % (name, k, pl), place(v, pl, 4000 + 100 * ci + k), "fits"))
            pl = PLACEMENTS[(k + ci + 1) % 3]
            h = place(v, pl, 4000 + 100 * ci + k)
            h[:256][h[:256] == 0] = FILL_COUNT  # 257 live symbols
            out.append(("chain/%s/k%d/%s/filled" % (name, k, pl), h, "deep" if (name, k) in DEEP_FILLED else "fits"))
    # 45 Fibonacci terms, each twice: lands exactly on max_len 32
    out.append(("chain/fib2x/k45/first", place(CHAINS["fib2x"](45), "first", 0), "fits"))
    return out


def _total(h):
    return sum(int(x) for x in h.view(np.uint64))


def _wide(base):
    out = []
    for i, (label, h, kind) in enumerate(base[::10]):
        for s in (20, 33, 46):
            if (_total(h) - 1) << s >= (1 << DOMAIN_BITS) - 1:
                continue
            g = h.copy()
            g[:256] <<= s  # the end mark keeps its count of 1
            out.append(("wide/s%d/%s" % (s, label), g, kind))
    # entries of one heap that differ only in bits >= 32, (a_i << 32) + b, and only in bits < 32, (a << 32) + b_i
    for k in (2, 3, 17, 64, 200, 256):
        w = words(5000 + k, k)
        a_i = [1 + int(x % np.uint64(3)) for x in w]
        b_i = [int(x >> np.uint64(32)) for x in w]
        b_s = [1 + int((x >> np.uint64(40)) % np.uint64(3)) for x in w]
        pl = PLACEMENTS[k % 3]
        out.append(("wide/high-only/k%d/%s" % (k, pl), place([(a << 32) + 12345 for a in a_i], pl, 5000 + k), "fits"))
        out.append(("wide/low-only/k%d/%s" % (k, pl), place([(5 << 32) + b for b in b_i], pl, 5000 + k), "fits"))
        out.append(("wide/low-only-123/k%d/%s" % (k, pl), place([(5 << 32) + b for b in b_s], pl, 5000 + k), "fits"))
    # the last totals inside the domain.  256 counts of 2^47 - 1 are 2^55 - 256; the first one gives up another 300 so that
    # with the end mark the total is 2^55 - 555
    v = [(1 << 47) - 1] * 256
    v[0] -= 300
    out.append(("wide/total-2^55-555", place(v, "first", 0), "fits"))
    # 255 counts of 2^47, one of 2^47 - 2, the end mark: 2^55 - 1, the largest total the heap word holds
    v = [1 << 47] * 256
    v[255] -= 2
    out.append(("wide/total-2^55-1", place(v, "first", 0), "fits"))
    for label, h, _ in out[-2:]:
        assert _total(h) == (1 << 55) - (555 if label.endswith("555") else 1)
    return out


def _deep():
    out = [("deep/fib%d" % k, place(fib(k), "first", 0), "deep") for k in (33, 34, 40, 50, 60, 75)]
    v = fib(50)
    order = np.argsort(words(6050, 50), kind="stable")
    out.append(("deep/fib50/shuffled", place([v[int(i)] for i in order], "drawn", 6050), "deep"))
    out.append(("deep/pow3/k34", place([3 ** i for i in range(34)], "first", 0), "deep"))
    h = np.ones(NSYM, dtype=np.int64)  # 2^12 .. 2^47 at the odd byte values 1, 3, .., 71; ones everywhere else
    h[1:72:2] = [1 << e for e in range(12, 48)]
    out.append(("deep/pow2-12..47/ones", h, "deep"))
    h = place(fib(40) + [1] * 216, "first", 0)  # 257 live symbols: the ones lift the chain, the code has 24 bits
    out.append(("deep/fib40+216ones", h, "fits"))
    for _, h, _ in out:
        assert _total(h) < 1 << 54
    return out


def _out_of_domain():
    out = []
    # total exactly 2^55: 2^54 at byte value 0, 2^54 - 1 at byte value 1, and the end mark's 1
    h = place([1 << 54, (1 << 54) - 1], "first", 0)
    assert _total(h) == 1 << 55
    out.append(("ood/total-2^55", h, "out_of_domain"))
    # the same edge for the .crs builder, which does not read [256]: byte values 0 and 1 at 2^54 each
    out.append(("ood/two-2^54", place([1 << 54, 1 << 54], "first", 0), "out_of_domain"))
    for name, c in (("2^55", 1 << 55), ("2^63", 1 << 63), ("2^64-1", (1 << 64) - 1)):
        u = np.zeros(NSYM, dtype=np.uint64)
        u[7] = c
        u[256] = 1
        out.append(("ood/single-%s" % name, u.view(np.int64).copy(), "out_of_domain"))
    return out


def n_live(h):
    return int(np.count_nonzero(h[:256]))


def total(h):
    """the sum of the 257 counts as a Python int (out_of_domain entries are uint64)"""
    return _total(h)


_cache = {}


def family():
    if "family" not in _cache:
        base = _ties() + _near_ties() + _chains()
        every = base + _wide(base) + _deep() + _out_of_domain()
        assert len({label for label, _, _ in every}) == len(every)
        by_size = sorted(range(len(every)), key=lambda i: (n_live(every[i][1]), i))
        order, lo, hi = [], 0, len(by_size) - 1
        while lo <= hi:  # most live symbols, fewest, second most, second fewest, ..
            order.append(by_size[hi])
            if lo < hi:
                order.append(by_size[lo])
            hi -= 1
            lo += 1
        fam = [every[i] for i in order]
        for _, h, _ in fam:
            assert h.dtype == np.int64 and h.shape == (NSYM,) and h[256] == 1
            h.setflags(write=False)
        _cache["family"] = fam
    return _cache["family"]


def crs_extras():
    if "crs" not in _cache:
        out = []
        for k, depth in ((64, 63), (65, 64), (66, 65)):
            out.append(("crs/fib%d" % k, place(fib(k), "first", 0)[:256].copy(), depth))
        out.append(("crs/empty", np.zeros(256, dtype=np.int64), "empty"))
        one = np.zeros(256, dtype=np.int64)
        one[99] = 5
        out.append(("crs/single", one, "single"))
        for _, h, _ in out:
            h.setflags(write=False)
        _cache["crs"] = out
    return _cache["crs"]


def pinned():
    """[(entry number, label, int64[257])]: the entries small enough to exist as a byte stream (total <= PIN_TOTAL)"""
    return [(i, label, h) for i, (label, h, kind) in enumerate(family()) if kind != "out_of_domain" and total(h) <= PIN_TOTAL]


def materialise(i, h):
    """entry number i as bytes: exactly h[v] occurrences of byte value v"""
    return dg.counts_to_bytes(h[:256], seed=i)


def family_sha256():
    m = hashlib.sha256()
    for _, h, _ in family():
        m.update(np.ascontiguousarray(h, dtype="<i8").tobytes())
    for _, h, _ in crs_extras():
        m.update(np.ascontiguousarray(h, dtype="<i8").tobytes())
    return m.hexdigest()
