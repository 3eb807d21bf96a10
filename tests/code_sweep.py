"""Every code shape for the kernels that take a caller's code (numpy and the oracle only; no GPU, no numpy RNG: every
choice comes from datagen.splitmix64 through hist_families.words, so the cases can never change).

A kernel that is handed a ghf_code only needs data over that code's live symbols, so a code of 32 bits is driven here by
items of a few hundred bytes where a data-derived one needs megabytes.  The codes are the ones orc.build_code gives for
the "fits" entries of tests/hist_families.py (and for EXTRA_HISTS, the sweep's own list), grouped by
(min_len, max_len, decoder class, live-symbol bucket); `per_group` codes are drawn from every group.

pool()            -> [Entry]: label, hist, code (OrcCode), length[257], min_len, max_len, variant (range_worlds.
                     decoder_class), bucket, live (the live byte symbols), header (orc.header_bytes)
left_out()        -> the labels of the "fits" entries without a live byte symbol; nothing else is skipped
items(entry)      -> [Item]: name, mode, data (uint8), body (orc_encode_body), ranges [(first, count)] * 3
typed_cases(e)    -> [Typed]: name, e, n, entries (one pool Entry per plane), planes [uint8[n]] * e, tensor, base, new
                     (= base ^ tensor), ranges [(first, count)] * 3 in elements
image / record / table of an item: header || body, the run record of test_gpu_batch_seek.record_of, and
                     range_worlds.expected_table -- all from the oracle's code lengths; expected_index() is the side-car.
sha256()          -> one digest over every code and item (and the typed cases), pinned in golden/golden_code_sweep.json.
"""
import ctypes as C
import functools
import hashlib
import struct

import numpy as np

import hist_families as hf
import range_worlds as rw
from oracle import oracle as orc

PER_GROUP = 4
BUCKETS = ((1, 1), (2, 16), (17, 128), (129, 256))  # live byte symbols
REQUIRED_MAX_LEN = (1, 2, 5, 6, 8, 9, 10, 11, 12, 13, 16, 17, 24, 32)
MODES = ("typical", "flat", "deep", "tail")
# around the 64-symbol segment, the 128-symbol run of the run record, the 512-symbol run of the seek table, the
# 4096-symbol block; 8191 and the drawn sizes up to 20000 need a second round of 256 x 512 bits in the bodies decoders
EDGE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097, 8191)
N_EDGE, N_DRAWN, DRAWN_MAX = 5, 2, 20000
TAIL_RUN = 70          # the last symbols of a `tail` item, all of the greatest length
DEEP_RUN_ODDS = 24     # a `deep` item starts a new run at one position in this many
BOUND_EXACT_N = 20003  # 4 n + 4 is a multiple of 16: ghf_compress_batch_shared_bound(n) is the body's size to the byte
TYPED_CASES = 40
WIDTHS = (2, 4, 8)
RUN = 128              # symbols per run of a run record
MAGIC = 0x31524247
SEED_POOL, SEED_SIZES, SEED_ITEM, SEED_RANGE, SEED_TYPED, SEED_BASE = 0x5EED0001, 0x5EED1000, 0x5EED2000, 0x5EED3000, 0x5EED4000, 0x5EED5000

# Histograms of the sweep's own, for a required max_len that no "fits" entry of the family gives: (label, int64[257]).
# (hist_families.py is pinned by its digest and stays as it is.)
EXTRA_HISTS = []


def bucket_of(k):
    return next(i for i, (lo, hi) in enumerate(BUCKETS) if lo <= k <= hi)


class Entry:
    def __init__(self, label, hist):
        self.label, self.hist = label, hist
        self.code = orc.build_code(hist)
        self.length = np.array(list(self.code.length), dtype=np.int64)
        self.min_len, self.max_len = int(self.code.min_len), int(self.code.max_len)
        self.variant = rw.decoder_class(self.min_len, self.max_len)[0]
        self.live = np.flatnonzero(self.length[:256]).astype(np.int64)
        self.bucket = bucket_of(int(self.live.size))
        self.group = (self.min_len, self.max_len, self.variant, self.bucket)
        self.header = orc.header_bytes(self.code)
        self.deepest = int(self.live[np.flatnonzero(self.length[self.live] == self.length[self.live].max())[-1]])

    @property
    def first_bit(self):
        return 8 * int(self.header.size)


class Item:
    def __init__(self, entry, name, mode, data):
        self.entry, self.name, self.mode = entry, name, mode
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.data.setflags(write=False)
        self.n = int(self.data.size)
        self.body = orc_body(self.data, entry.code)
        self.ranges = None

    @property
    def image(self):
        return np.concatenate((self.entry.header, self.body))

    @property
    def record(self):
        return orc_record(self.data, self.entry.length)

    @property
    def table(self):
        return rw.expected_table(self.data, self.entry.length, self.entry.first_bit)

    def __repr__(self):
        return "%s :: %s" % (self.entry.label, self.name)


# ---------------------------------------------------------------- expected bytes, all from the oracle
def orc_body(data, code):
    a = np.ascontiguousarray(data, dtype=np.uint8)
    cap = 4 * a.size + 16
    out = np.zeros(cap, dtype=np.uint8)
    n = orc.lib().orc_encode_body(a.ctypes.data, a.size, C.byref(code), out.ctypes.data, cap)
    assert n != C.c_size_t(-1).value
    return out[:n].copy()


def record_of(run_bits, n, magic=MAGIC):
    """the bytes of a run record, as tests/test_gpu_batch_seek.py::record_of: u32 magic, u32 n, u16 run_bits[], zeros up
    to a multiple of 8"""
    raw = struct.pack("<II", magic, n) + np.asarray(run_bits, dtype="<u2").tobytes()
    return np.frombuffer(raw + bytes(-len(raw) % 8), dtype=np.uint8).copy()


def orc_record(data, length):
    bits = np.add.reduceat(np.asarray(length, dtype=np.int64)[data], range(0, data.size, RUN))
    assert bits.size == -(-data.size // RUN) and bits.max() <= 0xFFFF
    return record_of(bits, data.size)


def expected_index(data, length, first_bit):
    """the side-car of `data` coded with `length[]`, its first code at bit `first_bit`: chunk_bit[g] = the first bit of block
    g of 4096 symbols, seg_bit[s] = the end of segment s of 64 symbols counted from its block's first bit (include/ghf.h
    at ghf_index; the end mark belongs to no segment)"""
    n = int(data.size)
    cum = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(length, dtype=np.int64)[data], out=cum[1:])
    nblk, nseg = -(-n // 4096), -(-n // 64)
    chunk_bit = (first_bit + cum[4096 * np.arange(nblk)]).astype(np.uint64)
    seg = np.arange(nseg)
    seg_bit = (cum[np.minimum(64 * (seg + 1), n)] - cum[4096 * (seg // 64)]).astype(np.uint32)
    return chunk_bit, seg_bit


# ---------------------------------------------------------------- the pool
@functools.lru_cache(maxsize=None)
def candidates():
    """-> ([Entry] of every usable histogram, in family order then EXTRA_HISTS; [labels left out])"""
    out, left = [], []
    for label, h, kind in hf.family():
        if kind != "fits":
            continue
        if hf.n_live(h) == 0:
            left.append(label)
            continue
        out.append(Entry(label, h))
    for label, h in EXTRA_HISTS:
        out.append(Entry("sweep/" + label, np.asarray(h, dtype=np.int64)))
    return out, left


def left_out():
    return list(candidates()[1])


def pool(per_group=None):
    return _pool(PER_GROUP if per_group is None else per_group)


@functools.lru_cache(maxsize=None)
def _pool(per_group):
    cand, _ = candidates()
    groups = {}
    for e in cand:
        groups.setdefault(e.group, []).append(e)
    out = []
    for gi, key in enumerate(sorted(groups)):
        members = groups[key]
        order = np.argsort(hf.words(SEED_POOL + gi, len(members)), kind="stable")[:per_group]
        out += [members[int(i)] for i in sorted(order)]
    return out


# ---------------------------------------------------------------- items
def _typical(entry, w):
    wt = (np.int64(1) << (32 - entry.length[entry.live])).astype(np.uint64)  # P ~ 2^-len, in integers
    cum = np.cumsum(wt)
    return entry.live[np.searchsorted(cum, w % cum[-1], side="right")]


def draw(entry, mode, n, seed):
    """n bytes over the live symbols of `entry`, in one of the four modes"""
    w = hf.words(seed, n)
    lens = entry.length[entry.live]
    if mode == "typical":
        d = _typical(entry, w)
    elif mode == "flat":
        d = entry.live[(w % np.uint64(entry.live.size)).astype(np.int64)]
    elif mode == "deep":  # only symbols of the two greatest lengths, in runs
        deep = entry.live[lens >= np.unique(lens)[-2:].min()]
        starts = ((w >> np.uint64(40)) % np.uint64(DEEP_RUN_ODDS)) == 0
        starts[0] = True
        at = np.maximum.accumulate(np.where(starts, np.arange(n), 0))
        d = deep[(w[at] % np.uint64(deep.size)).astype(np.int64)]
    elif mode == "tail":  # a last segment and the end mark at the greatest width
        d = _typical(entry, w)
        d[-TAIL_RUN:] = entry.deepest
    else:
        raise ValueError(mode)
    return d.astype(np.uint8)


def sizes_for(ci):
    w = hf.words(SEED_SIZES + 16 * ci, len(EDGE_SIZES) + N_DRAWN)
    edge = [EDGE_SIZES[int(i)] for i in np.argsort(w[: len(EDGE_SIZES)], kind="stable")[:N_EDGE]]
    return edge + [1 + int(x % np.uint64(DRAWN_MAX)) for x in w[len(EDGE_SIZES) :]]


def ranges_for(n, seed):
    """three (first, count): a drawn one, one of count 1, and one that starts and ends on a 4096 boundary where n allows"""
    a, b, c = (int(x) for x in hf.words(seed, 3))
    first = a % n
    out = [(first, 1 + b % (n - first)), (c % n, 1)]
    blocks = n // 4096
    if blocks >= 2:
        f = 1 + c % (blocks - 1)
        out.append((4096 * f, 4096 * (1 + b % (blocks - f))))
    elif blocks == 1:
        out.append((0, 4096))
    else:
        out.append((0, n))
    for f, k in out:
        assert 0 <= f and 1 <= k and f + k <= n
    return out


@functools.lru_cache(maxsize=None)
def _items(per_group):
    out = {}
    for ci, e in enumerate(pool(per_group)):
        its = []
        for j, n in enumerate(sizes_for(ci)):
            mode = MODES[(ci + j) % 4]
            its.append(Item(e, "%s/%d" % (mode, n), mode, draw(e, mode, n, SEED_ITEM + 64 * ci + j)))
        if e.max_len == 32:
            its.append(Item(e, "deepest/%d" % BOUND_EXACT_N, "deepest", np.full(BOUND_EXACT_N, e.deepest, dtype=np.uint8)))
        for j, it in enumerate(its):
            it.ranges = ranges_for(it.n, SEED_RANGE + 64 * ci + j)
        out[e.label] = its
    return out


def items(entry, per_group=None):
    return _items(PER_GROUP if per_group is None else per_group)[entry.label]


# ---------------------------------------------------------------- typed cases
class Typed:
    def __init__(self, name, e, n, entries, planes, base, ranges):
        self.name, self.e, self.n, self.entries, self.planes, self.ranges = name, e, n, entries, planes, ranges
        self.tensor = np.stack(planes, axis=1).reshape(-1)  # byte p of element k = planes[p][k]
        self.base = base
        self.new = base ^ self.tensor                        # what the delta forms are given: new ^ base = tensor
        for a in (self.tensor, self.base, self.new):
            a.setflags(write=False)
        self.bodies = [orc_body(pl, en.code) for pl, en in zip(planes, entries)]
        self.variants = tuple(en.variant for en in entries)

    def image(self, p):
        return np.concatenate((self.entries[p].header, self.bodies[p]))

    def table(self, p):
        return rw.expected_table(self.planes[p], self.entries[p].length, self.entries[p].first_bit)

    def record(self, p):
        return orc_record(self.planes[p], self.entries[p].length)

    def __repr__(self):
        return "%s :: %s" % (self.name, " | ".join(en.label for en in self.entries))


def typed_cases(e, per_group=None):
    """TYPED_CASES tensors of e-byte elements; plane p's bytes come from a pool code of decoder class (k + p) % 6, so the
    planes of one tensor run different hot loops (at e = 8 the six classes, two of them twice)"""
    return _typed_cases(e, PER_GROUP if per_group is None else per_group)


@functools.lru_cache(maxsize=None)
def _typed_cases(e, per_group):
    by_class = {}
    for en in pool(per_group):
        by_class.setdefault(en.variant, []).append(en)
    sizes = list(EDGE_SIZES)
    out = []
    for k in range(TYPED_CASES):
        w = hf.words(SEED_TYPED + 4096 * e + 64 * k, 2 * e + 2)
        n = sizes[k] if k < len(sizes) else 1 + int(w[2 * e] % np.uint64(DRAWN_MAX))
        entries, planes = [], []
        for p in range(e):
            cls = by_class[(k + p) % 6]
            en = cls[int(w[2 * p] % np.uint64(len(cls)))]
            mode = MODES[int(w[2 * p + 1] % np.uint64(4))]
            entries.append(en)
            planes.append(draw(en, mode, n, SEED_TYPED + 4096 * e + 64 * k + 8 + p))
        base = hf.words(SEED_BASE + 4096 * e + k, -(-n * e // 8)).view(np.uint8)[: n * e].copy()
        out.append(Typed("E%d/case%02d/n%d" % (e, k, n), e, n, entries, planes, base, ranges_for(n, SEED_RANGE + 0x100000 * e + k)))
    return out


# ---------------------------------------------------------------- the digest
def sha256():
    m = hashlib.sha256()
    for e in pool():
        m.update(e.label.encode())
        m.update(e.length.astype("<i8").tobytes())
        m.update(e.header.tobytes())
        for it in items(e):
            m.update(it.name.encode())
            m.update(it.data.tobytes())
            m.update(np.asarray(it.ranges, dtype="<i8").tobytes())
    for w in WIDTHS:
        for t in typed_cases(w):
            m.update(repr(t).encode())
            m.update(t.tensor.tobytes())
            m.update(t.base.tobytes())
            m.update(np.asarray(t.ranges, dtype="<i8").tobytes())
    return m.hexdigest()
