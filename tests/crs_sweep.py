"""Every tree shape for the kernels that take a caller's .crs tree (numpy and the oracle only; no GPU, no numpy RNG: every
choice comes from datagen.splitmix64 through hist_families.words, so the cases can never change).

A kernel that is handed a tree only needs data over that tree's leaves, so a code of 64 bits is driven here by items of a
few hundred bytes where a data-derived one needs 2^44.  The trees:

  reference-built   orc.crs_tree(h[:256]) for the entries of hist_families.family() / crs_extras() and for EXTRA_HISTS (the
                    sweep's own Fibonacci counts: every depth 33..64 then has a reference-built tree) with at least two
                    live byte values and a depth of at most 64; grouped by depth, PER_GROUP drawn from every depth up to
                    32, every deeper one taken
  mirrors           of every drawn reference-built tree: the children swapped at every parent, the codes complemented.  A
                    valid .crs that DecodeHuffTree reads and that no encoder run writes ("left is the lighter child" no
                    longer holds)
  hand-built        right and left combs at COMB_DEPTHS, balanced trees of 2 .. 256 leaves (fixed length 1..8: these never
                    self-synchronise), and balanced trees of 2^j leaves with one leaf replaced by a comb down to depth D
                    (HYBRIDS); the keys are permuted by splitmix64, so leaf order is not key order

pool()        -> [Tree]: label, kind ("ref" / "mirror" / "hand"), codes[256] ('0'/'1' strings, '' = absent), length[256],
                 value[256] (the code as a Python int), live, min_len, max_len, header (the preorder bytes), left[] / right[]
                 / root / n_leaves in the numbering of ghf_tree (256 + i = the i-th parent in preorder), leftmost / rightmost
                 (the keys of the all-zeros and the all-ones leaf), deepest_ones / deepest_zeros
left_out()    -> the labels of the trees deeper than 64
items(tree)   -> [Item]: name, mode, data (uint8); body (MSB first, zero-filled), total_bits, left_bits, file
                 ([tree][left_bits][last byte][whole body bytes]), decoder_input (the stored last byte appended), index()
                 (the side-car, first bit 8 * (tree_bytes + 2)), pieces(own) ([(lo, hi, first, end_bit, landing, n_symbols)]),
                 cuts() (the piece sizes it is cut at)
flipped_bit(item) / wrong_left_bits(item): damage whose effect the plain decoder below proves
sha256()      -> one digest over every tree and item, pinned in golden/golden_crs_sweep.json.
"""
import functools
import hashlib
from math import gcd

import numpy as np

import code_sweep as cs
import hist_families as hf
from oracle import oracle as orc

PER_GROUP = 2
MAX_DEPTH = 64
MODES = ("typical", "flat", "deep", "tail")
EDGE_SIZES = cs.EDGE_SIZES
N_EDGE, N_DRAWN, DRAWN_MAX = 5, 2, 20000
TAIL_RUN = 70           # the last symbols of a `tail` item, all of the greatest length
DEEP_RUN_ODDS = 24      # a `deep` item starts a new run at one position in this many
ENDS_MAX = 200          # symbols of an `ends` item at the most
ENDS_PREFIX = 150       # of which drawn; the rest steers the total to the wanted left_bits
BLOCK_N = 4097          # symbols of a `block` item: one more than a block of the side-car
SUB_BITS = 512          # K6's subsequence
RUN_SUBS = 96           # a run0 / run1 item's run covers this many subsequences (>= 80: beyond kScanAfterFew = 64 passes)
PIECE_SIZES = (64, 1000, 4096)  # own bytes of a piece
PIECES_PER_ID = 5000  # a depth's pieces go into ceil(pieces / this) ids: every piece is a host round trip of about half a millisecond
RUN_PREFIX = 5          # drawn symbols in front of the run (then one more where the bit count has to become odd)
COMB_DEPTHS = (1, 2, 8, 9, 10, 11, 12, 13, 16, 17, 32, 33, 63, 64)
RUN_COMBS = (16, 32, 64)  # the combs that carry the run items: one depth per stride of K6's function rows (16 / 32 / 64)
HYBRIDS = ((7, 13), (7, 17), (7, 33), (4, 64))
SEED_POOL, SEED_SIZES, SEED_ITEM, SEED_ENDS, SEED_RUN, SEED_BLOCK, SEED_KEYS = (
    0xC5EED001, 0xC5EED100, 0xC5EE2000, 0xC5EE3000, 0xC5EE4000, 0xC5EE5000, 0xC5EE6000)

# Histograms of the sweep's own: Fibonacci counts (below 2^55 in total) at k = depth + 1 live byte values, placed "drawn"
# or "reversed", never "first" as the family's are.  (label, int64[256])
EXTRA_HISTS = [("fib/k%d/%s" % (d + 1, pl), hf.place(hf.fib(d + 1), pl, 7000 + d)[:256].copy())
               for d in range(33, 65) for pl in (hf.PLACEMENTS[1 + d % 2],)]


class Tree:
    def __init__(self, label, kind, codes):
        self.label, self.kind = label, kind
        self.codes = list(codes)
        assert len(self.codes) == 256
        self.length = np.array([len(c) for c in self.codes], dtype=np.int64)
        self.value = [int(c, 2) if c else 0 for c in self.codes]
        self.live = np.flatnonzero(self.length).astype(np.int64)
        lens = self.length[self.live]
        self.min_len, self.max_len = int(lens.min()), int(lens.max())
        self.n_leaves = int(self.live.size)
        self._walk()
        self.tree_bytes = int(self.header.size)
        self.first_bit = 8 * (self.tree_bytes + 2)
        self.deepest = int(self.live[np.flatnonzero(lens == lens.max())[-1]])
        ends = {c: k for k, c in enumerate(self.codes) if c}
        self.deepest_ones = "1" * self.max_len in ends
        self.deepest_zeros = "0" * self.max_len in ends
        # the bits of every code, one row per key, for the packer
        self.bits = np.zeros((256, self.max_len), dtype=np.uint8)
        for k in self.live.tolist():
            self.bits[k, : self.length[k]] = np.frombuffer(self.codes[k].encode(), dtype=np.uint8) - 48

    def _walk(self):
        """the preorder header and ghf_tree's arrays from the code strings; asserts that they are a complete prefix code"""
        by_code = {c: k for k, c in enumerate(self.codes) if c}
        assert len(by_code) == self.n_leaves >= 2
        hdr, left, right = [], [0] * 256, [0] * 256
        n_parents = 0
        order = []
        stack = [("", None, 0)]  # (path, parent index, side)
        while stack:
            path, parent, side = stack.pop()
            if path in by_code:
                node = by_code[path]
                hdr += [0, node]
                order.append(node)
            else:
                assert len(path) < self.max_len, (self.label, "not a complete prefix code at", path)
                node = 256 + n_parents
                n_parents += 1
                hdr += [255, 255]
                stack.append((path + "1", node - 256, 1))
                stack.append((path + "0", node - 256, 0))
            if parent is not None:
                (right if side else left)[parent] = node
        assert n_parents == self.n_leaves - 1 and len(order) == self.n_leaves
        self.header = np.array(hdr, dtype=np.uint8)
        self.left, self.right, self.root = left, right, 256
        self.leftmost, self.rightmost = order[0], order[-1]

    def __repr__(self):
        return self.label


def mirror(t):
    flip = str.maketrans("01", "10")
    return Tree(t.label + "~mirror", "mirror", [c.translate(flip) for c in t.codes])


# ---------------------------------------------------------------- reference-built trees
@functools.lru_cache(maxsize=None)
def candidates():
    """-> ([Tree] of every usable histogram: family order, crs_extras, EXTRA_HISTS; [labels deeper than MAX_DEPTH])"""
    hists = [(label, h[:256]) for label, h, _ in hf.family()]
    hists += [(label, h) for label, h, expect in hf.crs_extras()]
    hists += [("sweep/" + label, h) for label, h in EXTRA_HISTS]
    out, left = [], []
    for label, h in hists:
        if int(np.count_nonzero(h)) < 2:
            continue
        codes = orc.crs_code_strings(orc.crs_tree(h))
        if max(len(c) for c in codes) > MAX_DEPTH:
            left.append(label)
            continue
        out.append(Tree(label, "ref", codes))
    return out, left


def left_out():
    return list(candidates()[1])


def drawn():
    """the reference-built trees of the pool: PER_GROUP of every depth up to 32, every deeper one"""
    groups = {}
    for t in candidates()[0]:
        groups.setdefault(t.max_len, []).append(t)
    out = []
    for d in sorted(groups):
        members = groups[d]
        if d <= 32:
            order = np.argsort(hf.words(SEED_POOL + d, len(members)), kind="stable")[:PER_GROUP]
            members = [members[int(i)] for i in sorted(order)]
        out += members
    return out


# ---------------------------------------------------------------- hand-built trees
def _keys(n, seed):
    """n distinct byte values in a drawn order"""
    return [int(k) for k in np.argsort(hf.words(SEED_KEYS + seed, 256), kind="stable")[:n]]


def _from_leaves(label, leaf_codes, seed):
    codes = [""] * 256
    for k, c in zip(_keys(len(leaf_codes), seed), leaf_codes):
        codes[k] = c
    return Tree(label, "hand", codes)


def comb_codes(prefix, depth, bit):
    """a comb below `prefix` down to `depth` more levels: `bit` leads on, the other bit ends in a leaf"""
    other = "10"[int(bit)]
    return [prefix + bit * i + other for i in range(depth)] + [prefix + bit * depth]


def hand_built():
    out = []
    for d in COMB_DEPTHS:
        out.append(_from_leaves("hand/comb-right/d%d" % d, comb_codes("", d, "1"), 10 * d))
        out.append(_from_leaves("hand/comb-left/d%d" % d, comb_codes("", d, "0"), 10 * d + 1))
    for j in range(1, 9):
        out.append(_from_leaves("hand/balanced/%d" % (1 << j), [format(i, "0%db" % j) for i in range(1 << j)], 1000 + j))
    for n, (j, d) in enumerate(HYBRIDS):
        at = int(hf.words(SEED_KEYS + 2000 + n, 1)[0] % np.uint64(1 << j))
        leaves = []
        for i in range(1 << j):
            c = format(i, "0%db" % j)
            leaves += comb_codes(c, d - j, "10"[n % 2]) if i == at else [c]
        out.append(_from_leaves("hand/balanced%d+comb/d%d" % (1 << j, d), leaves, 2000 + n))
    return out


@functools.lru_cache(maxsize=None)
def pool():
    ref = drawn()
    out = ref + [mirror(t) for t in ref] + hand_built()
    assert len({t.label for t in out}) == len(out)
    return out


def groups():
    """the depths of the pool, ascending: the ids of tests/test_gpu_crs_sweep.py"""
    return sorted({t.max_len for t in pool()})


def trees_of(max_len):
    return [t for t in pool() if t.max_len == max_len]


def piece_parts(max_len):
    """into how many ids the pieces of this depth are split"""
    return max(1, -(-sum(it.n_pieces() for t in trees_of(max_len) for it in items(t)) // PIECES_PER_ID))


def piece_part(max_len, k):
    """[(tree, [Item])]: part k of that depth's items, every piece_parts(max_len)-th (tree, item) pair from the k-th on"""
    pairs = [(t, it) for t in trees_of(max_len) for it in items(t)][k :: piece_parts(max_len)]
    return [(t, [it for u, it in pairs if u is t]) for t in trees_of(max_len) if any(u is t for u, _ in pairs)]


# ---------------------------------------------------------------- expected bytes
def pack(tree, data):
    """-> (body bytes MSB first and zero-filled, total bits): every symbol's code string behind the one before"""
    data = np.asarray(data, dtype=np.int64)
    lens = tree.length[data]
    assert lens.min() > 0
    cum = np.zeros(data.size + 1, dtype=np.int64)
    np.cumsum(lens, out=cum[1:])
    total = int(cum[-1])
    sym = np.repeat(np.arange(data.size), lens)
    off = np.arange(total) - cum[sym]
    return np.packbits(tree.bits[data[sym], off]), total


class Item:
    def __init__(self, tree, name, mode, data):
        self.tree, self.name, self.mode = tree, name, mode
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.data.setflags(write=False)
        self.n = int(self.data.size)
        assert self.n >= 1
        self.cum = np.zeros(self.n + 1, dtype=np.int64)  # cum[i] = the first bit of symbol i's code, from the body's start
        np.cumsum(tree.length[self.data], out=self.cum[1:])
        self.total_bits = int(self.cum[-1])
        self.left_bits = -self.total_bits % 8

    @functools.cached_property
    def body(self):
        b, total = pack(self.tree, self.data)
        assert total == self.total_bits and b.size == -(-total // 8)
        return b

    @property
    def whole(self):
        """the body's whole bytes: what the file stores behind the two prefix bytes"""
        return self.body[: self.total_bits // 8]

    @property
    def file(self):
        last = int(self.body[-1]) if self.left_bits else 0
        return np.concatenate((self.tree.header, np.array([self.left_bits, last], dtype=np.uint8), self.whole))

    @property
    def decoder_input(self):
        """what ghf_crs_decode takes: the file, with the stored last byte appended when left_bits != 0"""
        f = self.file
        return np.concatenate((f, f[self.tree.tree_bytes + 1 : self.tree.tree_bytes + 2])) if self.left_bits else f

    def index(self):
        return cs.expected_index(self.data, self.tree.length, self.tree.first_bit)

    def pieces(self, own):
        """the whole body bytes cut every `own` bytes, the last piece with the stored last byte behind it: [(lo, hi, first,
        end_bit, landing, n_symbols)] in the terms of ghf_crs_sync_piece -- first / end_bit / landing count from bit 8 * lo
        resp. 8 * hi, n_symbols = the codes that start in the piece"""
        nbytes = self.total_bits // 8
        out, first = [], 0
        npieces = -(-nbytes // own)
        starts = self.cum[:-1]
        for k in range(npieces):
            lo, hi = k * own, min(nbytes, (k + 1) * own)
            last = k == npieces - 1
            end = self.total_bits if last else 8 * hi
            a, b = np.searchsorted(starts, [8 * lo + first, end], side="left")
            landing = 0 if last else int(self.cum[b]) - 8 * hi
            out.append((lo, hi, first, end - 8 * lo, landing, int(b - a)))
            first = landing
        assert sum(p[5] for p in out) == (self.n if npieces else 0)
        return out

    def cuts(self):
        """the piece sizes this item is cut at: every one of PIECE_SIZES (none for an item without a whole body byte)"""
        return list(PIECE_SIZES) if self.total_bits >= 8 else []

    def n_pieces(self):
        return sum(-(-(self.total_bits // 8) // own) for own in self.cuts())

    def __repr__(self):
        return "%s :: %s" % (self.tree.label, self.name)


# ---------------------------------------------------------------- items
def _typical(tree, w):
    """P ~ 2^-len: in doubles, whose sums of powers of two are exact here or rounded the same way everywhere"""
    cum = np.cumsum(np.ldexp(1.0, -tree.length[tree.live]))
    u = (w >> np.uint64(11)).astype(np.float64) * (cum[-1] / float(1 << 53))
    return tree.live[np.minimum(np.searchsorted(cum, u, side="right"), tree.live.size - 1)]


def draw(tree, mode, n, seed):
    w = hf.words(seed, n)
    lens = tree.length[tree.live]
    if mode == "typical":
        d = _typical(tree, w)
    elif mode == "flat":
        d = tree.live[(w % np.uint64(tree.live.size)).astype(np.int64)]
    elif mode == "deep":  # only leaves of the two greatest depths, in runs
        deep = tree.live[lens >= np.unique(lens)[-2:].min()]
        starts = ((w >> np.uint64(40)) % np.uint64(DEEP_RUN_ODDS)) == 0
        starts[0] = True
        at = np.maximum.accumulate(np.where(starts, np.arange(n), 0))
        d = deep[(w[at] % np.uint64(deep.size)).astype(np.int64)]
    elif mode == "tail":
        d = _typical(tree, w)
        d[-TAIL_RUN:] = tree.deepest
    else:
        raise ValueError(mode)
    return d.astype(np.uint8)


def sizes_for(ti):
    w = hf.words(SEED_SIZES + 16 * ti, len(EDGE_SIZES) + N_DRAWN)
    edge = [EDGE_SIZES[int(i)] for i in np.argsort(w[: len(EDGE_SIZES)], kind="stable")[:N_EDGE]]
    return edge + [1 + int(x % np.uint64(DRAWN_MAX)) for x in w[len(EDGE_SIZES) :]]


def reachable_left_bits(tree):
    """the values left_bits can take under this tree: the multiples of gcd(8, every length) below 8"""
    g = 8
    for l in np.unique(tree.length[tree.live]).tolist():
        g = gcd(g, int(l))
    return list(range(0, 8, g))


def _steer(tree, have, want):
    """the shortest list of keys whose lengths take a bit count of `have` (mod 8) to `want` (mod 8); ties go to the first
    key of that length"""
    by_len = {}
    for k in tree.live.tolist():
        by_len.setdefault(int(tree.length[k]) % 8, k)
    paths, frontier = {have % 8: []}, [have % 8]
    while frontier and want % 8 not in paths:
        nxt = []
        for r in frontier:
            for step in sorted(by_len):
                q = (r + step) % 8
                if q not in paths:
                    paths[q] = paths[r] + [by_len[step]]
                    nxt.append(q)
        frontier = nxt
    return paths[want % 8]


def ends_items(tree, ti):
    out = []
    for r in reachable_left_bits(tree):
        w = hf.words(SEED_ENDS + 64 * ti + r, ENDS_PREFIX + 1)
        m = 1 + int(w[ENDS_PREFIX] % np.uint64(ENDS_PREFIX))
        d = tree.live[(w[:m] % np.uint64(tree.live.size)).astype(np.int64)].tolist()
        d += _steer(tree, int(tree.length[d].sum()), -r)
        assert len(d) <= ENDS_MAX
        it = Item(tree, "ends/left%d/%d" % (r, len(d)), "ends", np.array(d, dtype=np.uint8))
        assert it.left_bits == r
        out.append(it)
    return out


def run_item(tree, ti, which):
    """a few drawn symbols, an odd number of bits, then a run of the leftmost (run0) or rightmost (run1) leaf over RUN_SUBS
    subsequences.  The leaf's length divides 512 and is even, so no subsequence starts on a boundary of the run by itself:
    every shifted parse of the run is valid, and the true boundary travels one subsequence per pass."""
    key = tree.leftmost if which == 0 else tree.rightmost
    k = int(tree.length[key])
    assert k % 2 == 0 and SUB_BITS % k == 0, (tree.label, k)
    w = hf.words(SEED_RUN + 64 * ti + which, RUN_PREFIX)
    d = tree.live[(w % np.uint64(tree.live.size)).astype(np.int64)].tolist()
    if int(tree.length[d].sum()) % 2 == 0:
        d.append(next(x for x in tree.live.tolist() if tree.length[x] % 2 == 1))
    assert int(tree.length[d].sum()) % 2 == 1
    d += [key] * (RUN_SUBS * SUB_BITS // k)
    return Item(tree, "run%d/%d" % (which, len(d)), "run%d" % which, np.array(d, dtype=np.uint8))


def block_item(tree, ti):
    long_keys = tree.live[tree.length[tree.live] >= 33]
    w = hf.words(SEED_BLOCK + 64 * ti, BLOCK_N)
    return Item(tree, "block/%d" % BLOCK_N, "block", long_keys[(w % np.uint64(long_keys.size)).astype(np.int64)])


def _is_run_comb(tree):
    return tree.kind == "hand" and tree.label.startswith("hand/comb-") and tree.max_len in RUN_COMBS


@functools.lru_cache(maxsize=None)
def _items(ti):
    t = pool()[ti]
    its = []
    for j, n in enumerate(sizes_for(ti)):
        mode = MODES[(ti + j) % 4]
        its.append(Item(t, "%s/%d" % (mode, n), mode, draw(t, mode, n, SEED_ITEM + 64 * ti + j)))
    its += ends_items(t, ti)
    if _is_run_comb(t):
        its.append(run_item(t, ti, 1 if "right" in t.label else 0))
    if t.max_len >= 33:
        its.append(block_item(t, ti))
    return its


def items(tree):
    return _items(pool().index(tree))


def run_items():
    """[(stride of K6's function rows, Item)]: the slow-settling items, two per stride"""
    out = []
    for t in pool():
        if _is_run_comb(t):
            out += [({16: 16, 32: 32, 64: 64}[t.max_len], it) for it in items(t) if it.mode.startswith("run")]
    return out


# ---------------------------------------------------------------- a plain decoder, for the cases that damage a stream
def decode_bits(tree, bits, start, end, limit=None):
    """walks `bits` (an array of 0 / 1) from bit `start` -> (keys, the bit behind the last whole code, whether the walk
    stopped inside a code): codes are taken while they start in front of `end` and lie wholly in `bits`"""
    by_code = {c: k for k, c in enumerate(tree.codes) if c}
    out, pos = [], start
    while pos < end and (limit is None or len(out) < limit):
        path, p = "", pos
        while path not in by_code:
            if p >= bits.size:
                return out, pos, True
            path += "01"[bits[p]]
            p += 1
        out.append(by_code[path])
        pos = p
    return out, pos, False


def flipped_bit(item, seed):
    """-> a body bit in segment 0 (the first 64 symbols; the item has more than 128) whose flip provably moves the segment's
    end: 64 codes walked from the segment's first bit over the damaged bits end elsewhere than the side-car says"""
    assert item.n > 128
    bits = np.unpackbits(item.body)[: item.total_bits].copy()
    want = int(item.cum[64])
    for w in hf.words(seed, 64).tolist():
        at = int(w % want)
        bits[at] ^= 1
        keys, pos, cut = decode_bits(item.tree, bits, 0, item.total_bits, limit=64)
        bits[at] ^= 1
        if not cut and len(keys) == 64 and pos != want:
            return at
    raise AssertionError("no flip of %r moves its first segment's end" % item)


def wrong_left_bits(item):
    """-> the values of left_bits, one off the true one, under which the stream provably does not end on a code boundary: one
    more cuts the last code (if that has two bits or more), one less appends a zero bit that is no whole code (if the leftmost
    leaf has two bits or more)"""
    t, out = item.tree, []
    bits = np.concatenate((np.unpackbits(item.body)[: item.total_bits], np.zeros(8, dtype=np.uint8)))
    for left in (item.left_bits + 1, item.left_bits - 1):
        end = item.total_bits + item.left_bits - left
        if 0 <= left <= 7 and decode_bits(t, bits[:end], 0, end)[2]:
            out.append(left)
    return out


# ---------------------------------------------------------------- the digest
def sha256():
    m = hashlib.sha256()
    for t in pool():
        m.update(t.label.encode())
        m.update(t.length.astype("<i8").tobytes())
        m.update(t.header.tobytes())
        for it in items(t):
            m.update(it.name.encode())
            m.update(it.data.tobytes())
    return m.hexdigest()
