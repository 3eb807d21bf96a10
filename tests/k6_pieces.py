"""K6 (ghf_sync.hip behind ghf_sync_piece / ghf_decoded_size / ghf_decode(index = NULL)) on canonical codes: the cases and
a model of the ghf_sync_piece contract (numpy and the oracle only; no GPU, no library, no numpy RNG: every choice comes from
datagen.splitmix64 through hist_families.words, as in code_sweep.py).

The model, in the words of include/ghf.h: a piece is the body bytes [lo, hi) with its look-ahead (zeros behind the body's
end); it is decoded from bit 8 * lo + first_bit, ANY first_bit < 512; n_symbols = the codes that start in
[first_bit, end_bit = 8 * (hi - lo)), up to the first end mark met; landing = the bits the last of them runs past end_bit;
where the parse meets an end mark the contract defines no next piece and landing is None.  The code is complete, so every
bit pattern decodes: parse_table() gives, for every bit of a body, the length of the code that would start there -- one
bit at a time, all positions side by side -- and whether that code is the end mark; Stream.sync() walks it.

codes()        -> [ShapeCode] x 8 in six shapes, by rule from code_sweep.pool(): one shape per path of K6's prologue, its
                  class walk and the stride rule (SHAPES; k6_mode / cls / stride are recomputed here from the lengths)
tier_a(code)   -> [Chain] x 4: the `typical` and the `deep` stream cut at own sizes that put end_bit on K6's seams, every
                  first_bit the previous landing; in both look-ahead layouts
tier_b(code)   -> [Piece]: byte cuts of one stream whose true first_bit takes every value 0 .. max_len - 1
tier_c(code)   -> [Guess]: wrong first_bits on pieces of 1, 2, 64, 65 and 96 subsequences, on drawn bytes and (cls8, cls4,
                  the (7,8) code) on a run of one symbol on which a wrong parse never falls into step
tier_d(code)   -> [Marked]: streams whose end mark starts at every bit around a subsequence edge and around the edge of a
                  group of 64 subsequences, and ends exactly on end_bit
tier_e(code)   -> [Image]: .crs2 images of 1, 2, 63, 64, 65, 4095, 4096, 4097 subsequences
sha256()       -> one digest over every expected triple and every image, pinned in golden/golden_k6_pieces.json
"""
import functools
import hashlib
from collections import namedtuple

import numpy as np

import code_sweep as cs
import hist_families as hf
import shard_model as sm

SUB_BITS, SUB_BYTES, GROUP = 512, 64, 64
SHAPES = ("cls8", "cls4", "two", "direct", "long16", "long32")
FILLS = ("typical", "deep")
A_OWN = (0, 8, 63, 64, 65, 4095, 4096, 4097)  # the empty piece comes first: first_bit <= end_bit makes its first_bit 0
A_BIG = (262080, 262144, 262208)              # 4096 subsequences and +- 64 bytes: once per code, on the `typical` stream
A_TAIL = 700                                  # bytes, about, behind the last fixed cut
LAYOUTS = ("plus16", "plus8")                 # own + 16 rounded to 16 in a zeroed buffer | own + 8 exactly, 0xFF behind
B_OWN = 161                                   # own bytes of a tier-B piece: two subsequences and 33 bytes
C_SUBS = (1, 2, 64, 65, 96)                   # 96: beyond kScanAfterFew = 64 passes
C_MAX_GUESSES = 24
C_LO = 5                                      # the byte at which the pieces of the drawn stream begin
D_SUB_EDGE, D_GROUP_EDGE = 3 * SUB_BITS, GROUP * SUB_BITS
E_NSUB = (1, 2, 63, 64, 65, 4095, 4096, 4097)
STALE = 4096                                  # stale 0xFF bytes behind the end mark, inside stream_bytes
SEED = 0x6B5EED000000
N_CASES = 1856  # pieces of tiers A (both layouts) and B, guesses of tier C, streams of tier D, images of tier E; see census()

Triple = namedtuple("Triple", "landing n_symbols has_end_mark")


def census_of(lengths):
    """{length: codes} of the 257 lengths"""
    ll = np.asarray(lengths)
    return {int(l): int(np.count_nonzero(ll == l)) for l in np.unique(ll[ll > 0])}


def k6_mode_of(lengths):
    """GHF_K6_PROLOGUE: 2 = at most two neighbouring lengths, 1 = the direct table resolves every code, 0 = table + miss path"""
    c = census_of(lengths)
    lo, hi = min(c), max(c)
    return 2 if hi - lo <= 1 and hi <= 31 else 1 if hi <= 12 else 0


def cls_of(lengths):
    """k6_cls: L = 8 or 4 when the code is 2^L - 1 codes of L bits and two of L + 1, the end mark one of the two; else 0"""
    c = census_of(lengths)
    for L in (8, 4):
        if c == {L: (1 << L) - 1, L + 1: 2} and int(lengths[256]) == L + 1:
            return L
    return 0


def stride_of(max_len):
    """settle_boundaries: the bytes of a function row of the scan (codes up to 32 bits)"""
    return 16 if max_len <= 16 else 32


class ShapeCode:
    def __init__(self, shape, entry, ci):
        self.shape, self.entry, self.ci = shape, entry, ci
        self.label = "%s/%d-%d" % (shape, entry.min_len, entry.max_len)
        self.t = sm.tables(entry.code)
        self.length = entry.length
        self.min_len, self.max_len = entry.min_len, entry.max_len
        self.live = entry.live
        self.mode, self.cls, self.stride = k6_mode_of(self.length), cls_of(self.length), stride_of(self.max_len)
        self.eof_len, self.eof_cw = int(self.length[256]), int(self.t.codes[256])
        self.by_len = {}  # length -> the codewords of that length (the end mark's among them)
        for s in range(257):
            if self.length[s]:
                self.by_len.setdefault(int(self.length[s]), []).append(int(self.t.codes[s]))

    def __repr__(self):
        return self.label


def _both_lengths(e):
    return np.unique(e.length[e.live]).size == 2


@functools.lru_cache(maxsize=None)
def codes():
    """By rule from code_sweep.pool() (the first of equals wins; the pool's order is pinned by its digest):
    cls8 / cls4: the first entry of that class; two: the first (7,8) entry that is no class and the first (1,2) entry, both
    with byte symbols of either length; direct: three or more lengths and max_len <= 12, the greatest (max_len, live symbols);
    long16: 13 <= max_len <= 16, likewise; long32: likewise among 17 <= max_len <= 31, and the max_len == 32 entry with the
    most live symbols."""
    pool = cs.pool()
    big = lambda es: max(es, key=lambda e: (e.max_len, e.live.size))
    picked = [("cls8", next(e for e in pool if cls_of(e.length) == 8)), ("cls4", next(e for e in pool if cls_of(e.length) == 4))]
    for shape in ((7, 8), (1, 2)):
        picked.append(("two", next(e for e in pool if (e.min_len, e.max_len) == shape and not cls_of(e.length) and _both_lengths(e))))
    picked.append(("direct", big(e for e in pool if e.max_len <= 12 and len(census_of(e.length)) >= 3)))
    picked.append(("long16", big(e for e in pool if 13 <= e.max_len <= 16)))
    picked.append(("long32", big(e for e in pool if 17 <= e.max_len <= 31)))
    picked.append(("long32", big(e for e in pool if e.max_len == 32)))
    return tuple(ShapeCode(shape, e, ci) for ci, (shape, e) in enumerate(picked))


def by_label(label):
    return next(c for c in codes() if c.label == label)


# ---------------------------------------------------------------------------------------------------------- the model
def windows(buf):
    """for every bit p of buf (its last 8 bytes excepted): the 32 bits from p on, as uint64"""
    b = np.asarray(buf, dtype=np.uint8).astype(np.uint64)
    n = b.size - 8
    w = np.zeros(n, dtype=np.uint64)
    for k in range(5):
        w |= b[k : k + n] << np.uint64(32 - 8 * k)
    out = np.empty((n, 8), dtype=np.uint64)
    for j in range(8):
        out[:, j] = (w >> np.uint64(8 - j)) & np.uint64(0xFFFFFFFF)
    return out.reshape(-1)


def parse_table(code, buf):
    """(length of the code that starts at every bit of buf, whether it is the end mark), as bytes objects: bit by bit, a
    position takes the first length at which the bits read so far are a codeword (a prefix code: no other can follow)"""
    W = windows(buf)
    L = np.zeros(W.size, dtype=np.uint8)
    idx = np.arange(W.size)
    for l in range(1, code.max_len + 1):
        if l not in code.by_len:
            continue
        v = W[idx] >> np.uint64(32 - l)
        hit = np.isin(v, np.array(code.by_len[l], dtype=np.uint64))
        L[idx[hit]] = l
        idx = idx[~hit]
    assert idx.size == 0, "the code is complete: every bit pattern decodes"
    E = (L == code.eof_len) & ((W >> np.uint64(32 - code.eof_len)) == np.uint64(code.eof_cw))
    return L.tobytes(), E.astype(np.uint8).tobytes()


MUTANTS = ("counts_a_code_at_end_bit", "drops_the_last_code", "ignores_first_bit")


def walk(table, pos, end, mutant=None, trace=None):
    """codes that start in [pos, end) -> Triple, landing relative to `end`"""
    L, E = table
    if mutant == "counts_a_code_at_end_bit":
        end += 1
    n = 0
    start = pos
    while pos < end:
        if E[pos]:
            return Triple(None, n, 1)
        if trace is not None:
            trace.append(pos)
        start = pos
        pos += L[pos]
        n += 1
    if mutant == "counts_a_code_at_end_bit":
        end -= 1
    if mutant == "drops_the_last_code" and n:
        pos, n = start, n - 1
    return Triple(pos - end, n, 0)


class Stream:
    """data under a code: the body is the oracle's (orc_encode_body: codes, end mark, 1 bits up to a byte)"""

    def __init__(self, code, name, data):
        self.code, self.name = code, name
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.data.setflags(write=False)
        self.n = int(self.data.size)
        self.body = cs.orc_body(self.data, code.entry.code)
        self.cum = np.zeros(self.n + 1, dtype=np.int64)  # cum[i] = the first bit of symbol i's code
        np.cumsum(code.length[self.data], out=self.cum[1:])
        self.mark_bit = int(self.cum[-1])
        assert self.body.size == (self.mark_bit + code.eof_len + 7) // 8

    def __repr__(self):
        return "%s :: %s" % (self.code.label, self.name)

    @property
    def image(self):
        return np.concatenate((self.code.entry.header, self.body))

    def padded(self, extra):
        """the body with `extra` zero bytes behind it: what a piece's look-ahead is cut from"""
        return np.concatenate((self.body, np.zeros(extra, dtype=np.uint8)))

    @functools.cached_property
    def table(self):
        return parse_table(self.code, self.padded(SUB_BYTES + 16))

    def forget(self):
        self.__dict__.pop("table", None)

    def sync(self, lo, hi, first_bit, mutant=None, trace=None):
        """the model of ghf_sync_piece on the body bytes [lo, hi)"""
        assert 0 <= lo <= hi <= self.body.size and 0 <= first_bit < 512 and first_bit <= 8 * (hi - lo)
        if mutant == "ignores_first_bit":
            first_bit = 0
        return walk(self.table, 8 * lo + first_bit, 8 * hi, mutant, trace)

    def true_first(self, lo):
        """the first code boundary at or behind byte lo, in bits from there"""
        return int(self.cum[np.searchsorted(self.cum, 8 * lo, side="left")]) - 8 * lo

    def symbols(self, lo, first_bit, n):
        """the n symbols whose codes start from bit 8 * lo + first_bit on (a true boundary)"""
        k = int(np.searchsorted(self.cum, 8 * lo + first_bit, side="left"))
        assert self.cum[k] == 8 * lo + first_bit
        return self.data[k : k + n]


def expected_bits(code, mode):
    """the mean code length of a draw in that mode, a little low: for sizing a draw"""
    lens = code.length[code.live].astype(np.float64)
    if mode == "deep":
        return float(np.unique(lens)[-2:].min())
    w = np.ldexp(1.0, -lens.astype(np.int64))
    return float((lens * w).sum() / w.sum()) * 0.95


def drawn(code, mode, body_bytes, seed):
    """data of that mode whose codes just reach 8 * body_bytes bits: a draw, cut behind the first symbol that gets there"""
    n0 = int(8 * body_bytes / expected_bits(code, mode)) + 4096
    d = cs.draw(code.entry, mode, n0, seed)
    cum = np.cumsum(code.length[d])
    assert cum[-1] >= 8 * body_bytes, (code, mode, body_bytes)
    return d[: int(np.searchsorted(cum, 8 * body_bytes, side="left")) + 1]


def steer(code, gap):
    """symbols whose lengths add up to `gap` bits (the live lengths have no common divisor): the fewest, the longest first;
    per length the last live symbol, whose codeword is the greatest of its length"""
    sym = {}
    for s in code.live.tolist():
        sym[int(code.length[s])] = s
    best = [None] * (gap + 1)
    best[0] = []
    for g in range(1, gap + 1):
        for l in sorted(sym, reverse=True):
            if l <= g and best[g - l] is not None and (best[g] is None or len(best[g - l]) + 1 < len(best[g])):
                best[g] = best[g - l] + [sym[l]]
    assert best[gap] is not None, (code, gap)
    return best[gap]


# -------------------------------------------------------------------------------------------------------------- tier A
Piece = namedtuple("Piece", "stream lo hi first_bit want")  # own bytes [lo, hi); want: the model's Triple


class Chain:
    def __init__(self, stream, fill, pieces, skew):
        self.stream, self.fill, self.pieces, self.skew = stream, fill, pieces, skew

    def out_offsets(self):
        """where each piece's output begins, from a 16-byte boundary: the chain's output starts `skew` bytes behind one"""
        at, out = self.skew, []
        for p in self.pieces:
            out.append(at)
            at += p.want.n_symbols
        return out


@functools.lru_cache(maxsize=None)
def stream_a(code, fill):
    fixed = sum(A_OWN) + (sum(A_BIG) if fill == "typical" else 0)
    d = drawn(code, fill, fixed + A_TAIL, SEED + (code.ci << 16) + FILLS.index(fill))
    if fill == "typical":
        # the last data code must begin in front of the byte in which the end mark begins: the cut at that byte then leaves
        # the mark entirely in the look-ahead of the piece in front of it
        cum = np.cumsum(code.length[d])
        k = d.size
        while not (cum[k - 1] - code.length[d[k - 1]] < cum[k - 1] // 8 * 8):
            k -= 1
        assert d.size - k <= 64
        d = d[:k]
    return Stream(code, "A/%s" % fill, d)


@functools.lru_cache(maxsize=None)
def tier_a(code):
    """[Chain]: per fill one chain of true entry bits.  `typical` ends with the cut that leaves the end mark in the
    look-ahead (the last piece: n_symbols 0, has_end_mark 1); `deep` ends with a piece that holds symbols and the mark."""
    out = []
    for fi, fill in enumerate(FILLS):
        s = stream_a(code, fill)
        owns = list(A_OWN) + (list(A_BIG) if fill == "typical" else [])
        cuts = list(np.cumsum(owns))
        if fill == "typical":
            cuts.append(s.mark_bit // 8)
        cuts.append(s.body.size)
        assert cuts == sorted(cuts) and cuts[-2] < cuts[-1]
        pieces, lo, first = [], 0, 0
        for hi in cuts:
            want = s.sync(lo, int(hi), first)
            pieces.append(Piece(s, lo, int(hi), first, want))
            lo, first = int(hi), want.landing
        out.append(Chain(s, fill, pieces, (5 * code.ci + 7 * fi + 3) % 16))
        s.forget()
    return out


def piece_buffer(stream, lo, hi, layout):
    """-> (the allocation's bytes, piece_bytes): plus16 = own + 16 bytes in a zeroed buffer of (own + 16 rounded to 16) + 16,
    all of it the piece, as test_gpu_crs_sweep.py builds it; plus8 = own + 8 bytes, the documented minimum, and 0xFF behind"""
    own = hi - lo
    src = stream.padded(32)
    if layout == "plus16":
        size = (own + 16 + 15 & ~15) + 16
        buf = np.zeros(size, dtype=np.uint8)
        buf[: own + 16] = src[lo : hi + 16]
        return buf, size
    buf = np.full((own + 8 + 15 & ~15) + 64, 0xFF, dtype=np.uint8)
    buf[: own + 8] = src[lo : hi + 8]
    return buf, own + 8


# -------------------------------------------------------------------------------------------------------------- tier B
@functools.lru_cache(maxsize=None)
def stream_b(code):
    """deep bytes; then, for every f = 0 .. max_len - 1, the symbols of steer() and the deepest byte symbol (of max_len
    bits: the end mark is never alone at its length), placed so that its code ends f bits behind a byte's edge; deep bytes"""
    seed = SEED + (code.ci << 16) + 0x100
    deepest = code.entry.deepest
    assert code.length[deepest] == code.max_len
    d = drawn(code, "deep", 256, seed).tolist()
    bits = int(code.length[d].sum())
    for f in range(code.max_len):
        gap = code.max_len * code.max_len + (f - code.max_len - bits - code.max_len * code.max_len) % 8
        d += steer(code, gap) + [deepest]
        bits += gap + code.max_len
        assert bits % 8 == f % 8
    d += drawn(code, "deep", B_OWN + 256, seed + 1).tolist()
    return Stream(code, "B/entries", np.array(d, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def tier_b(code):
    """[Piece]: for every first_bit 0 .. max_len - 1 the first byte cut (from byte 1 on) at which it is the true one"""
    s = stream_b(code)
    found = {}
    for lo in range(1, s.body.size - B_OWN - 8):
        found.setdefault(s.true_first(lo), lo)
        if len(found) == code.max_len:
            break
    out = []
    for f in sorted(found):
        lo = found[f]
        out.append(Piece(s, lo, lo + B_OWN, f, s.sync(lo, lo + B_OWN, f)))
    return out


# -------------------------------------------------------------------------------------------------------------- tier C
Guess = namedtuple("Guess", "stream kind lo hi guess want true_first true_want")


def guesses_for(code, true_first):
    """stride - 1, stride, stride + 1, 255, 511, then every value 0 .. max_len - 1, the true one left out; 24 at the most"""
    out = []
    for g in [code.stride - 1, code.stride, code.stride + 1, 255, 511] + list(range(code.max_len)):
        if g != true_first and g not in out:
            out.append(g)
    return out[:C_MAX_GUESSES]


def run_symbol(code):
    """the first live symbol of min_len = L bits whose codeword, rotated by 1 .. L - 1 bits, is each time another L-bit
    code of a byte: no rotation is the end mark or the front of an (L + 1)-bit code, so a parse that enters a run of this
    symbol off a boundary reads L-bit codes for ever and never falls into step"""
    L = code.min_len
    short = set(code.by_len[L]) - ({code.eof_cw} if code.eof_len == L else set())
    for s in code.live.tolist():
        if code.length[s] == L:
            w = int(code.t.codes[s])
            rots = [((w << r) | (w >> (L - r))) & ((1 << L) - 1) for r in range(L)]
            if len(set(rots)) == L and all(r in short for r in rots):
                return s
    raise AssertionError(code)


@functools.lru_cache(maxsize=None)
def stream_c(code, kind):
    """-> (Stream, lo): `drawn`: typical bytes, the pieces begin at byte C_LO.  `run`: k symbols of L + 1 bits, then the
    run; k and the byte lo by search (the fewest symbols, then the first byte), so that no guess of guesses_for() stands
    a multiple of L bits from the true entry bit"""
    seed = SEED + (code.ci << 16) + 0x200
    need = C_LO + max(C_SUBS) * SUB_BYTES + 48
    if kind == "drawn":
        return Stream(code, "C/drawn", drawn(code, "typical", need, seed)), C_LO
    L, r = code.min_len, run_symbol(code)
    longer = next(s for s in code.live.tolist() if code.length[s] == L + 1)
    for k in range(0, 2 * L):
        for lo in range(0, 4):
            first = (k * (L + 1) - 8 * lo) % L if 8 * lo >= k * (L + 1) else None
            if first is None or any((g - first) % L == 0 for g in guesses_for(code, first)):
                continue
            d = [longer] * k + [r] * (8 * need // L + 1)
            return Stream(code, "C/run", np.array(d, dtype=np.uint8)), lo
    raise AssertionError(code)


def c_kinds(code):
    return ("drawn", "run") if code.mode == 2 and code.min_len > 1 else ("drawn",)


@functools.lru_cache(maxsize=None)
def tier_c(code):
    out = []
    for kind in c_kinds(code):
        s, lo = stream_c(code, kind)
        first = s.true_first(lo)
        for subs in C_SUBS:
            hi = lo + subs * SUB_BYTES
            true_want = s.sync(lo, hi, first)
            assert true_want.has_end_mark == 0
            for g in guesses_for(code, first):
                out.append(Guess(s, kind, lo, hi, g, s.sync(lo, hi, g), first, true_want))
    return out


# -------------------------------------------------------------------------------------------------------------- tier D
Marked = namedtuple("Marked", "stream edge offset")  # the end mark starts `offset` bits behind body bit `edge`


@functools.lru_cache(maxsize=None)
def tier_d(code):
    """[Marked]: per edge (a subsequence's, a group's) one stream per offset -max_len .. max_len: a drawn front up to
    max_len^2 bits or more short of the mark, then the symbols of steer()"""
    front = drawn(code, "typical", D_GROUP_EDGE // 8 + 16, SEED + (code.ci << 16) + 0x300)
    cum = np.concatenate(([0], np.cumsum(code.length[front])))
    out = []
    for edge in (D_SUB_EDGE, D_GROUP_EDGE):
        for off in range(-code.max_len, code.max_len + 1):
            mark = edge + off
            k = int(np.searchsorted(cum, mark - code.max_len * code.max_len, side="right")) - 1
            d = np.concatenate((front[:k], np.array(steer(code, mark - int(cum[k])), dtype=np.uint8)))
            s = Stream(code, "D/edge%d%+d" % (edge, off), d)
            assert s.mark_bit == mark
            out.append(Marked(s, edge, off))
    return out


def ends_on_end_bit(m):
    """the end mark's last bit is the body's last: no 1 bits behind it"""
    return (m.stream.mark_bit + m.stream.code.eof_len) % 8 == 0


# -------------------------------------------------------------------------------------------------------------- tier E
Image = namedtuple("Image", "stream nsub stale")


def nsub_of(code, stream_bytes):
    return -(-(8 * stream_bytes - 8 * int(code.entry.header.size)) // SUB_BITS)


@functools.lru_cache(maxsize=None)
def tier_e(code):
    """[Image]: per nsub of E_NSUB a body that ends in the first bytes of its last subsequence, once as it is and once with
    STALE bytes of 0xFF behind it inside stream_bytes (64 subsequences more)"""
    out = []
    for nsub in E_NSUB:
        s = Stream(code, "E/nsub%d" % nsub, drawn(code, "typical", (nsub - 1) * SUB_BYTES + 1, SEED + (code.ci << 16) + 0x400 + nsub))
        assert nsub_of(code, s.image.size) == nsub, (code, nsub, s.body.size)
        out += [Image(s, nsub, 0), Image(s, nsub + STALE // SUB_BYTES, STALE)]
    return out


def image_bytes(im):
    return np.concatenate((im.stream.image, np.full(im.stale, 0xFF, dtype=np.uint8)))


# -------------------------------------------------------------------------------------------------------------- digest
def census():
    """cases per tier"""
    cc = codes()
    return {"A": sum(len(ch.pieces) for c in cc for ch in tier_a(c)) * len(LAYOUTS), "B": sum(len(tier_b(c)) for c in cc),
            "C": sum(len(tier_c(c)) for c in cc), "D": sum(len(tier_d(c)) for c in cc), "E": sum(len(tier_e(c)) for c in cc)}


def triples(mutant=None, of_codes=None):
    """every expected triple of tiers A, B and C, in order (mutant: from a model that is wrong in that way)"""
    out = []
    for c in codes() if of_codes is None else of_codes:
        for ch in tier_a(c):
            for p in ch.pieces:
                t = p.want if mutant is None else p.stream.sync(p.lo, p.hi, p.first_bit, mutant)
                out.append((c.label, "A", p.lo, p.hi, p.first_bit) + tuple(t))
            ch.stream.forget()
        for p in tier_b(c):
            out.append((c.label, "B", p.lo, p.hi, p.first_bit) + tuple(p.want if mutant is None else p.stream.sync(p.lo, p.hi, p.first_bit, mutant)))
        for g in tier_c(c):
            out.append((c.label, "C" + g.kind, g.lo, g.hi, g.guess) + tuple(g.want if mutant is None else g.stream.sync(g.lo, g.hi, g.guess, mutant)))
    return out


def sha256(mutant=None, of_codes=None):
    m = hashlib.sha256()
    cc = codes() if of_codes is None else of_codes
    for c in cc:
        m.update(c.label.encode())
        m.update(c.length.astype("<i8").tobytes())
    m.update(repr(triples(mutant, cc)).encode())
    for c in cc:
        for d in tier_d(c):
            m.update(repr((c.label, d.edge, d.offset, d.stream.n)).encode())
            m.update(hashlib.sha256(d.stream.image.tobytes()).digest())
        for im in tier_e(c):
            m.update(repr((c.label, im.nsub, im.stale, im.stream.n)).encode())
            m.update(hashlib.sha256(image_bytes(im).tobytes()).digest())
    return m.hexdigest()
