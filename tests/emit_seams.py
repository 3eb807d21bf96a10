"""K5 (ghf_emit.hip) across chunk seams: the cases and their expected bytes (numpy and the oracle only; no GPU, no numpy
RNG: every choice comes from datagen.splitmix64 through hist_families.words, as in code_sweep.py).

A wave packs one chunk of C = 16 384 symbols.  The 16-byte unit a chunk shares with its predecessor belongs to the later
chunk: its wave loads the previous chunk's last 128 symbols, looks them up with its packer's own single-symbol lookup and
deposits the last `carry` = 1..127 bits in front of its own first code, clipping a code that straddles the unit boundary.
What this module lays out puts every packer at a seam at every carry, with 1-bit codes (127 carry bits = 127 of the 128
re-loaded symbols), with nothing but the deepest code (cut at every position), with the data as drawn and with the code that
has the most 1 bits, and walks every route a chunk can take behind a seam.

codes()            -> [SeamCode] x 12: two pool codes per packer (by rule, see codes()), shapes (1, 1) and (1, 2), and the
                      combs of depth 40 and 64 for k_emit_long
data_for(code, fill, n) -> uint8[n]: flat over the live symbols; the last 128 symbols of every full chunk by `fill`:
                      all of the least length, all the deepest symbol, as drawn, all the symbol with the most 1 bits
Case(code, fill, n)     -> data, bits (shard_model.code_bits, once), seams(ph), expect(variant), index(lead)
tier_a() / tier_b(packer) / tier_c()   -> [(Case, [Variant])]: the tuples of tests/test_gpu_emit_seams.py
routes(case, variant)   -> the routes the chunks of one emit take, from alignment, size and side-car alone
sha256()           -> one digest over codes, data and expected bytes, pinned in golden/golden_emit_seams.json
                      (sha256_small(): the same over the first code's tuples, for the tests that change a constant)
"""
import functools
import hashlib
from collections import namedtuple

import numpy as np

import code_sweep as cs
import hist_families as hf
import shard_model as sm
from oracle import oracle as orc
from test_gpu_crs import _comb

C = 16384     # symbols per chunk at every size used here (ghf_chunk_symbols; asserted in test_emit_seams_cpu.py)
TILE = 1024   # symbols per tile: 64 lanes x 16
TRIP = 4      # tiles per streamed trip
RELOAD = 128  # symbols of the previous chunk a seam loads again
LAST, REBASE, HEADER, LONG = 1, 2, 4, 8  # GHF_EMIT_*

PACKERS = ("max_len<=9", "max_len<=12", "max_len<=16", "max_len<=32", "k_emit_long")
FILLS = ("shallow", "deep", "mixed", "ones")
B_FILLS = ("deep", "ones")
PHASES8 = (0, 1, 7, 8, 63, 64, 121, 127)
N_A = 2 * C + 1029  # two seams; the last chunk: one full tile and 5 symbols
B_TAILS = (1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 5120, 5121, 9223)
B_SIZES = tuple(C + d for d in B_TAILS) + (2 * C, 3 * C)
ALIGNS = (0, 1, 15)     # d_in's offset from a 16-byte boundary
C_OFFSETS = (0, 3)
C_PLANS = ("behind_k1", "direct")
S_REBASE = 1 << 35      # under GHF_EMIT_REBASE the start bit is S_REBASE + ph
KEEP_UNITS = 3          # without it (and without a header) the start bit is 128 * KEEP_UNITS + ph: d_out[0] is stream byte 0
C_PHASE = 37
SEED_DATA, SEED_HELD = 0x5EA300000000, 0x5EA400000000
FRONTS = ("rebase", "rebase_last", "keep", "keep_last", "header_last")
FRONT_FLAGS = {"rebase": REBASE, "rebase_last": REBASE | LAST, "keep": 0, "keep_last": LAST, "header_last": HEADER | LAST}
ROUTES = ("trips_car", "trips", "odd_tile", "ragged", "unaligned", "end_full", "end_tile", "end_ragged",
          "front_zeros", "front_header", "front_keep")
N_TUPLES = 32824  # (code, fill, size, variant) tuples of the three tiers; see count()

Variant = namedtuple("Variant", "front ph align car plan", defaults=(0, False, "behind_k1"))


def packer_of(max_len):
    return 0 if max_len <= 9 else 1 if max_len <= 12 else 2 if max_len <= 16 else 3 if max_len <= 32 else 4


class SeamCode:
    """one code at the seams: `code` is the ctypes struct K5 is handed (orc.OrcCode: ghf_code's layout)"""

    def __init__(self, label, code, header):
        self.label, self.code, self.header = label, code, header
        self.t = sm.tables(code)
        self.length = np.array(self.t.lens, dtype=np.int64)
        self.min_len, self.max_len = self.t.min_len, self.t.max_len
        self.packer = packer_of(self.max_len)
        self.long = self.packer == 4
        self.live = np.flatnonzero(self.length[:256]).astype(np.int64)
        ll = self.length[self.live]
        self.deepest = int(self.live[np.flatnonzero(ll == ll.max())[-1]])
        self.shallowest = int(self.live[np.flatnonzero(ll == ll.min())[0]])
        # the live symbol whose codeword has the most 1 bits (of equals the longest, then the last): the canonical codes give
        # their deepest symbol nothing but 0 bits, and a seam that cuts or drops such a code wrongly still writes the right bytes
        pop = np.array([bin(self.t.codes[s]).count("1") for s in self.live])
        best = np.flatnonzero(pop == pop.max())
        self.ones = int(self.live[best[np.flatnonzero(ll[best] == ll[best].max())[-1]]])
        self.flags = LONG if self.long else 0

    @property
    def shape(self):
        return (self.min_len, self.max_len)

    def __repr__(self):
        return "%s %s" % (self.label, self.shape)


def long_code(depth):
    """the comb of test_gpu_shard_bits.py::test_long_codes_at_large_start_bits: leaf i has the code '1' * i + '0'"""
    _, cws, lens = _comb(depth)
    code = orc.OrcCode()
    for s in range(orc.NSYM):
        code.length[s], code.codeword[s], code.symbol[s] = 0, 0, 0xFFFFFFFF
    for s, (c, l) in enumerate(zip(cws, lens)):
        code.length[s], code.codeword[s], code.symbol[s] = l, c & 0xFFFFFFFF, c >> 32
    code.min_len, code.max_len = 1, depth
    return SeamCode("comb/depth%d" % depth, code, None)


@functools.lru_cache(maxsize=None)
def codes():
    """Per K5 packer, of code_sweep.pool(): the entry with min_len == 1 and the greatest (max_len, live symbols), then the
    entry with the greatest (min_len, max_len, live symbols); the first entries of shape (1, 1) and (1, 2); the two combs.
    (The first of equals wins: the pool's order is pinned by its digest.)"""
    pool = cs.pool()
    picked = []
    for p in range(4):
        es = [e for e in pool if packer_of(e.max_len) == p]
        picked.append(max((e for e in es if e.min_len == 1), key=lambda e: (e.max_len, e.live.size)))
        picked.append(max(es, key=lambda e: (e.min_len, e.max_len, e.live.size)))
    for shape in ((1, 1), (1, 2)):
        picked.append(next(e for e in pool if (e.min_len, e.max_len) == shape))
    out = tuple([SeamCode(e.label, e.code, e.header) for e in picked] + [long_code(40), long_code(64)])
    for ci, code in enumerate(out):
        code.ci = ci  # its data's seed
    return out


def short_codes():
    return codes()[:10]


def route_codes():
    """tier B: per packer its min_len == 1 code of codes(); k_emit_long: the deeper comb"""
    cc = codes()
    return (cc[0], cc[2], cc[4], cc[6], cc[11])


# ---------------------------------------------------------------------------------------------------------------- data
def data_for(code, fill, n):
    w = hf.words(SEED_DATA + (code.ci << 20) + n, n)
    d = code.live[(w % np.uint64(code.live.size)).astype(np.int64)].astype(np.uint8)
    if fill != "mixed":
        sym = {"shallow": code.shallowest, "deep": code.deepest, "ones": code.ones}[fill]
        for c in range(n // C):  # every full chunk
            d[(c + 1) * C - RELOAD : (c + 1) * C] = sym
    d.setflags(write=False)
    return d


def held_bytes(case, variant, size):
    """what d_out holds before a `keep` emit: a seeded pattern"""
    seed = SEED_HELD + (case.n << 8) + variant.ph
    return hf.words(seed, -(-size // 8)).view(np.uint8)[:size].copy()


def keep_front(held, S, rebased):
    """The image of an emit that has neither GHF_EMIT_REBASE nor GHF_EMIT_HEADER, in a buffer that held `held`: bytes
    [0, 16 * (S >> 7)) stay; in the first unit the bits in front of S stay; everything from S on is the model's --
    `rebased`, the bytes from S's unit through the end bit's unit (zeros behind the end bit) -- then `held` again."""
    want = np.array(held, dtype=np.uint8)
    u0 = 16 * (S >> 7)
    want[u0 : u0 + rebased.size] = rebased
    ph = S & 127
    first = np.unpackbits(want[u0 : u0 + 16])
    first[:ph] = np.unpackbits(np.asarray(held[u0 : u0 + 16], dtype=np.uint8))[:ph]
    want[u0 : u0 + 16] = np.packbits(first)
    return want


Expect = namedtuple("Expect", "S flags cap image end nbytes held lead")


class Case:
    def __init__(self, code, fill, n):
        self.code, self.fill, self.n = code, fill, n
        self.data = data_for(code, fill, n)
        self.nchunks = -(-n // C)

    def __repr__(self):
        return "%r / %s / n=%d" % (self.code, self.fill, self.n)

    @functools.cached_property
    def bits(self):
        return sm.code_bits(self.data, self.code.t)

    @functools.cached_property
    def cum(self):
        """cum[k] = bits of the first k symbols"""
        out = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.code.length[self.data], out=out[1:])
        return out

    @functools.cached_property
    def _index0(self):
        return sm.expected_index(self.data, self.code.t, 0, 0)

    def index(self, lead):
        """the side-car of an emit whose first code stands `lead` bits behind d_out[0]"""
        chunk_bit, seg_bit = self._index0
        return chunk_bit + np.uint64(lead), seg_bit

    def forget(self):
        """drop the bits (one byte each) and what else was derived from the data; all of it comes back on demand"""
        for k in ("bits", "cum", "_index0"):
            self.__dict__.pop(k, None)

    def seams(self, ph):
        """[(c, carry)]: chunk c >= 1 starts `carry` bits into its first unit when the start bit is ph mod 128"""
        return [(c, int((ph + self.cum[c * C]) % 128)) for c in range(1, self.nchunks)]

    def reload(self, c, carry):
        """(symbols of chunk c - 1 that the seam of chunk c must encode again for `carry` bits, whether the first of them
        is cut by the unit boundary)"""
        back = np.cumsum(self.code.length[self.data[c * C - RELOAD : c * C]][::-1])
        assert back[-1] >= 127  # the 128 symbols always cover the carry
        m = int(np.searchsorted(back, carry, side="left")) + 1 if carry else 0
        return m, bool(carry) and int(back[m - 1]) != carry

    def _rebased(self, ph, last):
        S = S_REBASE + ph
        buf, (end, nbytes) = sm.expected_shard(self.data, self.code.t, S, True, last, bits=self.bits)
        cap = sm.min_cap(S, end, sm.origin_of(S, True))
        image = np.zeros(cap, dtype=np.uint8)
        image[:nbytes] = buf
        return image, end - S_REBASE, nbytes

    def expect(self, v):
        """-> Expect: the start bit (None: d_start_bit = NULL), flags, the smallest cap, the cap bytes, d_end, what the
        buffer held (keep fronts) and the bits between d_out[0] and the first code"""
        flags = FRONT_FLAGS[v.front] | self.code.flags
        last = bool(flags & LAST)
        if v.front == "header_last":
            S = sm.header_bits(self.code.t)
            buf, (end, nbytes) = sm.expected_shard(self.data, self.code.t, S, False, True, bits=self.bits)
            cap = sm.min_cap(S, end, 0)
            image = np.zeros(cap, dtype=np.uint8)
            image[:nbytes] = buf
            return Expect(None, flags, cap, image, end, nbytes, None, S)
        image, rel_end, nbytes = self._rebased(v.ph, last)
        if v.front in ("rebase", "rebase_last"):
            return Expect(S_REBASE + v.ph, flags, image.size, image, S_REBASE + rel_end, nbytes, None, v.ph)
        S = 128 * KEEP_UNITS + v.ph
        u0 = 16 * KEEP_UNITS
        cap = u0 + image.size
        assert cap == sm.min_cap(S, 128 * KEEP_UNITS + rel_end, 0)
        held = held_bytes(self, v, cap)
        return Expect(S, flags, cap, keep_front(held, S, image), 128 * KEEP_UNITS + rel_end, u0 + nbytes, held, S)

    def blame(self, e, byte):
        """where byte `byte` of an emit's buffer lies: in front of the first code, in a seam's unit, or in a chunk's body"""
        bit = 8 * byte - e.lead
        if bit < -(e.lead % 128):
            return "in front of the first unit"
        if bit < 128 - e.lead % 128:
            return "the first unit of chunk 0 (the front)"
        c = int(np.searchsorted(self.cum[::C], bit, side="right")) - 1
        for k, carry in self.seams(e.lead % 128):
            unit = (e.lead + int(self.cum[k * C])) // 128 * 16
            if unit <= byte < unit + 16:
                m, cut = self.reload(k, carry)
                return "the unit of seam %d, carry %d, reload %d symbols%s" % (k, carry, m, ", first one cut" if cut else "")
        return "chunk %d of %d, behind its first unit" % (min(c, self.nchunks - 1), self.nchunks)


@functools.lru_cache(maxsize=None)
def case(code, fill, n):
    return Case(code, fill, n)


# --------------------------------------------------------------------------------------------------------------- tiers
def tier_a(code):
    """[(Case, [Variant])]: the four fills at N_A, all 128 start bits, REBASE | LAST with a side-car (long codes: REBASE)"""
    front = "rebase" if code.long else "rebase_last"
    return [(case(code, fill, N_A), [Variant(front, ph, 0, True) for ph in range(128)]) for fill in FILLS]


def fronts_of(code):
    return ("rebase", "keep") if code.long else FRONTS


def tier_b(code, align):
    """[(Case, [Variant])]: the `deep` and the `ones` fill at every size of B_SIZES, d_in `align` bytes off a 16-byte
    boundary; with and without a side-car, every front, ph in PHASES8 (the header front has one start bit: the header's end)"""
    out = []
    for fill, n in ((f, n) for f in B_FILLS for n in B_SIZES):
        vs = []
        for car in (True, False):
            for front in fronts_of(code):
                vs += [Variant(front, ph, align, car) for ph in ((0,) if front == "header_last" else PHASES8)]
        out.append((case(code, fill, n), vs))
    return out


def tier_c(code):
    front = "rebase_last"
    return [(case(code, "mixed", N_A), [Variant(front, C_PHASE, off, True, plan) for off in C_OFFSETS for plan in C_PLANS])]


def all_tuples():
    for code in codes():
        yield from tier_a(code)
    for code in route_codes():
        for align in ALIGNS:
            yield from tier_b(code, align)
    for code in short_codes():
        yield from tier_c(code)


def count():
    return sum(len(vs) for _, vs in all_tuples())


# -------------------------------------------------------------------------------------------------------------- routes
def chunk_routes(code, nsym, aligned, car):
    """the routes one chunk of nsym symbols takes through emit_chunk"""
    wide = code.packer >= 3  # the deposit-by-OR packers have no streamed trips
    r = set()
    nfull = nsym // TILE if aligned else 0
    streamed = not wide and nfull >= TRIP
    if streamed:
        r.add("trips_car" if car else "trips")
    if nfull - (TRIP * (nfull // TRIP) if streamed else 0):
        r.add("odd_tile")  # a full aligned tile that the plain loop takes
    if aligned and nsym % TILE:
        r.add("ragged")
    if not aligned:
        r.add("unaligned")
    return r


def routes(cs_, v, behind_seam=False):
    """the routes of one emit; behind_seam: only what chunks c >= 1 take (chunk 0's front and the end mark stay)"""
    r = set()
    for c in range(1 if behind_seam else 0, cs_.nchunks):
        r |= chunk_routes(cs_.code, min(C, cs_.n - c * C), v.align % 16 == 0, v.car)
    if FRONT_FLAGS[v.front] & LAST:
        tail = cs_.n - (cs_.nchunks - 1) * C
        r.add("end_full" if tail == C else "end_ragged" if tail % TILE else "end_tile")
    r.add({"rebase": "front_zeros", "rebase_last": "front_zeros", "keep": "front_keep", "keep_last": "front_keep",
           "header_last": "front_header"}[v.front])
    return frozenset(r)


def routes_of_packer(packer):
    """the routes a packer can take: no trips beyond 16 bits; k_emit_long has no end mark and writes no header"""
    out = [r for r in ROUTES if not (packer >= 3 and r.startswith("trips"))]
    return tuple(r for r in out if not (packer == 4 and (r.startswith("end_") or r == "front_header")))


def route_table():
    """{route: [emits per packer]} over tier B, counted behind the seams"""
    tab = {r: [0] * len(PACKERS) for r in ROUTES}
    for code in route_codes():
        for align in ALIGNS:
            for cs_, vs in tier_b(code, align):
                for v in vs:
                    for r in routes(cs_, v, behind_seam=True):
                        tab[r][code.packer] += 1
    return tab


# -------------------------------------------------------------------------------------------------------------- digest
def small_tuples():
    """what sha256_small covers: tier A and the aligned tier B of the first code"""
    code = codes()[0]
    return tier_a(code) + tier_b(code, 0)


def sha256_small():
    return sha256(small_tuples(), codes()[:1])


def sha256(tuples=None, of_codes=None):
    m = hashlib.sha256()
    for code in codes() if of_codes is None else of_codes:
        m.update(code.label.encode())
        m.update(code.length.astype("<i8").tobytes())
        m.update(np.array(code.t.codes, dtype="<u8").tobytes())
    seen = set()
    for cs_, vs in all_tuples() if tuples is None else tuples:
        if id(cs_) not in seen:
            seen.add(id(cs_))
            m.update(repr(cs_).encode())
            m.update(cs_.data.tobytes())
            chunk_bit, seg_bit = cs_.index(0)
            m.update(chunk_bit.astype("<u8").tobytes())
            m.update(seg_bit.astype("<u4").tobytes())
        for v in vs:
            key = (id(cs_), v.front, v.ph)
            if key in seen:  # alignment, side-car and plan change no expected byte
                continue
            seen.add(key)
            e = cs_.expect(v)
            m.update(repr((v.front, v.ph, e.S, e.flags, e.cap, e.end, e.nbytes)).encode())
            m.update(e.image.tobytes())
        cs_.forget()
    return m.hexdigest()
