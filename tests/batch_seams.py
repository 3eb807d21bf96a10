"""The one-workgroup-per-item kernels (ghf_batch*.hip, the loops of ghf_batch_core.h) across their round seams: the cases
and their expected bytes (numpy and the oracle only; no GPU, no numpy RNG: every choice comes from datagen.splitmix64
through hist_families.words, as in code_sweep.py and emit_seams.py).

Every kernel of the family works in rounds and carries state across the round edge by hand.  The packers take 4096 symbols
a round and keep the `carry` = B & 127 bits of the incomplete 16-byte unit in the stage; the decoders that find the code
boundaries themselves take 256 x 512 bits a round, start lane 0 of the next round `over[255]` bits behind the edge and let
a round's symbols leave in slices of 16 KiB; the run-record decoders take 256 runs of 128 symbols; the side-car decoders
256 segments of 64.  What this module lays out puts each of them at its seam at every phase the seam can have.

codes()              -> the ten codes of emit_seams.short_codes(): shapes (1,9) (8,9) (1,12) (7,10) (1,16) (2,16) (1,32)
                        (2,32) (1,1) (1,2)
tier P  p_items(code), tails(code), p_planes(k, e), own_items()   every packer at every carry, the body's last unit
tier S  s_items(code), s_planes(k, e)                             the side-car decoders at their round of 16 384 symbols
tier R  r_items(code)                                             the boundary-finding decoders at their edge of 131 072 bits
tier U  u_items(code), u_planes(k, e)                             the run-record decoders at their round of 32 768 symbols
pack_model / decode_model                                         numpy restatements of the two round loops, with mutants
unreachable()        -> the (code, carry) and (code, over) pairs no item can have, by name (pinned in the golden file)
sha256(), census()   -> one digest over every code, item and expected byte; counts and bytes per tier
"""
import functools
import hashlib
from math import gcd

import numpy as np

import code_sweep as cs
import emit_seams as es
import hist_families as hf
import shard_model as sm
from oracle import oracle as orc

# ---- the geometry (asserted against the constexpr lines of ghf_batch_core.h in test_batch_seams_cpu.py) ---------------
LANES = 256                  # kBatchThreads
ROUND = 4096                 # kBatchRoundSymbols: symbols per packer round
STAGE_WORDS = ROUND + 8      # kBatchStageWords
SIDE_ROUND = 16384           # kBatchDecRoundBytes: symbols per round of the side-car decoders
SUB_BITS = 512               # kImgSubBits
EDGE_BITS = LANES * SUB_BITS  # kImgRoundBits = 131 072: bits per round of the boundary-finding decoders
SLICE = 16384                # kImgStageBytes: a round's symbols leave in slices of this many
RUN = 128                    # kBatchRunSymbols
RUN_ROUND = RUN * LANES      # kBatchSeekRoundBytes = 32 768: symbols per round of the run-record decoders
SEG, BLOCK = 64, 4096        # the side-car's segment and block

GUARD = 0xA5
MAX_ITEM = 1 << 20          # GHF_BATCH_MAX_ITEM
OK, E_CAP, E_CORRUPT = 0, 5, 7
FILLS = ("shallow", "deep", "mixed", "ones")
TWO_FILLS = ("deep", "ones")
WIDTHS = (2, 4, 8)
NEAR = 64                    # the symbols on either side of a seam that follow the fill
N_P = 2 * ROUND + 37         # two seams and a ragged last round
ZONE_AT, ZONE = 1024, 128    # the symbols of a round that steer its bits: [ZONE_AT, ZONE_AT + ZONE)
PLANE_STEP = 17              # plane p of a tier-P tensor is at carry (c + 17 p) % 128: every plane at its own
S_CODES, U_CODES = (8, 7), (8, 7)  # (1, 1) and (2, 32)
S_SIZES = tuple(SIDE_ROUND * k + d for k in (1, 2) for d in (0, 1, 63, 64, 65))
U_SIZES = tuple(RUN_ROUND * k + d for k in (1, 2) for d in (0, 1, 127, 128, 129))
U_DEEP_N = 2 * RUN_ROUND + 1  # (2, 32): nothing but the deepest symbol, every run 4096 bits
U_DAMAGED_N = RUN_ROUND + 129
PHASE_CODES = (0, 7)         # (1, 9) and (2, 32): round 0 decodes to every count mod 16
THICK_CODE, EXACT_CODE = 0, 3  # (1, 9): mostly 1-bit codes; (7, 10): round totals of exactly 16 384 and 16 385
SUFFIX = 5                   # drawn symbols behind a straddling code
SEED_P, SEED_T, SEED_S, SEED_U, SEED_R, SEED_O = (0xBA5E00000000 + (k << 36) for k in range(6))
PACK_MUTANTS = ("keep_lost", "stage_not_zeroed", "carry_mod_64", "last_unit_whole")
DECODE_MUTANTS = ("carry_zero", "slice_at_total")


def codes():
    return es.short_codes()


def label(code):
    return "%s %s" % (code.label, code.shape)


def fill_symbol(code, fill):
    return {"shallow": code.shallowest, "deep": code.deepest, "ones": code.ones}[fill]


def flat(code, n, seed):
    """n symbols drawn flat over the live symbols"""
    w = hf.words(seed, n)
    return code.live[(w % np.uint64(code.live.size)).astype(np.int64)].astype(np.uint8)


@functools.lru_cache(maxsize=None)
def steer_pair(code):
    """(A, B, 1 / (len B - len A) mod 128): the shallowest symbol and the first live symbol whose length differs from its
    by an odd number -- changing j of the A in a round's zone to B moves the round's bits by j * (len B - len A), which
    reaches every residue mod 128 within 127 symbols.  None: every live symbol has the same length, and a full round's
    bits are what they are."""
    a = int(code.length[code.shallowest])
    odd = [int(s) for s in code.live if (int(code.length[s]) - a) % 2]
    if not odd:
        assert len(set(code.length[code.live].tolist())) == 1, code
        return None
    b = min(odd, key=lambda s: (int(code.length[s]), s))
    return code.shallowest, b, pow(int(code.length[b]) - a, -1, 128)


def steer(d, lo, hi, code, target):
    """the bits of d[lo:hi) become `target` mod 128 by the zone at lo + ZONE_AT"""
    a, b, inv = steer_pair(code)
    zone = d[lo + ZONE_AT : lo + ZONE_AT + ZONE]
    zone[:] = a
    bits = int(code.length[d[lo:hi]].sum())
    j = (target - bits) % 128 * inv % 128
    zone[:j] = b
    assert int(code.length[d[lo:hi]].sum()) % 128 == target % 128


# ====================================================================================================== tier P: the packers
class Item:
    """one flat item under one code: the data, and from the oracle its body, side-car and run record"""

    def __init__(self, code, tag, data):
        self.code, self.tag = code, tag
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.data.setflags(write=False)
        self.n = int(self.data.size)

    def __repr__(self):
        return "%s / %s / n=%d" % (label(self.code), self.tag, self.n)

    @functools.cached_property
    def body(self):
        return cs.orc_body(self.data, self.code.code)

    @functools.cached_property
    def index(self):
        return cs.expected_index(self.data, self.code.length, 0)

    @functools.cached_property
    def record(self):
        return cs.orc_record(self.data, self.code.length)

    @functools.cached_property
    def image(self):
        return np.concatenate((self.code.header, self.body))

    def round_bits(self, per=ROUND):
        return np.add.reduceat(self.code.length[self.data], range(0, self.n, per))

    def carries(self, lead=0):
        """the carry in front of rounds 1, 2, ..: the bits before them mod 128 (`lead`: the bits in front of the body)"""
        return [int(x) % 128 for x in lead + np.cumsum(self.round_bits())[:-1]]


def p_data(code, fill, c):
    d = flat(code, N_P, SEED_P + (code.ci << 20) + c)
    if fill != "mixed":
        for s in (ROUND, 2 * ROUND):
            d[s - NEAR : min(s + NEAR, N_P)] = fill_symbol(code, fill)
    if steer_pair(code) is None:
        assert c == 0
    else:
        steer(d, 0, ROUND, code, c)
        steer(d, ROUND, 2 * ROUND, code, 127 - 2 * c)
    return d


def carries_of(code):
    """the carries tier P asks of a code at seam 1 (seam 2 then has 127 - c): all 128, or the one its rounds have"""
    return tuple(range(128)) if steer_pair(code) else (0,)


@functools.lru_cache(maxsize=None)
def p_case(code, fill, c):
    return Item(code, "%s/carry %d" % (fill, c), p_data(code, fill, c))


def p_items(code):
    return [p_case(code, fill, c) for fill in FILLS for c in carries_of(code)]


@functools.lru_cache(maxsize=None)
def tails(code):
    """16 items of one seam and a ragged round whose body_bytes takes every value mod 16"""
    end_len, out = int(code.length[256]), []
    if steer_pair(code):
        n = ROUND + 37
        for m in range(16):
            d = flat(code, n, SEED_T + (code.ci << 20) + m)
            steer(d, 0, ROUND, code, 8 * m - end_len - int(code.length[d[ROUND:]].sum()))
            out.append(Item(code, "last unit %d" % m, d))
    else:
        sizes, n = {}, ROUND + 37
        while len(sizes) < 16:
            sizes.setdefault(((int(code.length[code.shallowest]) * n + end_len + 7) >> 3) % 16, n)
            n += 1
        out = [Item(code, "last unit %d" % m, flat(code, sizes[m], SEED_T + (code.ci << 20) + m)) for m in range(16)]
    for m, it in enumerate(out):
        assert it.body.size % 16 == m, it
    return tuple(out)


class Tensor:
    """elements of e bytes whose byte plane p is the data of planes[p]"""

    def __init__(self, name, planes):
        self.name, self.planes, self.e, self.n = name, planes, len(planes), planes[0].n
        assert all(pl.n == self.n for pl in planes)

    @property
    def data(self):
        return np.stack([pl.data for pl in self.planes], axis=1).reshape(-1)

    def __repr__(self):
        return "%s :: %s" % (self.name, " | ".join(label(pl.code) + " " + pl.tag for pl in self.planes))


def plane_carry(code, c, p):
    return (c + PLANE_STEP * p) % 128 if steer_pair(code) else 0


def p_planes(k, e):
    """launch k of width e: plane p under code (k + p) % 10; 4 x 128 tensors with every plane at a carry of its own, then
    the 16 last-unit items of code k beside drawn planes of their size"""
    cc = codes()
    mine = [cc[(k + p) % len(cc)] for p in range(e)]
    out = [Tensor("P%d/E%d/%s/c%d" % (k, e, fill, c), [p_case(code, fill, plane_carry(code, c, p)) for p, code in enumerate(mine)])
           for fill in FILLS for c in range(128)]
    for m, t in enumerate(tails(mine[0])):
        rest = [Item(code, "drawn", flat(code, t.n, SEED_T + (1 << 30) + (code.ci << 20) + 16 * k + m)) for code in mine[1:]]
        out.append(Tensor("P%d/E%d/last unit %d" % (k, e, m), [t] + rest))
    return out


def raw_of(k, e):
    """the one raw plane of forms launch k: never plane 0, so that code k is packed in its own launch"""
    return 1 << (1 + k % (e - 1))


# ---- ghf_compress_batch: the item's own code --------------------------------------------------------------------------
class Own:
    """an item and the code orc.build_code gives its own histogram: the image is orc.compress(data).  `like`: an Own of the
    same multiset, whose code is this one's"""

    def __init__(self, base, tag, data, like=None):
        self.base, self.tag = base, tag
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.data.setflags(write=False)
        self.n = int(self.data.size)
        self.code = like.code if like else orc.build_code(orc.histogram(self.data))
        self.length = like.length if like else np.array(list(self.code.length), dtype=np.int64)
        self.header = like.header if like else orc.header_bytes(self.code)
        self.lead = 8 * int(self.header.size)

    def __repr__(self):
        return "own code of %s (%d, %d) / %s / n=%d" % (self.base.label, self.code.min_len, self.code.max_len, self.tag, self.n)

    @functools.cached_property
    def image(self):
        return orc.compress(self.data)

    @functools.cached_property
    def index(self):
        return cs.expected_index(self.data, self.length, self.lead)

    def carries(self):
        rb = np.add.reduceat(self.length[self.data], range(0, self.n, ROUND))
        return [int(x) % 128 for x in self.lead + np.cumsum(rb)[:-1]]


@functools.lru_cache(maxsize=None)
def own_multiset(code):
    """(N_P symbols whose counts are the pool histogram of `code` scaled to N_P, every live symbol at least once; the Own of
    them in ascending order, whose code every order of them has)"""
    h = np.asarray(next(e.hist for e in cs.pool() if e.label == code.label), dtype=np.float64)[:256]
    live = np.flatnonzero(h)
    k = np.maximum(1, np.floor(h[live] * (N_P - live.size) / h[live].sum())).astype(np.int64)
    order = np.argsort(-h[live], kind="stable")
    i = 0
    while k.sum() != N_P:  # the rounding's remainder goes to (or comes from) the most frequent symbols
        j = order[i % order.size]
        step = 1 if k.sum() < N_P else -1
        if k[j] + step >= 1:
            k[j] += step
        i += 1
    ms = np.repeat(live, k).astype(np.uint8)
    return ms, Own(code, "sorted", ms)


def _exchange(d, L, mine, theirs, need, limit):
    """exchanges between positions `mine` and `theirs` (one length each per exchange) that move the bits of `mine` by
    `need` mod 128 in at most `limit` exchanges; -> whether one was found (and made)"""
    if need % 128 == 0:
        return True
    lm, lt = L[d[mine]], L[d[theirs]]
    plans = []
    for x in np.unique(lm):
        for y in np.unique(lt):
            if (y - x) % 2:
                j = need * pow(int(y - x), -1, 128) % 128
                if j <= min(limit, int((lm == x).sum()), int((lt == y).sum())):
                    plans.append((j, int(x), int(y)))
    if not plans:
        return False
    j, x, y = min(plans)
    a, b = mine[np.flatnonzero(lm == x)[:j]], theirs[np.flatnonzero(lt == y)[:j]]
    d[a], d[b] = d[b], d[a]
    return True


def swap_in(d, L, mine, theirs, length):
    """the symbols at `mine` become symbols of `length`, exchanged with such symbols at `theirs`"""
    want = mine[L[d[mine]] != length]
    have = theirs[L[d[theirs]] == length][: want.size]
    if have.size < want.size:
        return False
    d[want], d[have] = d[have], d[want]
    return True


@functools.lru_cache(maxsize=None)
def _last_round_plans(code):
    """(x, {r: (j1, y1, j2, y2)}): the last round's 37 symbols all of length x (the least the multiset has 300 of) and then
    j1 of them of length y1 and j2 of length y2 (of either at most a quarter of what the multiset has) have 37 x + r bits
    mod 128; the fewest exchanges win"""
    ms, probe = own_multiset(code)
    counts = np.bincount(probe.length[ms])
    x = int(np.flatnonzero(counts >= 300)[0])
    k = N_P - 2 * ROUND
    most = {int(y): min(k, int(counts[y]) // 4) for y in np.flatnonzero(counts) if y != x and counts[y] >= 4}  # a quarter: round 1 has them
    plans = {}
    for y1 in most:
        for y2 in most:
            for j1 in range(most[y1] + 1):
                for j2 in range(min(most[y2], k - j1) + 1 if y2 > y1 else 1):
                    r = (j1 * (y1 - x) + j2 * (y2 - x)) % 128
                    if r not in plans or j1 + j2 < plans[r][0] + plans[r][2]:
                        plans[r] = (j1, y1, j2, y2)
    plans[0] = (0, x, 0, x)
    return x, plans


def own_data(code, fill, c):
    """the multiset of own_multiset(code) in an order that asks seam 1 to carry c and seam 2 to 127 - c behind the item's own
    header.  The multiset never changes, so the item's own code never does; a carry is reached by exchanging symbols of two
    lengths between the rounds: seam 2 between the 37 symbols of the last round and the rounds in front of it
    (_last_round_plans), then seam 1 between rounds 0 and 1 (lengths an odd number apart).  Where the multiset has too few
    symbols of such lengths the seam stays where it fell.  The fill -- the symbols of the least length, of the greatest
    length, with the most 1 bits that rounds 0 and 1 have -- stands NEAR in front of either seam and NEAR behind the first;
    the last round belongs to seam 2's carry."""
    ms, probe = own_multiset(code)
    L, lead = probe.length, probe.lead
    d = ms[np.argsort(hf.words(SEED_O + (code.ci << 20) + c, N_P), kind="stable")].copy()
    if fill != "mixed":
        pop = np.array([bin(int(w)).count("1") for w in probe.code.codeword], dtype=np.int64)
        head = d[: 2 * ROUND]
        key = {"shallow": L[head], "deep": -L[head], "ones": -(64 * pop[head] + L[head])}[fill]
        front = np.concatenate((np.arange(ROUND - NEAR, ROUND + NEAR), np.arange(2 * ROUND - NEAR, 2 * ROUND)))
        top = np.argsort(key, kind="stable")[: front.size]
        src, dst = top[~np.isin(top, front)], front[~np.isin(front, top)]
        d[src], d[dst] = d[dst], d[src]
    free0, free1 = np.arange(ROUND - NEAR), np.arange(ROUND + NEAR, 2 * ROUND - NEAR)
    # seam 2 = lead + every bit - the last round's: the last round becomes all of one length, then two lengths more
    last = np.arange(2 * ROUND, N_P)
    x, plans = _last_round_plans(code)
    free = np.concatenate((free1, free0))
    assert swap_in(d, L, last, free, x)
    plan = plans.get((lead + int(L[d].sum()) - last.size * x - (127 - c)) % 128)
    if plan:  # (none, or too few symbols left beside the fill: seam 2 stays where it fell)
        j1, y1, j2, y2 = plan
        if swap_in(d, L, last[:j1], free, y1):
            swap_in(d, L, last[j1 : j1 + j2], free, y2)
    _exchange(d, L, free0, free1, c - lead - int(L[d[:ROUND]].sum()), 128)
    assert np.array_equal(np.sort(d), ms)
    return d


@functools.lru_cache(maxsize=None)
def own_items():
    """per code and fill 128 items, seam 1 asked to every carry behind the item's own header and seam 2 to 127 - c
    -> [Own]; what they reach is theirs to say (Own.carries) and the CPU test's to hold"""
    out = []
    for code in codes():
        ms, probe = own_multiset(code)
        for fill in FILLS:
            for c in range(128 if np.unique(ms).size > 1 else 1):
                out.append(Own(code, "%s/carry %d" % (fill, c), own_data(code, fill, c), like=probe))
    return tuple(out)


# ============================================================================== tiers S and U: the rounds that are handed their bits
def near_seams(code, fill, n, per, seed):
    d = flat(code, n, seed)
    for s in range(per, n + per, per):
        d[max(s - NEAR, 0) : min(s + NEAR, n)] = fill_symbol(code, fill)
    return d


@functools.lru_cache(maxsize=None)
def s_items(code):
    return tuple(Item(code, "%s/S" % fill, near_seams(code, fill, n, SIDE_ROUND, SEED_S + (code.ci << 20) + n)) for fill in TWO_FILLS for n in S_SIZES)


@functools.lru_cache(maxsize=None)
def u_items(code):
    out = [Item(code, "%s/U" % fill, near_seams(code, fill, n, RUN_ROUND, SEED_U + (code.ci << 20) + n)) for fill in TWO_FILLS for n in U_SIZES]
    if code.shape == (2, 32):
        out.append(Item(code, "deepest/U", np.full(U_DEEP_N, code.deepest, dtype=np.uint8)))
    return tuple(out)


def _planes_of(items_of, k, e, pair, what):
    cc = codes()
    mine = [cc[pair[(k + p) % 2]] for p in range(e)]
    sets = [items_of(code) for code in mine]
    count = min(len(s) for s in sets)
    return [Tensor("%s%d/E%d/%s" % (what, k, e, sets[0][i].tag), [s[i] for s in sets]) for i in range(count)]


def s_planes(k, e):
    """launch k (0, 1) of width e: plane p under S_CODES[(k + p) % 2], the items of s_items side by side"""
    return _planes_of(s_items, k, e, S_CODES, "S")


def u_planes(k, e):
    return _planes_of(u_items, k, e, U_CODES, "U")


def damaged_record(item):
    """the record with the first run of round 1 one bit long"""
    rec = item.record.copy()
    assert item.n > RUN_ROUND
    run = rec[8:].view("<u2")
    assert run[LANES] != 1
    run[LANES] = 1
    return rec


@functools.lru_cache(maxsize=None)
def u_damaged(code):
    return Item(code, "damaged/U", near_seams(code, "ones", U_DAMAGED_N, RUN_ROUND, SEED_U + (code.ci << 20) + 7))


# ============================================================================ tier R: the decoders that find the boundaries
@functools.lru_cache(maxsize=None)
def _tails(code, with_count):
    """coin change over the live lengths, once per code: last[t] (or last[t][count % 16]) = the length of the last symbol
    of some symbol sequence of exactly t bits, or 0"""
    lens = sorted(set(code.length[code.live].tolist()))
    T = 12 * code.max_len + 1
    if not with_count:
        last = [0] * T
        for t in range(1, T):
            last[t] = next((l for l in lens if t == l or (t > l and last[t - l])), 0)
        return last
    last = [[0] * 16 for _ in range(T)]
    for t in range(1, T):
        for cm in range(16):
            last[t][cm] = next((l for l in lens if (t == l and cm == 1) or (t > l and last[t - l][(cm - 1) % 16])), 0)
    return last


def exact(code, bits, seed, count_mod=None):
    """live symbols of exactly `bits` bits (and of a count that is count_mod mod 16): drawn flat up to a tail of 8 .. 9 max_len
    bits, which coin change fills.  None: no sequence of live symbols has that many bits."""
    lens = code.length[code.live]
    if bits % functools.reduce(gcd, lens.tolist()):
        return None
    first_of = {}
    for s in code.live:
        first_of.setdefault(int(code.length[s]), int(s))
    room = 8 * code.max_len
    head = np.zeros(0, dtype=np.uint8)
    if bits > room:
        d = flat(code, (bits - room) // int(lens.min()) + 1, seed)
        cum = np.cumsum(code.length[d])
        head = d[: int(np.searchsorted(cum, bits - room, side="right"))]
    left = bits - int(code.length[head].sum())
    tail = []
    if count_mod is None:
        last = _tails(code, False)
        while left:
            assert last[left], (code, bits)
            tail.append(first_of[last[left]])
            left -= last[left]
    else:
        last, cm = _tails(code, True), (count_mod - head.size) % 16
        while left:
            assert last[left][cm], (code, bits, count_mod)
            tail.append(first_of[last[left][cm]])
            left, cm = left - last[left][cm], (cm - 1) % 16
        assert cm == 0
    out = np.concatenate((head, np.array(tail, dtype=np.uint8)))
    assert int(code.length[out].sum()) == bits
    return out


class RItem(Item):
    """an item of tier R: `cut` = the stream bytes the decoder is given (None: the whole body), `cap` (None: n)"""

    def __init__(self, code, family, over, data, cut=None, cap=None):
        super().__init__(code, "%s/over %d" % (family, over), data)
        self.family, self.over, self.cut, self.cap = family, over, cut, cap
        self.cum = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(code.length[self.data], out=self.cum[1:])
        self.end_len = int(code.length[256])

    @property
    def stream_bytes(self):
        return int(self.body.size) if self.cut is None else self.cut

    @functools.cached_property
    def round_totals(self):
        """the symbols that begin in each round of EDGE_BITS bits; the end mark's round is the last"""
        rounds = int(self.cum[self.n]) // EDGE_BITS + 1
        return np.bincount(self.cum[:-1] // EDGE_BITS, minlength=rounds)

    @functools.cached_property
    def verdict(self):
        """(status, d_out_bytes, the symbols a decode pass stores, the rounds the item takes)"""
        totals = self.round_totals
        if self.cut is not None and 8 * self.cut < self.cum[self.n] + self.end_len:
            assert 8 * self.cut > self.cum[self.n]  # the bytes stop inside the end mark ...
            assert totals.size == 1                   # ... which round 0 meets: nothing is stored
            return E_CORRUPT, 0, 0, 1
        if self.cap is not None and self.cap < self.n:
            through = np.cumsum(totals)
            r = int(np.searchsorted(through, self.cap, side="right"))  # the first round that would cross the cap
            return E_CAP, 0, int(through[r - 1]) if r else 0, r + 1
        return OK, self.n, self.n, int(totals.size)

    @property
    def sizes_verdict(self):
        """the same item in a sizes-only pass: no cap"""
        v = self.verdict
        return v if v[0] != E_CAP else (OK, self.n, 0, int(self.round_totals.size))

    def straddles_a_slice(self):
        """whether some lane's symbols of some round lie on both sides of a slice edge of that round's output"""
        sub = self.cum[:-1] // SUB_BITS  # the lane (and round) a symbol begins in
        firsts = np.flatnonzero(np.diff(np.concatenate(([-1], sub))))  # the first symbol of every lane that has one
        lasts = np.concatenate((firsts[1:], [self.n])) - 1
        base = np.concatenate(([0], np.cumsum(self.round_totals)))[sub[firsts] // LANES]
        return bool(np.any((firsts - base) // SLICE != (lasts - base) // SLICE))


def _suffix(code, seed):
    return flat(code, SUFFIX, seed + 99)


@functools.lru_cache(maxsize=None)
def r_items(code):
    """-> ([RItem], [names of what cannot exist]) around the edge at bit EDGE_BITS of the body"""
    out, missing = [], []
    seed = SEED_R + (code.ci << 24)
    end_len = int(code.length[256])

    def add(family, over, bits, behind, **kw):
        head = exact(code, bits, seed + (len(out) << 8))
        if head is None:
            missing.append("%s: %s/over %d" % (label(code), family, over))
            return None
        it = RItem(code, family, over, np.concatenate((head, np.asarray(behind, dtype=np.uint8))), **kw)
        out.append(it)
        return it

    # a data code begins len - over bits in front of the edge: the deepest, then the one with the most 1 bits
    for family, sym in (("deep", code.deepest), ("ones", code.ones)):
        L = int(code.length[sym])
        for over in range(L):
            it = add(family, over, EDGE_BITS - (L - over), np.concatenate(([sym], _suffix(code, seed + over))))
            if it is not None:
                assert it.cum[it.n - SUFFIX - 1] == EDGE_BITS - L + over and it.round_totals.size == 2
    # the end mark begins on the edge (round 1 has no symbol), ends on it, straddles it
    add("mark begins on the edge", 0, EDGE_BITS, [])
    add("mark ends on the edge", 0, EDGE_BITS - end_len, [])
    for over in range(1, end_len):
        add("mark straddles", over, EDGE_BITS - (end_len - over), [])
    # ... and is the first code behind a straddling data code
    L = int(code.length[code.deepest])
    for over in range(1, L):
        add("mark behind the straddler", over, EDGE_BITS - (L - over), [code.deepest])
    # the bytes stop inside a straddling end mark
    for over in range(1, end_len):
        add("cut inside the mark", over, EDGE_BITS - (end_len - over), [], cut=EDGE_BITS // 8)
    # the cap is one below the size and the symbol that crosses it begins in round 1
    over = min(1, L - 1)
    it = add("cap", over, EDGE_BITS - (L - over), np.concatenate(([code.deepest], _suffix(code, seed + 77))))
    if it is not None:
        it.cap = it.n - 1
        assert it.verdict == (E_CAP, 0, it.n - SUFFIX, 2)
    # round 0 decodes to every count mod 16
    if code.ci in PHASE_CODES:
        over = 1
        for m in range(16):
            head = exact(code, EDGE_BITS - (L - over), seed + (m << 12) + 5, count_mod=(m - 1) % 16)
            it = RItem(code, "phase %d" % m, over, np.concatenate((head, [code.deepest], _suffix(code, seed + m))))
            assert it.round_totals[0] % 16 == m and it.round_totals.size == 2
            out.append(it)
    # slices: rounds of far more than 16 Ki symbols
    one = [int(s) for s in code.live if code.length[s] == 1]
    if code.shape in ((1, 1), (1, 2)):
        per = EDGE_BITS // int(code.length[code.shallowest])
        it = RItem(code, "slices", 0, flat(code, 2 * per + 5, seed + 3))
        assert it.round_totals.tolist() == [per, per, 5]
        out.append(it)
    if code.ci == THICK_CODE:  # 1-bit codes with a few 2-bit ones: round 0 leaves in eight slices, round 1 starts at an odd phase
        two = next(int(s) for s in code.live if code.length[s] == 2)
        d = np.full(2 * EDGE_BITS + 5, one[0], dtype=np.uint8)
        d[[100, 20000, 40000, 60000, 80000, 140000, 170000, 200000]] = two
        d = d[: int(np.searchsorted(np.cumsum(code.length[d]), 2 * EDGE_BITS, side="left")) + 1 + 5]
        it = RItem(code, "slices", 0, d)
        assert it.round_totals.tolist() == [EDGE_BITS - 5, EDGE_BITS - 3, 5] and it.straddles_a_slice()
        out.append(it)
    if code.ci == EXACT_CODE:  # a round of exactly one slice, and of one slice and a symbol
        seven = next(int(s) for s in code.live if code.length[s] == 7)
        eight = next(int(s) for s in code.live if code.length[s] == 8)
        for want, front in ((SLICE, [eight] * SLICE), (SLICE + 1, [seven] * 8 + [eight] * (SLICE - 7))):
            it = RItem(code, "round of %d" % want, 0, np.concatenate((np.array(front, dtype=np.uint8), flat(code, 100, seed + want))))
            assert it.round_totals.tolist() == [want, 100] and it.cum[want] == EDGE_BITS
            out.append(it)
    return tuple(out), tuple(missing)


def r_planes(k, e):
    """launch k of width e: plane 0 = the items of r_items(code k) that decode whole and are no more than MAX_ITEM bytes as
    elements, plane p > 0 drawn under code (k + p) % 10 at the same count (its rounds fall where they fall).  Under (1, 1)
    the edge lies 131 072 symbols into an item: at e = 8 the two items whose end mark stands at the edge are left"""
    cc = codes()
    out = []
    for i, it in enumerate(x for x in r_items(cc[k])[0] if x.cut is None and x.cap is None and x.n * e <= MAX_ITEM):
        rest = [Item(cc[(k + p) % len(cc)], "drawn", flat(cc[(k + p) % len(cc)], it.n, SEED_R + (1 << 34) + (k << 24) + (p << 16) + i))
                for p in range(1, e)]
        out.append(Tensor("R%d/E%d/%s" % (k, e, it.tag), [it] + rest))
    return out


# ======================================================================================================= what cannot exist
def unreachable():
    """by name: the carries a packer seam cannot have and the `over` values no code can straddle the edge by.  A code
    whose live symbols all have one length l packs 4096 l bits a round -- a multiple of 128 -- so its carry is the one in
    front of round 0; under it every code begins at a multiple of l (behind a header of a multiple of 64 bits), so the
    edge at 131 072 is never inside one and an end mark of one bit never straddles."""
    names = []
    for code in codes():
        if steer_pair(code) is None:
            names += ["%s: carry %d" % (label(code), c) for c in range(1, 128)]
        names += list(r_items(code)[1])
    return names


# ===================================================================================== the packer's round loop, restated
def pack_model(data, length, bits, end_bits, room, header=None, mutant=None):
    """batch_shared_compress_body's step 4 (header None) or k_compress_batch's rounds (header: the item's own) on arrays of
    bits: the stage, `carry`, `keep`, the last unit byte by byte.  bits = the data's codes, one entry per bit; end_bits =
    the end mark's.  -> `room` bytes that held GUARD.  mutant: one of PACK_MUTANTS"""
    out = np.full(room, GUARD, dtype=np.uint8)
    n = int(data.size)
    rb = np.add.reduceat(length[data], range(0, n, ROUND))
    B = 0
    stage = np.zeros(32 * STAGE_WORDS, dtype=np.uint8)
    if header is not None:
        B = 8 * int(header.size)
        whole = int(header.size) & ~15
        out[:whole] = header[:whole]
        stage[: B & 127] = np.unpackbits(header[whole:])
    total_bytes = (B + bits.size + end_bits.size + 7) >> 3
    at = 0
    for r, round_bits in enumerate(int(x) for x in rb):
        carry = B & (63 if mutant == "carry_mod_64" else 127)
        stage[carry : carry + round_bits] |= bits[at : at + round_bits]
        T = carry + round_bits
        last = r + 1 == rb.size
        if last:
            pad = -(T + end_bits.size) & 7
            stage[T : T + end_bits.size] |= end_bits
            stage[T + end_bits.size : T + end_bits.size + pad] |= 1
            T += end_bits.size + pad
        base_byte = (B - carry) >> 3
        full_units = T >> 7
        units = (T + 127) >> 7 if last else full_units
        unit_bytes = np.packbits(stage[: 128 * units])
        stop = base_byte + 16 * units if mutant == "last_unit_whole" else min(base_byte + 16 * units, total_bytes)
        stop = min(stop, room)
        if stop > base_byte:
            out[base_byte:stop] = unit_bytes[: stop - base_byte]
        keep = stage[128 * full_units : 128 * full_units + 128].copy()
        if not last:
            if mutant != "stage_not_zeroed":
                stage[:] = 0
            stage[:128] = 0 if mutant == "keep_lost" else keep
        B += round_bits
        at += round_bits
    return out


def packed(item, mutant=None):
    """pack_model on a flat item under its shared code -> the slot's bytes: body_bytes rounded up to 16, and 16 of guard"""
    room = (int(item.body.size) + 15 & ~15) + 16
    t = item.code.t
    el, ec = t.lens[256], t.codes[256]
    end_bits = np.array([(ec >> (el - 1 - i)) & 1 for i in range(el)], dtype=np.uint8)
    return pack_model(item.data, item.code.length, sm.code_bits(item.data, t), end_bits, room, mutant=mutant)


def slot_of(item):
    room = (int(item.body.size) + 15 & ~15) + 16
    want = np.full(room, GUARD, dtype=np.uint8)
    want[: item.body.size] = item.body
    return want


# ============================================================================ the boundary decoder's round loop, restated
@functools.lru_cache(maxsize=None)
def _lut16(code):
    """(sym, len) by the first 16 bits of a window, len 0 where the code is longer than that (or none begins so), and per
    length beyond 16 the sorted codewords with their symbols"""
    lens = np.array(code.t.lens)
    sym, length = np.zeros(1 << 16, dtype=np.int64), np.zeros(1 << 16, dtype=np.int64)
    longer = []
    for l in sorted(set(lens[lens > 0].tolist())):
        syms = np.flatnonzero(lens == l)
        cws = np.array([code.t.codes[s] for s in syms], dtype=np.uint64)
        if l <= 16:
            for s, c in zip(syms, cws):
                lo = int(c) << (16 - l)
                sym[lo : lo + (1 << (16 - l))], length[lo : lo + (1 << (16 - l))] = s, l
        else:
            order = np.argsort(cws)
            longer.append((l, cws[order], syms[order]))
    return sym, length, longer


def code_at_every_bit(stream, code):
    """(sym, len) of the code that begins at every bit of the stream (zeros behind it); len 0: none does"""
    b = np.concatenate((stream, np.zeros(8, dtype=np.uint8))).astype(np.uint64)
    nbytes = int(stream.size)
    v = np.zeros(nbytes, dtype=np.uint64)  # the 40 bits from every byte on
    for k in range(5):
        v |= b[k : k + nbytes] << np.uint64(32 - 8 * k)
    win = np.empty((nbytes, 8), dtype=np.uint64)
    for s in range(8):
        win[:, s] = (v >> np.uint64(8 - s)) & np.uint64(0xFFFFFFFF)
    win = win.reshape(-1)
    sym16, len16, longer = _lut16(code)
    top = (win >> np.uint64(16)).astype(np.int64)
    sym_at, len_at = sym16[top], len16[top]
    rest = np.flatnonzero(len_at == 0)
    for l, cws, syms in longer:
        if rest.size == 0:
            break
        cand = win[rest] >> np.uint64(32 - l)
        k = np.minimum(np.searchsorted(cws, cand), cws.size - 1)
        hit = cws[k] == cand
        len_at[rest[hit]], sym_at[rest[hit]] = l, syms[k[hit]]
        rest = rest[~hit]
    return sym_at.tolist(), len_at.tolist()


def decode_model(stream, code, first_bit=0, cap=None, room=0, mutant=None, scan=None):
    """batch_decode_rounds, lane after lane: rounds of EDGE_BITS bits from first_bit on, lane 0 of a round `carry` bits
    behind its edge, a round's symbols stored in slices of SLICE at total + lo.  -> (status, total, rounds, `room` bytes
    that held GUARD; room 0: a sizes-only pass).  mutant: one of DECODE_MUTANTS; scan: code_at_every_bit(stream, code), where
    the caller has it"""
    sym_at, len_at = scan or code_at_every_bit(stream, code)
    end_bit = 8 * int(stream.size)
    out = np.full(room, GUARD, dtype=np.uint8)
    base, carry, total, rounds = first_bit, 0, 0, 0
    while True:
        rounds += 1
        pos, edge = base + (0 if mutant == "carry_zero" else carry), base + EDGE_BITS
        syms, stop = [], None
        while pos < edge:
            l = len_at[pos] if pos < end_bit else 0
            if l == 0 or l > end_bit - pos:
                stop = "cut off"
                break
            if sym_at[pos] == 256:
                stop = "end mark"
                break
            syms.append(sym_at[pos])
            pos += l
        if stop == "cut off":
            return E_CORRUPT, 0, rounds, out
        if cap is not None and total + len(syms) > cap:
            return E_CAP, 0, rounds, out
        if room:
            for lo in range(0, len(syms), SLICE):
                at = total + (0 if mutant == "slice_at_total" else lo)
                piece = syms[lo : lo + SLICE]
                out[at : at + len(piece)] = piece
        total += len(syms)
        if stop == "end mark":
            return OK, total, rounds, out
        carry, base = pos - edge, edge


@functools.lru_cache(maxsize=2)
def scan_of(item):
    return code_at_every_bit(item.body[: item.stream_bytes], item.code)


def decoded(item, mutant=None):
    """decode_model on an item of tier R as the decode pass takes it: into cap bytes, 16 of guard behind them"""
    cap = item.n if item.cap is None else item.cap
    return decode_model(item.body[: item.stream_bytes], item.code, cap=cap, room=item.n + 16, mutant=mutant, scan=scan_of(item))


def want_decoded(item):
    status, nbytes, stored, rounds = item.verdict
    out = np.full(item.n + 16, GUARD, dtype=np.uint8)
    out[:stored] = item.data[:stored]
    return status, nbytes, rounds, out


# ===================================================================================================== the mutant tables
def pack_mutant_table():
    """{code: [per mutant of PACK_MUTANTS the carries of the `ones` fill at which it changes a byte of the slot]}"""
    table = {}
    for code in codes():
        caught = dict.fromkeys(PACK_MUTANTS, 0)
        for it in p_items(code):
            if it.tag.startswith("ones/"):
                want = slot_of(it)
                for m in PACK_MUTANTS:
                    caught[m] += int(not np.array_equal(packed(it, m), want))
        table[label(code)] = [caught[m] for m in PACK_MUTANTS]
    return table


def decode_mutant_table():
    """{code: {mutant: [items at which it changes the verdict or a byte, items that could show it]}}: the carry matters to
    the `ones` items with over > 0, the slice's place to every item that stores a round of more than one slice"""
    table = {}
    for code in codes():
        caught = {m: [0, 0] for m in DECODE_MUTANTS}
        for it in r_items(code)[0]:
            want = want_decoded(it)
            shows = {"carry_zero": it.family == "ones" and it.over > 0,
                     "slice_at_total": it.verdict[0] != E_CORRUPT and int(it.round_totals.max()) > SLICE}
            for m in DECODE_MUTANTS:
                if shows[m]:
                    g = decoded(it, m)
                    caught[m][0] += int(g[:2] != want[:2] or not np.array_equal(g[3], want[3]))
                    caught[m][1] += 1
        table[label(code)] = caught
    return table


# ================================================================================================================ digest
def census():
    """{tier: (items, symbols, expected bytes)}"""
    rows = {}

    def row(name, items, want):
        items = list(items)
        rows[name] = (len(items), sum(it.n for it in items), sum(int(want(it).size) for it in items))

    row("P carries", (it for c in codes() for it in p_items(c)), lambda it: it.body)
    row("P last units", (it for c in codes() for it in tails(c)), lambda it: it.body)
    row("P own codes", own_items(), lambda it: it.image)
    row("S", (it for k in S_CODES for it in s_items(codes()[k])), lambda it: it.data)
    row("R", (it for c in codes() for it in r_items(c)[0]), lambda it: it.data)
    row("U", (it for k in U_CODES for it in u_items(codes()[k])), lambda it: it.record)
    return rows


def sha256():
    m = hashlib.sha256()
    for code in codes():
        m.update(label(code).encode())
        m.update(code.length.astype("<i8").tobytes())
        m.update(np.array(code.t.codes, dtype="<u8").tobytes())

    def flat_item(it, index=True):
        m.update(repr(it).encode())
        m.update(it.data.tobytes())
        m.update(it.body.tobytes())
        m.update(it.record.tobytes())
        if index:
            chunk_bit, seg_bit = it.index
            m.update(chunk_bit.astype("<u8").tobytes())
            m.update(seg_bit.astype("<u4").tobytes())

    for code in codes():
        for it in p_items(code) + list(tails(code)):
            flat_item(it)
    for k in range(len(codes())):
        for e in WIDTHS:  # the planes of a launch are the items above; the drawn planes beside the last units are new
            for t in p_planes(k, e)[-16:]:
                for pl in t.planes[1:]:
                    flat_item(pl)
    for it in own_items():
        m.update(repr(it).encode())
        m.update(it.data.tobytes())
        m.update(it.image.tobytes())
        m.update(it.index[0].astype("<u8").tobytes())
        m.update(it.index[1].astype("<u4").tobytes())
    for k in S_CODES:
        for it in s_items(codes()[k]):
            flat_item(it)
    for k in U_CODES:
        for it in u_items(codes()[k]) + (u_damaged(codes()[k]),):
            flat_item(it, index=False)
        m.update(damaged_record(u_damaged(codes()[k])).tobytes())
    for code in codes():
        items, missing = r_items(code)
        for it in items:
            m.update(repr((it, it.cut, it.cap, it.verdict, it.sizes_verdict)).encode())
            m.update(it.data.tobytes())
            m.update(it.body.tobytes())
        m.update(repr(missing).encode())
    m.update(repr(unreachable()).encode())
    return m.hexdigest()
