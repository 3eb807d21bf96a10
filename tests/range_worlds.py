"""The inputs of the range / seek decode tests, and what each of them must exercise.  No GPU is needed here.

ghf_decode_range runs three kernels over one table image (k_seek_expand, k_decode_head, K7 = k_decode), and K7 picks one
of six hot loops per launch from the code's lengths alone.  A "world" is a small input whose code lands in one named
class; `world(name)` computes, with the oracle only, what the tests need to know about it BEFORE anything is decoded:
the code lengths, the compressed bytes of every block of 4096 symbols, the stream.  `decoder_class` restates K7's choice
as a function of (min_len, max_len); it is written down here from the list of K7's hot loops, not imported from the
library, and tests/test_range_worlds_cpu.py holds every world against the class it was chosen for.

Random choices come from datagen.splitmix64 (no numpy RNG: the worlds must never change)."""
import functools
import struct

import numpy as np

import datagen as dg
from cases import CASES
from oracle import oracle as orc

BLOCK = 4096        # symbols per side-car block = one K7 group
SEG = 64            # symbols per segment = one K7 lane
STAGED_MAX = 4608   # K7 stages a block's compressed span in LDS when it is at most this long
LUT_BITS_MAX = 12   # the direct table's index; longer codes take the miss path
PAIR_BITS_MAX = 10  # the pair table's index

REC = np.dtype([("start", "<u8"), ("run", "<u2", (8,))])
assert REC.itemsize == 24


def expected_table(data, length, first_bit, flags=0):
    """the table image of `data` coded with `length[]`, its first code at bit `first_bit` of the buffer"""
    n = data.size
    nb = -(-n // 4096)
    cum = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(length, dtype=np.int64)[data], out=cum[1:])
    rec = np.zeros(nb, dtype=REC)
    rec["start"] = first_bit + cum[0:n:4096][:nb]
    edges = np.minimum(np.arange(nb * 8 + 1, dtype=np.int64) * 512, n)
    runs = np.diff(cum[edges]).reshape(nb, 8)
    assert runs.max(initial=0) <= 0xFFFF
    rec["run"] = runs
    hdr = b"GHFSEEK1" + struct.pack("<IIQIIQ", 1, flags, n, 4096, 512, nb)
    return np.frombuffer(hdr + bytes(64 - len(hdr)) + rec.tobytes(), dtype=np.uint8).copy()


# ---------------------------------------------------------------- K7's choice, restated
def decoder_class(min_len, max_len):
    """-> (variant, pair_bits): the hot loop K7 runs for a code with these lengths, and the pair table's index bits"""
    assert 1 <= min_len <= max_len <= 32
    if 2 * max_len <= PAIR_BITS_MAX:
        return 0, 2 * max_len  # pair table
    if max_len <= 8:
        return 1, 0            # K = 4
    if max_len <= 10:
        return 2, 0            # K = 3
    if max_len <= LUT_BITS_MAX:
        return 3, 0            # K = 2
    if max_len <= 16:
        return 4, 0            # K = 2 with the miss path
    return 5, 0                # K = 1 with the miss path


# ---------------------------------------------------------------- the worlds
NONSTAT_RUN = (40777, 5 * BLOCK)  # (first symbol, symbols) of the stretch of `nonstat` that the code does not fit


def _nonstat():
    data = dg.weighted_bytes(200000, dg.thresholds_from_probs([16, 8, 4, 2, 1]), seed=11, values=[65, 66, 67, 68, 69])
    a, k = NONSTAT_RUN
    run = (100 + dg.uniform_bytes(k, seed=12).astype(np.int64) % 200) % 256  # 100 .. 299, wrapping past 255
    data[a : a + k] = run.astype(np.uint8)
    return data


_BUILDERS = {
    "pair5": lambda: dg.make("sym16", 200005, seed=1),
    "pair2": lambda: dg.counts_to_bytes([150000, 9], seed=84),
    "len8": lambda: dg.make("uniform", 200011, seed=2) % np.uint8(128),
    "len9": lambda: dg.make("uniform", 200003, seed=3),
    "len12": lambda: dg.make("zipf", 200007, seed=5),
    "len14": lambda: dg.make("text", 200001, seed=4),
    "len22": lambda: CASES["fib22"](),
    "nonstat": _nonstat,
}
WORLDS = list(_BUILDERS)

# name -> (min_len, max_len, largest block in bits, variant, pair_bits), as the oracle gives them; asserted, not only
# printed, by tests/test_range_worlds_cpu.py.  (To the nearest byte the blocks are 2083, 512, 3589, 4099, 3044, 2436, 1367
# and 5778 bytes long.)
EXPECTED = {
    "pair5": (4, 5, 16662, 0, 10),
    "pair2": (1, 2, 4098, 0, 4),
    "len8": (7, 8, 28711, 1, 0),
    "len9": (8, 9, 32791, 2, 0),
    "len12": (2, 12, 24348, 3, 0),
    "len14": (3, 14, 19490, 4, 0),
    "len22": (1, 22, 10939, 5, 0),
    "nonstat": (1, 13, 46228, 4, 0),
}
LARGEST_BLOCK_BYTES = {"pair5": 2083, "pair2": 512, "len8": 3589, "len9": 4099, "len12": 3044, "len14": 2436, "len22": 1367,
                       "nonstat": 5778}


class World:
    """one input and what the oracle says about it"""

    def __init__(self, name):
        self.name = name
        self.data = np.ascontiguousarray(_BUILDERS[name](), dtype=np.uint8)
        self.n = int(self.data.size)
        self.nb = -(-self.n // BLOCK)
        code = orc.build_code(orc.histogram(self.data))
        self.length = [int(v) for v in code.length]
        self.min_len, self.max_len = int(code.min_len), int(code.max_len)
        self.stream = orc.compress(self.data)
        self.stream_bytes = int(self.stream.size)
        self.first_bit = 8 * int(orc.header_bytes(code).size)
        self.sym_len = np.asarray(self.length, dtype=np.int64)[self.data]  # bits of every symbol's code
        cum = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.sym_len, out=cum[1:])
        edges = np.minimum(np.arange(self.nb + 1, dtype=np.int64) * BLOCK, self.n)
        self.block_bits = np.diff(cum[edges])
        self.block_bytes = (self.block_bits + 7) // 8  # compressed bytes of every block of 4096 symbols, rounded up
        self.variant, self.pair_bits = decoder_class(self.min_len, self.max_len)

    def table(self, flags=0):
        return expected_table(self.data, self.length, self.first_bit, flags)

    def block_count_above(self, bits):
        """per block: how many of its codes are longer than `bits`"""
        long = (self.sym_len > bits).astype(np.int64)
        pad = np.zeros(self.nb * BLOCK, dtype=np.int64)
        pad[: self.n] = long
        return pad.reshape(self.nb, BLOCK).sum(axis=1)

    # ---- the ranges
    def fixed_pairs(self):
        """the fixed pairs of test_gpu_seek.range_pairs (test_range_worlds_cpu holds the two lists against each other)"""
        n = self.n
        return [
            (4096 * 5, 10000), (4096 * 5 + 100, 10000),            # block-aligned / unaligned start
            (0, 10), (4096 * 7, 33), (4096 * 7 + 3, 40),          # end inside the first segment of a block
            (1000, 5017), (4096 * 2, 4096 + 77),                   # end inside a segment
            (100, 64 * 50 - 100), (4096 * 9, 64 * 3),              # end on a segment end
            (100, 4096 * 3 - 100), (4096, 8192), (4096 * 4 + 64, 4096 - 64),  # end on a block end
            (4096 * 3 + 70, 20), (64 * 11 + 1, 62),                # inside one segment
            (0, 1), (4095, 1), (4096, 1), (n - 1, 1),              # count 1
            (0, n),                                                # the whole stream
            (n - 5000, 5000), (n - 2 * 4096 - 1, 2 * 4096 + 1), (n - 64, 64), (n - 4096, 4096),  # ending at n
        ]

    def random_pairs(self, count=40):
        seed = 20240607 + 1000 * WORLDS.index(self.name)
        out = []
        for i in range(count):
            a, b = (int(v) for v in dg.splitmix64(np.array([seed + 2 * i, seed + 2 * i + 1], dtype=np.uint64)))
            first = a % self.n
            out.append((first, 1 + b % min(self.n - first, 20000)))
        return out

    def hot_pairs(self):
        """ranges that reach a hot pass of K7 when the output pointer is 16-byte aligned"""
        n, nb = self.n, self.nb
        return [
            (4096 * 3, 4096 * 6),
            (4096 * 2 + 16 * 9, 4096 * 5 + 1000),   # a head, then hot K7
            (4096 * 5, 4096 * 4 + 33),              # the end falls inside a segment
            (0, n),
            (4096 * (nb - 6), n - 4096 * (nb - 6)),
        ]

    def extra_pairs(self):
        n, nb = self.n, self.nb
        out = [
            (4096 * 3 + 5, 4096 * 4),                                              # the cold twin of hot_pairs()[0]
            (4096 * (nb - 1), n - 4096 * (nb - 1)), (4096 * (nb - 1) + 3, n - 4096 * (nb - 1) - 3),  # the last, partial block alone
        ]
        if self.name == "nonstat":
            out += self.unstaged_pairs()
        return out

    def unstaged_pairs(self):
        """`nonstat` only: over, into and out of the stretch whose blocks do not fit K7's staged span"""
        return [
            (4096 * 8, 4096 * 9),          # blocks 8 .. 16: all of the stretch
            (4096 * 11 + 777, 9000),       # begins inside it (777 % 16 != 0): the head reads an oversized block
            (4096 * 7 + 100, 4096 * 4),    # ends inside it
        ]

    def pairs(self):
        out = self.fixed_pairs() + self.random_pairs() + self.hot_pairs() + self.extra_pairs()
        for first, count in out:
            assert 0 <= first and 1 <= count and first + count <= self.n, (self.name, first, count)
        return out


def k7_view(first, count):
    """-> (gI, groups): the first block K7 takes for this range and the number of groups of its view (0: K7 does not run).
    The view's last group always takes the cold path; the ones in front of it are hot when everything else allows it."""
    end = first + count
    gI = first // BLOCK + (1 if first % BLOCK else 0)
    if end <= gI * BLOCK:
        return gI, 0
    return gI, -(-(end - gI * BLOCK) // BLOCK)


@functools.lru_cache(maxsize=None)
def world(name):
    return World(name)


# ---------------------------------------------------------------- the stream's tail
TAIL_KINDS = {"uniform": 21, "sym16": 22}  # kind -> seed
TAIL_N0, TAIL_WINDOW = 8200, 400


@functools.lru_cache(maxsize=None)
def tail_data(kind):
    return dg.make(kind, TAIL_N0 + TAIL_WINDOW, seed=TAIL_KINDS[kind])


@functools.lru_cache(maxsize=None)
def tail_sizes(kind):
    """-> {r: n}: for every r in 0 .. 15 that has one, the smallest n in [TAIL_N0, TAIL_N0 + TAIL_WINDOW) at which the
    oracle's stream of tail_data(kind)[:n] has stream_bytes % 16 == r.  That remainder decides how the stream's last,
    incomplete 16-byte vector is read."""
    data = tail_data(kind)
    found = {}
    for n in range(TAIL_N0, TAIL_N0 + TAIL_WINDOW):
        r = int(orc.compress(data[:n]).size) % 16
        found.setdefault(r, n)
        if len(found) == 16:
            break
    return found
