"""CPU: tests/shard_model.py -- the expected-value model of tests/test_gpu_shard_bits.py -- checked against the reference.
Composing the model's shards at any cut gives exactly the single-stream .crs2 of the oracle (the C restatement of the
reference) and the SHA-256 that golden.json recorded from the compiled reference; the model's packer agrees with the
oracle's orc_pack_at at every bit phase."""
import ctypes as C

import numpy as np
import pytest

import shard_model as sm
from cases import CASES
from oracle import oracle as orc


def cuts_for(name, n):
    cuts = {"w2": sm.cuts_even(n, 2), "w8": sm.cuts_even(n, 8), "w8_random": sm.cuts_random(n, 8, seed=n)}
    if n <= 64:
        cuts["w_n+1"] = sm.cuts_random(n, n + 1, seed=1)
        cuts["w_n+3"] = sm.cuts_random(n, n + 3, seed=3)
    return cuts


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_shards_compose_to_the_reference_stream(name, golden):
    data = CASES[name]()
    code = orc.build_code(orc.histogram(data))
    ref = orc.compress(data)
    assert sm.sha256(ref) == golden[name]["crs2_sha256"]
    assert np.array_equal(sm.header_bytes(code), orc.header_bytes(code))
    for label, cuts in cuts_for(name, data.size).items():
        stream, shards = sm.stream_from_cuts(data, code, cuts)
        assert stream.size == ref.size and np.array_equal(stream, ref), (name, label)
        assert sm.sha256(stream) == golden[name]["crs2_sha256"], (name, label)
        world = len(cuts) - 1
        totals = [sm.body_bits(data[cuts[g] : cuts[g + 1]], code) for g in range(world)]
        for g, (S, origin, buf, (end, nbytes)) in enumerate(shards):
            assert nbytes == buf.size
            assert nbytes <= sm.shard_bytes(code, totals, world, g) <= nbytes + 16
            assert sm.min_cap(S, end, origin) <= sm.shard_bytes(code, totals, world, g)


def test_cuts_hold_the_empty_shards_the_gpu_tests_want():
    c = sm.cuts_random(1000, 8, seed=5)
    sizes = np.diff(c)
    assert c[0] == 0 and c[-1] == 1000 and sizes[0] == 0 and sizes[4] == 0 and sizes[-1] == 0
    for n in (1, 2, 3, 7, 8):
        for w in (n + 1, n + 3):
            sizes = np.diff(sm.cuts_random(n, w, seed=w))
            assert sizes.sum() == n and sizes[0] == 0 and (sizes[-1] == 0 or w == 2)


@pytest.mark.parametrize("name", ["zipf_64k", "fib32_maxlen32", "aaaabbc", "uniform_4k"])
def test_model_packer_equals_orc_pack_at(name):
    data = CASES[name]()[:5000]
    code = orc.build_code(orc.histogram(CASES[name]()))
    bits = sm.code_bits(data, code)
    for S in (8 * 1296 + 0, 8 * 1296 + 3, (1 << 38) + 7, 275_000_000_005):
        for last in (0, 1):
            buf, (end, nbytes) = sm.expected_shard(data, code, S, rebase=True, last=bool(last), bits=bits)
            ref = np.zeros(bits.size // 8 + 64, dtype=np.uint8)
            nb = orc.lib().orc_pack_at(data.ctypes.data, data.size, C.byref(code), S & 7, last, ref.ctypes.data, ref.size)
            assert end == S + nb
            off = (S >> 3) - 16 * (S >> 7)
            assert not buf[:off].any()
            assert np.array_equal(buf[off:], ref[: nbytes - off]), (name, S, last)


def test_index_model_by_hand():
    """three blocks of 4096 one- and two-bit codes: chunk_bit counts from the buffer's byte 0, seg_bit from the block"""
    code = orc.build_code(orc.histogram(np.array([0] * 10 + [1] * 5 + [2], dtype=np.uint8)))
    t = sm.tables(code)
    data = np.array(([0, 1] * 3000 + [2] * 2300)[:8300], dtype=np.uint8)
    S = (1 << 35) + 77
    origin = 16 * (S >> 7)
    chunk_bit, seg_bit = sm.expected_index(data, code, S, origin)
    lens = [t.lens[v] for v in data.tolist()]
    assert chunk_bit.tolist() == [S - 8 * origin + sum(lens[: 4096 * b]) for b in range(3)]
    assert seg_bit.tolist() == [sum(lens[4096 * (s // 64) : min(64 * (s + 1), data.size)]) for s in range(-(-data.size // 64))]
