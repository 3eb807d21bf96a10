"""GPU: ghf_decode_range and the seek table in every decoder class (tests/range_worlds.py), all bit-exact.

K7 picks one of six hot loops from the code's lengths, has a staged and an unstaged cold path, and runs a hot pass only when
its view's output pointer is 16-byte aligned; k_decode_head and k_seek_expand read the same table image in its pair-table
and its one-symbol form.  tests/test_range_worlds_cpu.py shows, without a GPU, that the worlds and ranges used here reach
each of these.  Expected outputs are slices of the input; expected streams, code lengths and tables come from the oracle."""
import ctypes as C

import numpy as np
import pytest

import pkgload
import range_worlds as rw
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

E_FORMAT, E_CORRUPT = 6, 7
GUARD = 0xA5
PAD = 256


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Packed:
    """one input compressed with an index, its stream held against the oracle's, and its table"""

    def __init__(self, ghf, ctx, torch, data, want_stream):
        self.data = data
        self.n = int(data.size)
        self.d_in = to_dev(torch, data)
        self.idx = ctx.index_alloc(self.n)
        self.d_stream, nbytes, self.d_code = ctx.compress(self.d_in, index=self.idx)
        ctx.sync()
        self.nbytes = int(nbytes.item())
        got = self.d_stream[: self.nbytes].cpu().numpy()
        assert self.nbytes == want_stream.size and np.array_equal(got, want_stream), "the stream differs from the oracle's"
        d_table = ctx.seek_pack(self.idx)
        ctx.sync()
        self.table = d_table.cpu().numpy()
        self.info = ghf.seek_parse(self.table)
        self.d_table = to_dev(torch, self.table)

    def sources(self):
        return {"index": {"index": self.idx}, "table": {"info": self.info, "d_table": self.d_table}}

    def free(self, ctx):
        ctx.index_free(self.idx)


def guarded(torch, nbytes):
    """a 256-byte aligned buffer of PAD + nbytes + PAD + 67 bytes, all GUARD"""
    buf = torch.full((nbytes + 2 * PAD + 67,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf


def guards_intact(buf, off, count):
    return bool((buf[:off] == GUARD).all()) and bool((buf[off + count :] == GUARD).all())


# ---------------------------------------------------------------- 1. every range of a world, four ways
@pytest.mark.parametrize("name", rw.WORLDS)
def test_ranges_in_every_class(env, name):
    ghf, ctx, torch = env
    w = rw.world(name)
    p = Packed(ghf, ctx, torch, w.data, w.stream)
    code = ctx.code_to_host(p.d_code)
    assert list(code.length) == w.length and (code.min_len, code.max_len) == (w.min_len, w.max_len)
    assert np.array_equal(p.table, w.table()), "first difference at byte %d" % int(np.nonzero(p.table != w.table())[0][0])
    buf = guarded(torch, w.n)
    for first, count in w.pairs():
        for source, kw in p.sources().items():
            for off in (PAD, PAD + 67):  # a 16-byte aligned and an odd output pointer
                buf.fill_(GUARD)
                out = buf[off : off + count]
                assert out.data_ptr() % 16 == (0 if off == PAD else 3)
                ctx.decode_range(p.d_stream, p.nbytes, p.d_code, first, count, d_out=out, **kw)
                ctx.sync()
                where = (name, source, first, count, off)
                assert torch.equal(out, p.d_in[first : first + count]), where
                assert guards_intact(buf, off, count), where
    if name in ("nonstat", "len22"):  # the whole stream through the side-car that k_seek_expand rebuilt
        idx2 = ctx.seek_expand(p.info, p.d_table, p.d_stream, p.nbytes, p.d_code)
        buf.fill_(GUARD)
        back, nout = ctx.decode(p.d_stream, p.nbytes, p.d_code, idx2, d_out=buf[PAD : PAD + w.n])
        ctx.sync()
        assert int(nout.item()) == w.n and torch.equal(back, p.d_in)
        assert guards_intact(buf, PAD, w.n)
        ctx.index_free(idx2)
    p.free(ctx)


# ---------------------------------------------------------------- 2. a GHF_EMIT_REBASE shard: no end mark behind its last symbol
@pytest.mark.parametrize("name", ["pair5", "len22"])
def test_rebased_shard_ranges(env, name):
    """as test_gpu_seek.test_rebased_shard_keeps_its_flag, in the pair-table class and in the one with the longest codes"""
    ghf, ctx, torch = env
    w = rw.world(name)
    d_in = to_dev(torch, w.data)
    d_code = ctx.build_code(ctx.histogram(d_in))
    assert list(ctx.code_to_host(d_code).length) == w.length
    ctx.encode_plan(d_in, d_code)
    S = 128 * 77777 + 37
    start = torch.tensor([S], dtype=torch.int64, device="cuda")
    idx = ctx.index_alloc(w.n)
    d_out = torch.zeros(ghf.shard_bound(w.n), dtype=torch.uint8, device="cuda")
    end = ctx.encode_emit(d_in, d_code, d_out, start_bit=start, flags=ghf.EMIT_REBASE, index=idx)  # no GHF_EMIT_LAST
    ctx.sync()
    idx.flags = ghf.INDEX_NO_END_MARK
    nbytes = int(end[1].item())
    d_table = ctx.seek_pack(idx)
    ctx.sync()
    table = d_table.cpu().numpy()
    ctx.index_free(idx)
    assert np.array_equal(table, rw.expected_table(w.data, w.length, S % 128, flags=ghf.INDEX_NO_END_MARK))
    info = ghf.seek_parse(table)
    assert info.flags == ghf.INDEX_NO_END_MARK
    buf = guarded(torch, w.n)
    for first, count in ((w.n - 7000, 7000), (4096 * 3, w.n - 4096 * 3)):
        for off in (PAD, PAD + 67):
            buf.fill_(GUARD)
            out = buf[off : off + count]
            ctx.decode_range(d_out, nbytes, d_code, first, count, info=info, d_table=d_table, d_out=out)
            ctx.sync()
            assert torch.equal(out, d_in[first : first + count]), (name, first, count, off)
            assert guards_intact(buf, off, count), (name, first, count, off)


# ---------------------------------------------------------------- 3. the stream's tail
@pytest.mark.parametrize("kind", sorted(rw.TAIL_KINDS))
def test_nothing_behind_the_stream_is_read(env, kind):
    """stream_bytes % 16 takes every value 0 .. 15; what lies behind the stream (zeros in one buffer, 0xFF in the other)
    must not change a range that ends at n"""
    ghf, ctx, torch = env
    sizes = rw.tail_sizes(kind)
    assert sorted(sizes) == list(range(16))
    data = rw.tail_data(kind)
    for r, n in sorted(sizes.items()):
        piece = np.ascontiguousarray(data[:n])
        want = orc.compress(piece)
        assert want.size % 16 == r
        p = Packed(ghf, ctx, torch, piece, want)
        for fill in (0x00, 0xFF):
            d_stream = torch.full((p.nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
            assert d_stream.data_ptr() % 16 == 0
            d_stream[: p.nbytes] = p.d_stream[: p.nbytes]
            for first, count in ((n - 5000, 5000), (4096, n - 4096), (n - 1, 1)):
                for source, kw in p.sources().items():
                    out = ctx.decode_range(d_stream, p.nbytes, p.d_code, first, count, **kw)
                    ctx.sync()
                    assert torch.equal(out[:count], p.d_in[first : first + count]), (kind, r, n, fill, source, first, count)
        p.free(ctx)


# ---------------------------------------------------------------- 4. a side-car that lies, seen by every hot loop
def lying_copy(ghf, torch, ctx, idx, lane):
    """the live index copied between guard bytes, the end of segment `lane` of block 4 one bit late -> (fake index, keep-alive)"""
    chunk, seg = ctx.index_to_host(idx)
    seg = seg.copy()
    seg[4 * 64 + lane] += 1
    cb = torch.full((PAD + chunk.nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    sb = torch.full((PAD + seg.nbytes + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    cb[PAD : PAD + chunk.nbytes] = to_dev(torch, chunk.view(np.uint8))
    sb[PAD : PAD + seg.nbytes] = to_dev(torch, seg.view(np.uint8))
    fake = ghf.Index()
    C.memmove(C.byref(fake), C.byref(idx), C.sizeof(ghf.Index))
    fake.d_chunk_bit = cb.data_ptr() + PAD
    fake.d_seg_bit = sb.data_ptr() + PAD
    return fake, (cb, sb, cb.clone(), sb.clone())


@pytest.mark.parametrize("lane", [20, 63])
@pytest.mark.parametrize("name", rw.WORLDS)
def test_lying_side_car_is_caught_by_the_hot_loop(env, name, lane):
    """The lane of block 4 starts where it should and decodes its true 64 symbols, so it consumes one bit fewer than the
    side-car claims: K7's end-to-end check of a segment must fire in whichever hot loop the class runs (block 4 is a
    whole block in front of the view's last group and the output is 16-byte aligned).  Behind segment 20 lane 21 starts
    one bit late and decodes other symbols than were written, which in a small alphabet (pair5) soon include the end mark:
    a second witness.  Behind segment 63 nobody starts -- the next block has its own start bit -- so there the segment's
    own check is the only one that can notice.  Ordinary runs, each done once."""
    import test_gpu_seek as seek

    ghf, ctx, torch = env
    w = rw.world(name)
    assert w.block_bytes[4] <= 4576 and w.nb > 9
    p = Packed(ghf, ctx, torch, w.data, w.stream)
    fake, (cb, sb, cb0, sb0) = lying_copy(ghf, torch, ctx, p.idx, lane)
    first, count = 4096 * 3, 4096 * 6
    buf = guarded(torch, w.n)

    def harmless(nbytes):
        return guards_intact(buf, PAD, nbytes) and torch.equal(cb, cb0) and torch.equal(sb, sb0)

    out = buf[PAD : PAD + count]
    assert out.data_ptr() % 16 == 0
    st = seek._status_of(ghf, ctx, lambda: ctx.decode_range(p.d_stream, p.nbytes, p.d_code, first, count, index=fake, d_out=out))
    assert st == E_CORRUPT, st
    assert harmless(count)
    buf.fill_(GUARD)
    ctx.decode_range(p.d_stream, p.nbytes, p.d_code, first, count, index=p.idx, d_out=out)
    ctx.sync()
    assert torch.equal(out, p.d_in[first : first + count]) and harmless(count)
    # ... and the whole stream
    buf.fill_(GUARD)
    whole = buf[PAD : PAD + w.n]
    st = seek._status_of(ghf, ctx, lambda: ctx.decode(p.d_stream, p.nbytes, p.d_code, fake, d_out=whole))
    assert st == E_CORRUPT, st
    assert harmless(w.n)
    buf.fill_(GUARD)
    back, nout = ctx.decode(p.d_stream, p.nbytes, p.d_code, p.idx, d_out=whole)
    ctx.sync()
    assert int(nout.item()) == w.n and torch.equal(back, p.d_in) and harmless(w.n)
    p.free(ctx)


@pytest.mark.parametrize("what", ["run_plus_1", "start_plus_8"])
@pytest.mark.parametrize("name", ["pair5", "len12", "len22"])
def test_damaged_table_in_other_classes(env, name, what):
    """the table damages of test_gpu_seek.test_corrupted_table_is_reported_and_harms_nothing (blocks 5 and 7) through
    decode_range, where k_seek_expand reads a pair table, a full 12-bit table and one with codes beyond it"""
    import test_gpu_seek as seek

    ghf, ctx, torch = env
    w = rw.world(name)
    p = Packed(ghf, ctx, torch, w.data, w.stream)
    bad = seek._corrupt(p.table, what)
    assert bad.size == p.table.size and not np.array_equal(bad, p.table)
    d_bad = to_dev(torch, bad)
    first, count = 4096 * 3 + 5, 4096 * 10
    assert first + count <= w.n
    buf = guarded(torch, count)
    out = buf[PAD : PAD + count]
    st = seek._status_of(ghf, ctx, lambda: ctx.decode_range(p.d_stream, p.nbytes, p.d_code, first, count, info=p.info,
                                                            d_table=d_bad, d_out=out, table_bytes=bad.size))
    assert st in (E_CORRUPT, E_FORMAT), st
    assert guards_intact(buf, PAD, count)
    # the context is usable again: the intact table decodes the same range
    buf.fill_(GUARD)
    ctx.decode_range(p.d_stream, p.nbytes, p.d_code, first, count, info=p.info, d_table=p.d_table, d_out=out)
    ctx.sync()
    assert torch.equal(out, p.d_in[first : first + count]) and guards_intact(buf, PAD, count)
    p.free(ctx)
