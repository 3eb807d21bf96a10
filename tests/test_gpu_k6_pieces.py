"""GPU: K6 on canonical codes, the cases of tests/k6_pieces.py -- pieces at every seam of their own, every true entry bit,
wrong entry bits (below and beyond the stride of the scan's function rows), the end mark against K6's edges and whole
.crs2 images at the levels of the scan.

Nothing expected comes from the library: every (landing, n_symbols, has_end_mark) is the model's, every body and image the
oracle's (tests/test_k6_pieces_cpu.py holds the model to the oracle and asserts what the cases cover).  Every output sits
between guard bytes that are checked afterwards.

The ids are per code and tier, `<shape>/<min>-<max>`; a failure names the stream and the piece, e.g. `cls8/8-9 :: C/run,
bytes [3, 6147), first_bit 16`: k6_pieces.by_label() and the tier's function give that case alone."""
import numpy as np
import pytest

import k6_pieces as kp
import pkgload
from guarded import GUARD, Arena, first_diff
from test_gpu_crs_sweep import Streams, sync_status, to_dev

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_CAP = 0, 1, 5
CODES = kp.codes()
by_code = pytest.mark.parametrize("code", CODES, ids=[c.label for c in CODES])


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


@pytest.fixture(scope="module", autouse=True)
def warm(env):
    """the first launch of a kernel loads its code object: a class code and a long one run here, so that no id's time
    depends on the order in which the ids run.  Plain calls: nothing is compared here."""
    ghf, ctx, torch = env
    for label in ("cls8/8-9", "long32/1-32"):
        code = kp.by_label(label)
        d_code = device_code(torch, code)
        for p in kp.tier_b(code)[:2]:
            buf, piece_bytes = kp.piece_buffer(p.stream, p.lo, p.hi, "plus16")
            d_piece = to_dev(torch, buf)
            ctx.sync_piece(d_piece, piece_bytes, p.first_bit, 8 * (p.hi - p.lo), d_code)
            ctx.decode(d_piece, piece_bytes, d_code, None, cap=8 * (p.hi - p.lo) + 64)
    sync_status(ghf, ctx)


@pytest.fixture(autouse=True)
def clean_status(env):
    """a failed id leaves no latched status behind for the next one"""
    yield
    ghf, ctx, torch = env
    torch.cuda.synchronize()
    ctx.L.ghf_clear_status(ctx.h)


def device_code(torch, code):
    t = torch.from_numpy(np.frombuffer(bytes(code.entry.code), dtype=np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def where(p):
    return "%r, bytes [%d, %d), first_bit %d" % (p.stream, p.lo, p.hi, p.first_bit)


def same(got, want):
    """the triple of a call against the model's: landing is left out where the model defines none"""
    return got[1:] == (want.n_symbols, bool(want.has_end_mark)) and (want.landing is None or got[0] == want.landing)


def sync(env, d_piece, piece_bytes, first_bit, end_bit, d_code, what):
    ghf, ctx, torch = env
    try:
        return ctx.sync_piece(d_piece, piece_bytes, first_bit, end_bit, d_code)
    except ghf.GhfError as e:  # (K6 reports to the host at once)
        raise AssertionError((what, "first_bit %d" % first_bit, str(e)))


# ------------------------------------------------------------------------------------------------ tier A: true chains
def chain(env, d_code, ch, layout):
    """ghf_sync_piece + ghf_decode(index = NULL) piece by piece, the outputs back to back in one guarded region; the piece
    whose end_bit is 0 is synchronised and not decoded"""
    ghf, ctx, torch = env
    s = ch.stream
    a = Arena()
    r = a.add(s.n + 1, skew=ch.skew)  # (one byte more than anything writes: a piece of no symbols is handed a byte of room)
    a.alloc(torch)
    d_out, at = a.view(r), 0
    nbs = torch.full((len(ch.pieces),), -1, dtype=torch.int64, device="cuda")
    for k, p in enumerate(ch.pieces):
        buf, piece_bytes = kp.piece_buffer(s, p.lo, p.hi, layout)
        d_piece = to_dev(torch, buf)
        assert d_piece.data_ptr() % 16 == 0
        end_bit = 8 * (p.hi - p.lo)
        got = sync(env, d_piece, piece_bytes, p.first_bit, end_bit, d_code, (where(p), layout))
        assert same(got, p.want), (where(p), layout, got, tuple(p.want))
        if end_bit:
            nsym = p.want.n_symbols
            ctx.decode(d_piece, piece_bytes, d_code, None, d_out=d_out[at : at + max(nsym, 1)], nbytes=nbs[k : k + 1])
            at += nsym
    assert at == s.n
    status = sync_status(ghf, ctx)
    assert status == OK, (s, layout, "latched status", status)
    assert a.fetch(), (s, layout, "guard bytes")
    assert nbs.cpu().tolist() == [p.want.n_symbols if p.hi > p.lo else -1 for p in ch.pieces], (s, layout)
    got = a.got(r)
    assert np.array_equal(got[: s.n], s.data), (s, layout, first_diff(got[: s.n], s.data))
    assert got[s.n] == GUARD, (s, layout)


@by_code
def test_true_chains(env, code):
    ghf, ctx, torch = env
    d_code = device_code(torch, code)
    for ch in kp.tier_a(code):
        for layout in kp.LAYOUTS:
            chain(env, d_code, ch, layout)


# ------------------------------------------------------------------------------------------- tier B: every entry bit
def entry_bits(env, code, pieces):
    ghf, ctx, torch = env
    d_code = device_code(torch, code)
    a = Arena()
    regions = [a.add(p.want.n_symbols, skew=(3 * i + p.first_bit) % 16) for i, p in enumerate(pieces)]
    a.alloc(torch)
    nbs = torch.full((len(pieces),), -1, dtype=torch.int64, device="cuda")
    for k, p in enumerate(pieces):
        buf, piece_bytes = kp.piece_buffer(p.stream, p.lo, p.hi, kp.LAYOUTS[k % 2])
        d_piece = to_dev(torch, buf)
        got = sync(env, d_piece, piece_bytes, p.first_bit, 8 * (p.hi - p.lo), d_code, where(p))
        assert same(got, p.want), (where(p), got, tuple(p.want))
        ctx.decode(d_piece, piece_bytes, d_code, None, d_out=a.view(regions[k]), nbytes=nbs[k : k + 1])
    status = sync_status(ghf, ctx)
    assert status == OK, (code, "latched status", status)
    assert a.fetch(), (code, "guard bytes")
    assert nbs.cpu().tolist() == [p.want.n_symbols for p in pieces], code
    for p, r in zip(pieces, regions):
        want = p.stream.symbols(p.lo, p.first_bit, p.want.n_symbols)
        assert np.array_equal(a.got(r), want), (where(p), first_diff(a.got(r), want))


@by_code
def test_every_true_entry_bit(env, code):
    pieces = kp.tier_b(code)
    assert [p.first_bit for p in pieces] == list(range(code.max_len))
    entry_bits(env, code, pieces)


# --------------------------------------------------------------------------------------------- tier C: wrong guesses
@by_code
def test_wrong_guesses(env, code):
    """a wrong first_bit gives the model's triple from that bit -- never "did not converge" --, and the true first_bit on
    the same buffer gives the true triple again: the side-car a call rebuilt does not outlive it.  The decode behind the
    last, true call gives the piece's symbols."""
    ghf, ctx, torch = env
    d_code = device_code(torch, code)
    cases = kp.tier_c(code)
    pieces = list(dict.fromkeys((g.kind, g.lo, g.hi) for g in cases))
    a = Arena()
    regions = {key: a.add(next(g for g in cases if (g.kind, g.lo, g.hi) == key).true_want.n_symbols, skew=i % 16) for i, key in enumerate(pieces)}
    a.alloc(torch)
    for key in pieces:
        mine = [g for g in cases if (g.kind, g.lo, g.hi) == key]
        g0 = mine[0]
        buf, piece_bytes = kp.piece_buffer(g0.stream, g0.lo, g0.hi, "plus16")
        d_piece = to_dev(torch, buf)
        end_bit = 8 * (g0.hi - g0.lo)
        what = "%r, bytes [%d, %d), true first_bit %d" % (g0.stream, g0.lo, g0.hi, g0.true_first)
        for g in mine:
            got = sync(env, d_piece, piece_bytes, g.guess, end_bit, d_code, what)
            assert same(got, g.want), (what, "first_bit %d" % g.guess, got, tuple(g.want))
            got = sync(env, d_piece, piece_bytes, g.true_first, end_bit, d_code, what)
            assert same(got, g.true_want), (what, "the true first_bit behind first_bit %d" % g.guess, got, tuple(g.true_want))
        ctx.decode(d_piece, piece_bytes, d_code, None, d_out=a.view(regions[key]))
    status = sync_status(ghf, ctx)
    assert status == OK, (code, "latched status", status)
    assert a.fetch(), (code, "guard bytes")
    for key in pieces:
        g0 = next(g for g in cases if (g.kind, g.lo, g.hi) == key)
        want = g0.stream.symbols(g0.lo, g0.true_first, g0.true_want.n_symbols)
        assert np.array_equal(a.got(regions[key]), want), (g0.stream, key, first_diff(a.got(regions[key]), want))


# ---------------------------------------------------------------------- tiers D and E: the whole-stream calls (and the last piece)
def whole(env, code, items, as_piece):
    """items: [(name, image bytes, data)].  ghf_decoded_size, ghf_decode(index = NULL), and a cap of n - 1: GHF_E_CAP and
    nothing stored; as_piece: the body alone as a stream's only piece as well"""
    ghf, ctx, torch = env
    d_code = device_code(torch, code)
    hdr = int(code.entry.header.size)
    files = Streams(torch, [raw for _, raw, _ in items])
    a, plan = Arena(), []
    for i, (_, raw, data) in enumerate(items):
        plan.append((a.add(data.size, skew=i % 16), a.add(data.size, skew=(i + 5) % 16), a.add(data.size, skew=(i + 11) % 16) if as_piece else None))
    a.alloc(torch)
    nbs = torch.full((len(items), 3), -1, dtype=torch.int64, device="cuda")
    for i, ((name, raw, data), (r_all, r_cap, r_piece)) in enumerate(zip(items, plan)):
        n = int(data.size)
        d_file = files.view(i)
        try:
            size = ctx.decoded_size(d_file, raw.size, d_code)
            assert size == n, (code, name, "ghf_decoded_size", size, n)
            ctx.decode(d_file, raw.size, d_code, None, d_out=a.view(r_all), nbytes=nbs[i, 0:1])
        except ghf.GhfError as e:
            raise AssertionError((code, name, str(e)))
        rc = ctx.L.ghf_decode(ctx.h, d_file.data_ptr(), raw.size, d_code.data_ptr(), None, a.view(r_cap).data_ptr(), n - 1, nbs[i, 1:2].data_ptr())
        assert rc == E_CAP, (code, name, "a cap of n - 1", rc)
        ctx.L.ghf_clear_status(ctx.h)
        if as_piece:
            body = raw[hdr:]
            buf = np.zeros((body.size + 16 + 15 & ~15) + 16, dtype=np.uint8)
            buf[: body.size] = body
            d_piece = to_dev(torch, buf)
            got = sync(env, d_piece, buf.size, 0, 8 * body.size, d_code, (code, name, "the body as the last piece"))
            assert got[1:] == (n, True), (code, name, "the body as the last piece", got)
            ctx.decode(d_piece, buf.size, d_code, None, d_out=a.view(r_piece), nbytes=nbs[i, 2:3])
    status = sync_status(ghf, ctx)
    assert status == OK, (code, "latched status", status)
    assert a.fetch(), (code, "guard bytes")
    h_nbs = nbs.cpu().tolist()
    for (name, raw, data), (r_all, r_cap, r_piece), nb in zip(items, plan, h_nbs):
        assert nb == [data.size, -1, data.size if as_piece else -1], (code, name, nb)
        assert np.array_equal(a.got(r_all), data), (code, name, first_diff(a.got(r_all), data))
        assert (a.got(r_cap) == GUARD).all(), (code, name, "a refused decode stored something")
        if as_piece:
            assert np.array_equal(a.got(r_piece), data), (code, name, "as a piece", first_diff(a.got(r_piece), data))


@by_code
def test_the_end_mark_at_the_edges_of_k6(env, code):
    whole(env, code, [(m.stream.name, m.stream.image, m.stream.data) for m in kp.tier_d(code)], as_piece=True)


@by_code
def test_whole_streams_at_the_levels_of_the_scan(env, code):
    items = [("%s%s" % (im.stream.name, " + %d stale bytes" % im.stale if im.stale else ""), kp.image_bytes(im), im.stream.data)
             for im in kp.tier_e(code)]
    whole(env, code, items, as_piece=False)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals(env):
    """each returns GHF_E_INVAL at once; with the status cleared, the next call on the same context gives the piece's triple"""
    import ctypes as C

    ghf, ctx, torch = env
    code = kp.by_label("direct/1-12")
    d_code = device_code(torch, code)
    p = kp.tier_b(code)[3]
    buf, piece_bytes = kp.piece_buffer(p.stream, p.lo, p.hi, "plus16")
    d_piece = to_dev(torch, buf)
    end_bit = 8 * (p.hi - p.lo)

    def call(ptr, nbytes, first_bit, end):
        landing, n, eof = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
        rc = ctx.L.ghf_sync_piece(ctx.h, ptr, nbytes, first_bit, end, d_code.data_ptr(), C.byref(landing), C.byref(n), C.byref(eof))
        ctx.L.ghf_clear_status(ctx.h)
        return rc

    for what, args in (("first_bit == 512", (d_piece.data_ptr(), piece_bytes, 512, end_bit)),
                       ("first_bit > end_bit", (d_piece.data_ptr(), piece_bytes, 9, 8)),
                       ("end_bit > 8 * piece_bytes", (d_piece.data_ptr(), piece_bytes, p.first_bit, 8 * piece_bytes + 1)),
                       ("an unaligned d_piece", (d_piece.data_ptr() + 1, piece_bytes - 1, p.first_bit, end_bit))):
        assert call(*args) == E_INVAL, what
        got = sync(env, d_piece, piece_bytes, p.first_bit, end_bit, d_code, where(p))
        assert same(got, p.want), (what, "the call behind it", got)
    entry_bits(env, code, [p])
