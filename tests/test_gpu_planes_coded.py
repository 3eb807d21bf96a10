"""GPU: the staged byte-plane calls for one large typed tensor (ghf_histogram_planes / ghf_planes_image_bytes /
ghf_compress_planes_coded).

Expected values come from numpy slicing (plane p of x is x[p::E]) and from the oracle (oracle.histogram / build_code /
compress / header_bytes / body_bits / decompress) alone; the body under a code that was trained on another tensor is packed
here from the oracle's code table."""

import numpy as np
import pytest

import datagen as dg
import pkgload
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

E_INVAL, E_EMPTY, E_CAP, E_FORMAT, E_NOCODE = 1, 3, 5, 6, 10
GUARD = 0xA5
GUARD_WORD = -0x5A5A5A5A5A5A5A5B
WIDTHS = (2, 4, 8)
HIST_N = (1, 15, 16, 17, 4095, 4097, 65536 + 3)
COMPRESS_N = (1, 64, 4097, 65536 + 3)


def hist_geom():
    """(G, TILE, FLUSH) as the binding exports them from ghf_internal.h: k_histogram_planes runs G persistent workgroups over
    tiles of TILE bytes of the interleaved buffer and moves a workgroup's u32 counters into its u64 sums every FLUSH tiles.
    Every size below follows them, so a retuned kernel moves the cases with it."""
    ghf = pkgload.load().ghf
    return ghf.PLANES_HIST_GROUPS, ghf.PLANES_HIST_TILE_BYTES, ghf.PLANES_HIST_FLUSH_TILES


def two_round_elems(e):
    """every workgroup of the grid takes two tiles; behind them seven whole vectors and E more bytes: a ragged end"""
    g, tile, _ = hist_geom()
    return (2 * g * tile + 7 * 16 + e) // e


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ghf = pkg.ghf
    ctx = ghf.Context(0)
    yield ghf, ctx, torch
    ctx.close()


@pytest.fixture(scope="module")
def uniform():
    """one run of uniform bytes for every histogram case (two tiles for every workgroup and a few bytes)"""
    n = max(two_round_elems(e) * e for e in WIDTHS)
    assert n < 64 << 20
    a = dg.uniform_bytes(n, seed=0x504C4853)
    a.setflags(write=False)
    return a


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()  # a copy: the shared inputs stay read-only


def normal_elems(n, e, seed=7):
    """n seeded standard-normal values as bytes: bf16 (the upper half of the fp32 value) / fp32 / fp64"""
    x = np.random.default_rng(seed).standard_normal(n)
    if e == 8:
        return x.view(np.uint8).copy()
    f = x.astype(np.float32)
    if e == 4:
        return f.view(np.uint8).copy()
    return (f.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()


_want = {}


def want_for(e, n, seed=7):
    """(bytes, [oracle image of plane p], [oracle tables of plane p]) -- computed once per case"""
    key = (e, n, seed)
    if key not in _want:
        x = normal_elems(n, e, seed)
        x.setflags(write=False)
        planes = [np.ascontiguousarray(x[p::e]) for p in range(e)]
        _want[key] = (x, [orc.compress(pl) for pl in planes], [orc.build_code(orc.histogram(pl)).as_dict() for pl in planes])
    return _want[key]


def plane_hists(x, e):
    return np.stack([orc.histogram(np.ascontiguousarray(x[p::e])) for p in range(e)])


def covered(h):
    h = h.copy()
    h[h == 0] = 1
    return h


def guarded_hists(ghf, ctx, torch, d_in, e, n, flags=0):
    """histogram_planes into the middle of a guarded buffer -> (int64[e, 257] on the host, guards untouched)"""
    buf = torch.full((e * ghf.NSYM + 16,), GUARD_WORD, dtype=torch.int64, device="cuda")
    ctx.histogram_planes(d_in, e, n_elems=n, flags=flags, out=buf[8 : 8 + e * ghf.NSYM])
    ctx.sync()
    h = buf.cpu().numpy()
    return h[8:-8].reshape(e, ghf.NSYM), bool((h[:8] == GUARD_WORD).all() and (h[-8:] == GUARD_WORD).all())


# ---------------------------------------------------------------- 1. the histograms are exact and nothing else is written
def check_hists(ghf, ctx, torch, x, e, what):
    n = x.size // e
    want = plane_hists(x, e)
    assert (want[:, 256] == 1).all()
    d_in = to_dev(torch, x)
    got, clean = guarded_hists(ghf, ctx, torch, d_in, e, n)
    assert clean, (what, n)
    assert np.array_equal(got, want), (what, n, np.argwhere(got != want)[:4])
    got, clean = guarded_hists(ghf, ctx, torch, d_in, e, n, flags=ghf.HIST_COVER_ALL)
    assert clean, (what, n)
    assert np.array_equal(got, covered(want)), (what, n)


@pytest.mark.parametrize("e", WIDTHS)
def test_plane_histograms_are_exact_between_guard_words(env, uniform, e):
    """uniform bytes, standard-normal values (at E = 2 the high plane takes a handful of values) and a constant tensor at
    every size, the one included at which every workgroup takes two tiles and one of them the ragged end"""
    ghf, ctx, torch = env
    for n in HIST_N + (two_round_elems(e),):
        check_hists(ghf, ctx, torch, uniform[: n * e], e, "uniform")
        check_hists(ghf, ctx, torch, normal_elems(n, e), e, "normal")
        # a constant tensor: every plane has one live value, every lane of a wave stands on one bin
        check_hists(ghf, ctx, torch, np.tile(np.arange(0xF1, 0xF1 + e, dtype=np.uint8), n), e, "constant")


def test_a_histogram_past_the_u32_flush_is_exact(env):
    """E = 2, one tile short of (FLUSH + 1) tiles for every workgroup plus a ragged end, just under 64 MiB: every workgroup
    but the last moves its u32 counters into its u64 sums after FLUSH tiles and then counts one tile more.  The low byte
    of element k is k % 5 and the high byte is constant, so the expected counts are arithmetic."""
    ghf, ctx, torch = env
    e = 2
    g, tile, flush = hist_geom()
    n_bytes = (g * (flush + 1) - 1) * tile + 3 * 16 + e
    assert n_bytes <= 64 << 20 and (n_bytes // tile) // g == flush
    n = n_bytes // e
    d_in = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    d_in[0::2] = (torch.arange(n, dtype=torch.int32, device="cuda") % 5).to(torch.uint8)
    d_in[1::2] = 0xEE
    got, clean = guarded_hists(ghf, ctx, torch, d_in, e, n)
    want = np.zeros((e, ghf.NSYM), dtype=np.int64)
    for v in range(5):
        want[0, v] = (n - v + 4) // 5
    want[1, 0xEE] = n
    want[:, 256] = 1
    assert want[0, :5].sum() == n
    assert clean and np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---------------------------------------------------------------- 2. GHF_PLANES_BUILD_CODES is ghf_compress_planes, byte for byte
def fetch(r):
    return r["out"].cpu().numpy(), [int(v) for v in r["out_bytes"].cpu().numpy()], r["codes"].cpu().numpy()


def check_against_oracle(ghf, r, h_out, sizes, h_codes, images, tables):
    for p, (img, tab) in enumerate(zip(images, tables)):
        at = p * r["slot_bytes"]
        assert sizes[p] == img.size, (p, sizes[p], img.size)
        assert np.array_equal(h_out[at : at + sizes[p]], img), p
        assert ghf.Code.from_buffer_copy(h_codes[p].tobytes()).as_dict() == tab, p


@pytest.mark.parametrize("n", COMPRESS_N)
@pytest.mark.parametrize("e", WIDTHS)
def test_build_codes_is_byte_exact_and_equals_compress_planes(env, e, n):
    ghf, ctx, torch = env
    x, images, tables = want_for(e, n)
    d_in = to_dev(torch, x)
    idx, idx2 = ctx.planes_index_alloc(n, e), ctx.planes_index_alloc(n, e)
    r = ctx.compress_planes_coded(d_in, e, n_elems=n, indexes=idx)
    slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
    # the filled side-cars decode at once: nothing between the two calls waits for the host
    back, nb = ctx.decode_planes(slots, [im.size for im in images], r["codes"], n, e, indexes=idx)
    ctx.sync()
    assert r["slot_bytes"] == ghf.planes_slot_bytes(n)
    h_out, sizes, h_codes = fetch(r)
    check_against_oracle(ghf, r, h_out, sizes, h_codes, images, tables)
    assert int(nb.item()) == n * e and np.array_equal(back[: n * e].cpu().numpy(), x)
    r2 = ctx.compress_planes(d_in, e, n_elems=n, indexes=idx2)
    ctx.sync()
    h_out2, sizes2, h_codes2 = fetch(r2)
    assert sizes2 == sizes and np.array_equal(h_codes2, h_codes)
    for p in range(e):
        at = p * r["slot_bytes"]
        assert np.array_equal(h_out2[at : at + sizes[p]], h_out[at : at + sizes[p]]), p
        for a, b in zip(ctx.index_to_host(idx[p]), ctx.index_to_host(idx2[p])):
            assert np.array_equal(a, b), p
    ctx.planes_index_free(idx)
    ctx.planes_index_free(idx2)


# ---------------------------------------------------------------- 3. codes trained on another tensor
def pack_body(code, data):
    """the body of `data` under an oracle code table: MSB first, the end mark, padded with 1-bits to a whole byte"""
    length, word = np.array(code.length, dtype=np.int64), np.array(code.codeword, dtype=np.int64)
    syms = np.concatenate([data.astype(np.int64), [256]])
    ln = length[syms]
    assert (ln > 0).all()
    start = np.cumsum(ln) - ln
    total = int(ln.sum())
    within = np.arange(total) - np.repeat(start, ln)
    bits = (np.repeat(word[syms], ln) >> (np.repeat(ln, ln) - 1 - within)) & 1
    bits = np.concatenate([bits, np.ones(-total % 8, dtype=np.int64)]).astype(np.uint8)
    return np.packbits(bits), total


@pytest.mark.parametrize("e", WIDTHS)
def test_codes_trained_on_one_tensor_compress_another(env, e):
    ghf, ctx, torch = env
    n = 65536 + 3
    a, b = normal_elems(n, e, seed=7), normal_elems(n, e, seed=11)
    assert not np.array_equal(a, b)
    d_a, d_b = to_dev(torch, a), to_dev(torch, b)
    codes_a = ctx.build_codes(ctx.histogram_planes(d_a, e, flags=ghf.HIST_COVER_ALL))
    idx = ctx.planes_index_alloc(n, e)
    r = ctx.compress_planes_coded(d_b, e, d_codes=codes_a, flags=0, indexes=idx)
    hists_b = ctx.histogram_planes(d_b, e)
    predicted = ctx.planes_image_bytes(hists_b, codes_a, e)
    own = ctx.planes_image_bytes(hists_b, ctx.build_codes(hists_b), e)
    ctx.sync()
    h_out, sizes, _ = fetch(r)
    assert [int(v) for v in predicted.cpu().numpy()] == sizes
    for p in range(e):
        a_p, b_p = np.ascontiguousarray(a[p::e]), np.ascontiguousarray(b[p::e])
        code_a = orc.build_code(covered(orc.histogram(a_p)))
        hist_b = orc.histogram(b_p)
        body, bits = pack_body(code_a, b_p)
        want = np.concatenate([orc.header_bytes(code_a), body])
        image = h_out[p * r["slot_bytes"] :][: sizes[p]]
        assert sizes[p] == want.size and np.array_equal(image, want), p
        assert np.array_equal(orc.decompress(image, cap=n + 8), b_p), p
        # Huffman is optimal for its own histogram: no other code makes fewer bits of B
        assert bits == orc.body_bits(hist_b, code_a) >= orc.body_bits(hist_b, orc.build_code(hist_b)), p
        assert int(own[p].item()) == orc.compress(b_p).size, p
    slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
    back, nb = ctx.decode_planes(slots, sizes, codes_a, n, e, indexes=idx)
    ctx.sync()
    assert int(nb.item()) == n * e and np.array_equal(back[: n * e].cpu().numpy(), b)
    ctx.planes_index_free(idx)


# ---------------------------------------------------------------- 4. refusals; the context stays usable after each
def good_call(ghf, ctx, torch):
    assert ctx.L.ghf_clear_status(ctx.h) == 0
    e, n = 2, 4097
    x, images, tables = want_for(e, n)
    r = ctx.compress_planes_coded(to_dev(torch, x), e)
    ctx.sync()
    check_against_oracle(ghf, r, *fetch(r), images, tables)


def refused(ghf, status, fn, *args, **kw):
    with pytest.raises(ghf.GhfError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, ei.value


def latched(ghf, ctx, status):
    with pytest.raises(ghf.GhfError) as ei:
        ctx.sync()
    assert ei.value.status == status, ei.value


def test_a_byte_without_a_code_and_a_code_that_is_not_complete_are_refused(env):
    ghf, ctx, torch = env
    e, n = 2, 4097
    a = normal_elems(n, e, seed=7)
    b = a.copy()
    b[2 * 100 + 1] = 0x7F  # bf16 with an exponent of 254: nothing standard-normal comes near it
    code_a_hi = orc.build_code(orc.histogram(np.ascontiguousarray(a[1::e])))
    assert code_a_hi.length[0x7F] == 0  # on the CPU: A's own code has nothing for that byte
    d_a, d_b = to_dev(torch, a), to_dev(torch, b)
    slot = ghf.planes_slot_bytes(n)

    def guarded():
        return torch.full((e * slot,), GUARD, dtype=torch.uint8, device="cuda")

    def untouched(d_out):
        torch.cuda.synchronize()
        return bool((d_out == GUARD).all().item())

    # codes trained on A without GHF_HIST_COVER_ALL: B's new high byte has no code
    codes_a = ctx.build_codes(ctx.histogram_planes(d_a, e))
    hists_b = ctx.histogram_planes(d_b, e)
    d_out = guarded()
    ctx.compress_planes_coded(d_b, e, d_codes=codes_a, flags=0, d_out=d_out)
    latched(ghf, ctx, E_NOCODE)
    assert untouched(d_out)
    sizes = ctx.planes_image_bytes(hists_b, codes_a, e)
    ctx.sync()
    sizes = sizes.cpu().numpy()
    assert sizes[1] == 0 and sizes[0] == orc.compress(np.ascontiguousarray(b[0::e])).size
    # the same context compresses B under its own codes
    x_images = [orc.compress(np.ascontiguousarray(b[p::e])) for p in range(e)]
    x_tables = [orc.build_code(orc.histogram(np.ascontiguousarray(b[p::e]))).as_dict() for p in range(e)]
    r = ctx.compress_planes_coded(d_b, e, flags=ghf.PLANES_BUILD_CODES)
    ctx.sync()
    check_against_oracle(ghf, r, *fetch(r), x_images, x_tables)
    # one length of plane 0's code made a bit longer: the Kraft sum falls short of 1
    codes_bad = ctx.build_codes(ctx.histogram_planes(d_a, e, flags=ghf.HIST_COVER_ALL))
    words = codes_bad.view(torch.int32)
    host = ghf.Code.from_buffer_copy(codes_bad[0].cpu().numpy().tobytes())
    sym = next(s for s in range(256) if host.length[s] < host.max_len)
    words[0, sym] += 1
    d_out = guarded()
    ctx.compress_planes_coded(d_b, e, d_codes=codes_bad, flags=0, d_out=d_out)
    latched(ghf, ctx, E_FORMAT)
    assert untouched(d_out)
    sizes = ctx.planes_image_bytes(hists_b, codes_bad, e)
    ctx.sync()
    sizes = sizes.cpu().numpy()
    assert sizes[0] == 0 and sizes[1] != 0
    good_call(ghf, ctx, torch)


def test_call_level_refusals_come_back_at_once_and_leave_the_context_usable(env):
    ghf, ctx, torch = env
    L = ctx.L
    e, n = 4, 4097
    x, _, _ = want_for(e, n)
    d_in = to_dev(torch, x)
    slot = ghf.planes_slot_bytes(n)
    codes = ctx.build_codes(ctx.histogram_planes(d_in, e, flags=ghf.HIST_COVER_ALL))
    ctx.sync()
    g_out = torch.full((16 * slot,), GUARD, dtype=torch.uint8, device="cuda")
    g_bytes = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    g_hists = torch.full((16 * ghf.NSYM,), GUARD_WORD, dtype=torch.int64, device="cuda")
    codes16 = codes.repeat(4, 1).contiguous()
    odd_in = torch.zeros(n * e + 16, dtype=torch.uint8, device="cuda")[1 : 1 + n * e]
    odd_codes = torch.zeros(codes.numel() + 16, dtype=torch.uint8, device="cuda")[4:]

    def coded(d_in_, n_, e_, d_codes_, flags, slot_):
        return L.ghf_compress_planes_coded(ctx.h, d_in_.data_ptr(), n_, e_, d_codes_.data_ptr() if d_codes_ is not None else None,
                                           flags, g_out.data_ptr(), slot_, g_bytes.data_ptr(), None)

    def hist(d_in_, n_, e_, flags):
        return L.ghf_histogram_planes(ctx.h, d_in_.data_ptr(), n_, e_, flags, g_hists.data_ptr())

    cases = [(lambda bad=bad: coded(d_in, n, bad, codes16, 0, slot), E_INVAL) for bad in (0, 1, 3, 16)]
    cases += [(lambda bad=bad: hist(d_in, n, bad, 0), E_INVAL) for bad in (0, 1, 3, 16)]
    cases += [(lambda bad=bad: L.ghf_planes_image_bytes(ctx.h, g_hists.data_ptr(), codes16.data_ptr(), bad, g_bytes.data_ptr()), E_INVAL)
              for bad in (0, 1, 3, 16)]
    cases += [
        (lambda: coded(odd_in, n, e, codes, 0, slot), E_INVAL),
        (lambda: coded(d_in, n, e, odd_codes, 0, slot), E_INVAL),
        (lambda: coded(d_in, n, e, None, ghf.PLANES_BUILD_CODES, slot), E_INVAL),
        (lambda: coded(d_in, n, e, codes, 2, slot), E_INVAL),
        (lambda: coded(d_in, n, e, codes, 0, slot + 8), E_INVAL),
        (lambda: coded(d_in, 0, e, codes, 0, slot), E_EMPTY),
        (lambda: coded(d_in, n, e, codes, 0, slot - 16), E_CAP),
        (lambda: hist(odd_in, n, e, 0), E_INVAL),
        (lambda: hist(d_in, n, e, 2), E_INVAL),
        (lambda: hist(d_in, (1 << 63), e, 0), E_INVAL),
        (lambda: hist(d_in, 0, e, 0), E_EMPTY),
    ]
    for k, (call, status) in enumerate(cases):
        assert call() == status, k
        torch.cuda.synchronize()
        assert bool((g_out == GUARD).all().item()) and bool((g_bytes == -1).all().item()), k
        assert bool((g_hists == GUARD_WORD).all().item()), k
        assert L.ghf_sync(ctx.h) == 0, k  # nothing latched either
        good_call(ghf, ctx, torch)


# ---------------------------------------------------------------- 5. the calls that were there before see nothing of it
def test_existing_calls_on_the_same_context_are_unaffected(env):
    ghf, ctx, torch = env
    e, n = 4, 4097
    x, images, tables = want_for(e, n)
    d_in = to_dev(torch, x)
    other, o_images, o_tables = want_for(e, n, seed=8)
    ctx.compress_planes_coded(to_dev(torch, other), e)  # same n_elems: the same workspace addresses, other bytes
    d_out, nbytes, _ = ctx.compress(d_in)
    r = ctx.compress_planes(d_in, e, n_elems=n)
    ctx.sync()
    flat = orc.compress(x)
    assert int(nbytes.item()) == flat.size and np.array_equal(d_out[: flat.size].cpu().numpy(), flat)
    check_against_oracle(ghf, r, *fetch(r), images, tables)
    # and the staged flat calls right behind a coded call plan the bytes that are there now
    codes = ctx.build_codes(ctx.histogram_planes(d_in, e, flags=ghf.HIST_COVER_ALL))
    ctx.compress_planes_coded(d_in, e, d_codes=codes, flags=0)
    r = ctx.compress_planes(to_dev(torch, other), e, n_elems=n)
    ctx.sync()
    check_against_oracle(ghf, r, *fetch(r), o_images, o_tables)
