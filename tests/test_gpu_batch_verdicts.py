"""GPU: the verdict of the batch host drivers on a call with TWO faults (DESIGN.md sections 9, 10, 12, 13, 15, 16, 24).

The refusal tests of the family (test_gpu_batch*.py) give one fault per call and look at the status.  Which of two faults a
driver reports -- the order of its checks -- and the text it leaves for ghf_last_error are part of what a caller sees, and
they are pinned here: every row of the table in build_cases names an entry point, breaks two of its arguments, and gives the
status AND the whole message of the fault the driver meets first ("" where it returns a bare GHF_E_INVAL or GHF_OK: the
last message stays as ghf_clear_status left it).  The expected values were read off the drivers' check order; a refused call
returns before anything is queued, so the whole table costs one good compress and decode per family and some host calls.

The orders that are easy to tidy away by accident have rows of their own (marked ORDER below): ghf_compress_batch and
ghf_decode_batch return GHF_OK for count == 0 before they look at null pointers, the shared and the planes calls refuse
null pointers first; the planes _seek wrappers report elem_bytes before a null pointer, the planes bodies decoders a null
pointer before elem_bytes.  Every _shared / _forms twin says its own name (marked PREFIX)."""
import ctypes as C

import numpy as np
import pytest

import pkgload

pytestmark = pytest.mark.gpu

OK, E_INVAL = 0, 1
E = 4
SIZES = [4097, 65, 1]  # one past a block, one past a segment, the smallest
PLANE_SIZES = [4100, 68, 4]  # the same in elements of E bytes
MAX_ITEM, PLANE_MAX = 4097, 4100
RAW_BAD = 1 << E  # names a plane at elem_bytes


class Good:
    """what the refused calls stand on: the items, one batch index wide enough for both families, one shared code and E plane
    codes from the batch histograms, and one good compress and decode per family"""

    def __init__(self, ghf, ctx, torch):
        rng = np.random.default_rng(24)
        self.datas = [rng.integers(0, 7, size=n, dtype=np.uint8) for n in SIZES]
        self.plane_datas = [rng.integers(0, 5, size=n, dtype=np.uint8) for n in PLANE_SIZES]
        self.items = [torch.from_numpy(d).cuda() for d in self.datas]
        self.plane_items = [torch.from_numpy(d).cuda() for d in self.plane_datas]
        self.bidx = ctx.batch_index_alloc(len(SIZES) * E, PLANE_MAX)  # 12 slots of up to 4100 symbols
        self.d_hist = ctx.histogram_batch(self.items, max_item_bytes=MAX_ITEM)
        self.d_code = ctx.build_code(self.d_hist)
        self.d_hists = ctx.histogram_batch_planes(self.plane_items, E, max_item_bytes=PLANE_MAX)
        self.d_codes = ctx.build_codes(self.d_hists)
        self.flat = ctx.compress_batch_shared(self.items, self.d_code, max_item_bytes=MAX_ITEM, index=self.bidx)
        self.flat_back = ctx.decode_batch_shared(self.flat["out_ptrs"], self.flat["out_bytes"], self.d_code, self.bidx, self.flat["in_bytes"])
        ctx.sync()
        self.planes = ctx.compress_batch_planes_shared(self.plane_items, self.d_codes, E, max_item_bytes=PLANE_MAX, index=self.bidx)
        self.planes_back = ctx.decode_batch_planes_shared(self.planes["out_ptrs"], self.planes["out_bytes"], self.d_codes, self.bidx,
                                                          self.planes["in_bytes"] // E, E)
        ctx.sync()
        for r, n in ((self.flat, 3), (self.flat_back, 3), (self.planes, 3 * E), (self.planes_back, 3)):
            assert r["status"].cpu().tolist() == [OK] * n
        for back, datas in ((self.flat_back, self.datas), (self.planes_back, self.plane_datas)):
            h = back["out"].cpu().numpy()
            for i, d in enumerate(datas):
                assert np.array_equal(h[i * back["out_stride"] :][: d.size], d), i

    def free(self, ctx):
        ctx.batch_index_free(self.bidx)


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    ghf = pkgload.load().ghf
    ctx = ghf.Context(0)
    good = Good(ghf, ctx, torch)
    yield ghf, ctx, torch, good
    good.free(ctx)
    ctx.close()


def build_cases(ghf, ctx, torch, g):
    """-> [(entry point, status, the whole message, thunk)]"""
    L, h = ctx.L, ctx.h
    f, p = g.flat, g.planes
    # the flat family's arrays: inputs, bodies (the decoders' streams), the decoders' outputs
    ip, ib = f["in_ptrs"].data_ptr(), f["in_bytes"].data_ptr()
    op, oc, ob, st = (f[k].data_ptr() for k in ("out_ptrs", "out_caps", "out_bytes", "status"))
    bp, bc, bb, bs = (g.flat_back[k].data_ptr() for k in ("out_ptrs", "out_caps", "out_bytes", "status"))
    code = g.d_code.data_ptr()
    g.own_codes = torch.zeros((3, C.sizeof(ghf.Code)), dtype=torch.uint8, device="cuda")  # ghf_compress_batch's, one per item
    own = g.own_codes.data_ptr()
    # the planes family's: 3 inputs, 3 E slots, 3 outputs
    pip, pib = p["in_ptrs"].data_ptr(), p["in_bytes"].data_ptr()
    pop, poc, pob, pst = (p[k].data_ptr() for k in ("out_ptrs", "out_caps", "out_bytes", "status"))
    pbp, pbc, pbb, pbs = (g.planes_back[k].data_ptr() for k in ("out_ptrs", "out_caps", "out_bytes", "status"))
    g.n_elems = p["in_bytes"] // E
    nel = g.n_elems.data_ptr()
    codes, hist, hists = g.d_codes.data_ptr(), g.d_hist.data_ptr(), g.d_hists.data_ptr()
    g.mask = torch.zeros(4, dtype=torch.int32, device="cuda")
    mask = g.mask.data_ptr()
    ix = g.bidx
    few = ghf.BatchIndex.from_buffer_copy(bytes(ix))  # covers two slots only
    few.count = 2
    bent = ghf.BatchIndex.from_buffer_copy(bytes(ix))  # strides the kernels do not assume: covers nothing, count 0 included
    bent.segs_per_item += 1
    R = lambda x: None if x is None else C.byref(x)

    def comp_own(ip=ip, mx=MAX_ITEM, n=3, ix=ix):
        return L.ghf_compress_batch(h, ip, ib, mx, n, op, oc, ob, own, R(ix), st)

    def dec_own(sp=op, cd=own, ix=ix, n=3):
        return L.ghf_decode_batch(h, sp, ob, cd, R(ix), ib, n, bp, bc, bb, bs)

    def images(n=3, d_o=bp, caps=bc, nb=bb):
        return L.ghf_decode_images_batch(h, op, ob, n, d_o, caps, nb, None, bs)

    def hist_flat(mx=MAX_ITEM, flags=0, d_h=hist):
        return L.ghf_histogram_batch(h, ip, ib, mx, 3, flags, d_h)

    def comp(ip=ip, mx=MAX_ITEM, n=3, cd=code, d_o=op, ix=ix):
        return L.ghf_compress_batch_shared(h, ip, ib, mx, n, cd, d_o, oc, ob, R(ix), st)

    def dec(sp=op, cd=code, ix=ix, n=3, d_o=bp):
        return L.ghf_decode_batch_shared(h, sp, ob, cd, R(ix), ib, n, d_o, bc, bb, bs)

    def bodies(cd=code, n=3, d_o=bp, caps=bc, nb=bb):
        return L.ghf_decode_bodies_batch_shared(h, op, ob, cd, n, d_o, caps, nb, bs)

    def hist_planes(mx=PLANE_MAX, e=E, flags=0, d_h=hists):
        return L.ghf_histogram_batch_planes(h, pip, pib, mx, 3, e, flags, d_h)

    def comp_planes(forms, ip=pip, mx=PLANE_MAX, n=3, e=E, cd=codes, raw=0, ix=ix):
        if forms:
            return L.ghf_compress_batch_planes_forms(h, ip, pib, mx, n, e, cd, raw, pop, poc, pob, R(ix), pst)
        assert raw == 0
        return L.ghf_compress_batch_planes_shared(h, ip, pib, mx, n, e, cd, pop, poc, pob, R(ix), pst)

    def raw_auto(d_h=hists, cd=codes, e=E):
        return L.ghf_batch_planes_raw_auto(h, d_h, cd, e, mask)

    def dec_planes(forms, sp=pop, cd=codes, ix=ix, n=3, e=E, raw=0):
        if forms:
            return L.ghf_decode_batch_planes_forms(h, sp, pob, cd, R(ix), nel, n, e, raw, pbp, pbc, pbb, pbs)
        assert raw == 0
        return L.ghf_decode_batch_planes_shared(h, sp, pob, cd, R(ix), nel, n, e, pbp, pbc, pbb, pbs)

    def bodies_planes(forms, sp=pop, cd=codes, n=3, e=E, raw=0, caps=pbc):
        if forms:
            return L.ghf_decode_bodies_batch_planes_forms(h, sp, pob, cd, n, e, raw, pbp, caps, pbb, pbs)
        assert raw == 0
        return L.ghf_decode_bodies_batch_planes_shared(h, sp, pob, cd, n, e, pbp, caps, pbb, pbs)

    # the refused seek calls never read a record: the bodies' own arrays stand in for the record arrays
    def seek_pack(ix=ix, nb=pib, n=3, e=E):
        return L.ghf_batch_seek_pack(h, R(ix), nb, n, e, pop, poc, pob, pst)

    def seek_flat(rp=op, cd=code, n=3):
        return L.ghf_decode_bodies_batch_shared_seek(h, op, ob, rp, ob, cd, n, bp, bc, bb, bs)

    def seek_planes(forms, rp=pop, cd=codes, n=3, e=E, raw=0, caps=pbc):
        if forms:
            return L.ghf_decode_bodies_batch_planes_forms_seek(h, pop, pob, rp, pob, cd, n, e, raw, pbp, caps, pbb, pbs)
        assert raw == 0
        return L.ghf_decode_bodies_batch_planes_shared_seek(h, pop, pob, rp, pob, cd, n, e, pbp, caps, pbb, pbs)

    def build_codes(n=E, flags=0):
        return L.ghf_build_codes(h, hists, n, codes, flags)

    MAX = "max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM"
    MAX_E = "max_item_bytes must be 1 .. GHF_BATCH_MAX_ITEM and a multiple of elem_bytes"
    COVER = "index does not cover (count, max_item_bytes) (use ghf_batch_index_alloc)"
    COVER_N = "index does not cover count items (use ghf_batch_index_alloc)"
    COVER_E = "index does not cover (count * elem_bytes, max_item_bytes / elem_bytes)"
    COVER_SLOTS = "index does not cover count * elem_bytes slots"
    CODE = "d_code is null or not 16-byte aligned"
    CODES = "d_codes is null or not 16-byte aligned"
    ELEM = "elem_bytes must be 2, 4 or 8"
    CAPS = "d_out_ptrs without d_out_caps"
    RAW = "raw_planes names a plane at or above elem_bytes"
    BARE = None  # a bare status: no message
    rows = [
        # -- 1. ghf_compress_batch: max_item_bytes, index, count == 0, null pointers
        ("ghf_compress_batch", E_INVAL, MAX, lambda: comp_own(mx=0, ix=few)),
        ("ghf_compress_batch", E_INVAL, COVER, lambda: comp_own(ix=bent, n=0)),  # ORDER: the count comes after
        ("ghf_compress_batch", OK, BARE, lambda: comp_own(n=0, ip=None)),  # ORDER: count == 0 before the null pointers
        ("ghf_compress_batch", E_INVAL, BARE, lambda: comp_own(n=2, ip=None)),
        # -- 2. ghf_decode_batch: null index, index, count == 0, null pointers
        ("ghf_decode_batch", OK, BARE, lambda: dec_own(n=0, cd=None)),  # ORDER
        ("ghf_decode_batch", E_INVAL, BARE, lambda: dec_own(ix=None, n=0)),
        ("ghf_decode_batch", E_INVAL, COVER_N, lambda: dec_own(ix=few, sp=None)),
        # -- 3. the shared calls: max_item_bytes, index, d_code, null pointers, count == 0
        ("ghf_compress_batch_shared", E_INVAL, BARE, lambda: comp(n=0, ip=None)),  # ORDER: the opposite of 1 and 2
        ("ghf_compress_batch_shared", E_INVAL, CODE, lambda: comp(cd=code + 8, d_o=None)),
        ("ghf_compress_batch_shared", E_INVAL, MAX, lambda: comp(mx=(1 << 20) + 1, ix=few)),
        ("ghf_compress_batch_shared", E_INVAL, COVER, lambda: comp(ix=few, cd=None)),
        ("ghf_decode_batch_shared", E_INVAL, BARE, lambda: dec(n=0, sp=None)),  # ORDER
        ("ghf_decode_batch_shared", E_INVAL, CODE, lambda: dec(cd=code + 8, d_o=None)),
        ("ghf_decode_batch_shared", E_INVAL, COVER_N, lambda: dec(ix=few, cd=None)),
        # -- 4. the histograms: (elem_bytes,) max_item_bytes, flags, null pointers, count == 0
        ("ghf_histogram_batch", E_INVAL, "unknown flags", lambda: hist_flat(flags=2, d_h=None)),
        ("ghf_histogram_batch", E_INVAL, MAX, lambda: hist_flat(mx=0, flags=2)),
        ("ghf_histogram_batch_planes", E_INVAL, ELEM, lambda: hist_planes(e=3, mx=6)),
        ("ghf_histogram_batch_planes", E_INVAL, MAX_E, lambda: hist_planes(e=4, mx=6, flags=2)),
        ("ghf_histogram_batch_planes", E_INVAL, "unknown flags", lambda: hist_planes(flags=2, d_h=None)),
        # -- 5. the decoders from nothing but bytes: null pointers, caps, (d_code,) count == 0
        ("ghf_decode_images_batch", E_INVAL, BARE, lambda: images(nb=None, caps=None)),
        ("ghf_decode_images_batch", E_INVAL, CAPS, lambda: images(caps=None, n=0)),
        ("ghf_decode_bodies_batch_shared", E_INVAL, BARE, lambda: bodies(nb=None, caps=None)),
        ("ghf_decode_bodies_batch_shared", E_INVAL, CAPS, lambda: bodies(caps=None, n=0)),
        ("ghf_decode_bodies_batch_shared", E_INVAL, CAPS, lambda: bodies(caps=None, cd=None)),
        ("ghf_decode_bodies_batch_shared", E_INVAL, CODE, lambda: bodies(cd=code + 8, n=0)),
    ]
    for forms in (False, True):  # PREFIX: each twin says its own name
        tail = "forms" if forms else "shared"
        # -- 6. the planes compress calls: elem_bytes, max_item_bytes, 32 bits, index, d_codes, raw_planes, null pointers, count == 0
        who = "ghf_compress_batch_planes_" + tail
        rows += [
            (who, E_INVAL, ELEM, lambda forms=forms: comp_planes(forms, e=3, mx=0)),
            (who, E_INVAL, "count * elem_bytes beyond 32 bits", lambda forms=forms: comp_planes(forms, n=0x40000000, e=8, mx=4104, ix=few)),
            (who, E_INVAL, COVER_E, lambda forms=forms: comp_planes(forms, ix=few, cd=None)),
            (who, E_INVAL, CODES, lambda forms=forms: comp_planes(forms, cd=codes + 8, raw=RAW_BAD) if forms else comp_planes(forms, cd=codes + 8, ip=None)),
            (who, E_INVAL, BARE, lambda forms=forms: comp_planes(forms, ip=None, n=0)),
        ]
        if forms:
            rows.append((who, E_INVAL, RAW, lambda: comp_planes(True, raw=RAW_BAD, ip=None)))
        # -- 7. the planes decoders with the live side-car: null index, elem_bytes, index, d_codes, raw_planes, null pointers, count == 0
        who = "ghf_decode_batch_planes_" + tail
        rows += [
            (who, E_INVAL, BARE, lambda forms=forms: dec_planes(forms, ix=None, e=3)),
            (who, E_INVAL, ELEM, lambda forms=forms: dec_planes(forms, e=3, ix=few)),
            (who, E_INVAL, COVER_SLOTS, lambda forms=forms: dec_planes(forms, ix=few, cd=None)),
        ]
        if forms:
            rows.append((who, E_INVAL, RAW, lambda: dec_planes(True, raw=RAW_BAD, sp=None)))
        # -- 8. the planes bodies decoders: null pointers, elem_bytes, caps, d_codes, raw_planes, count == 0
        who = "ghf_decode_bodies_batch_planes_" + tail
        rows += [
            (who, E_INVAL, BARE, lambda forms=forms: bodies_planes(forms, sp=None, e=3)),  # ORDER: null first
            (who, E_INVAL, ELEM, lambda forms=forms: bodies_planes(forms, e=3, caps=None)),
            (who, E_INVAL, CAPS, lambda forms=forms: bodies_planes(forms, caps=None, cd=None)),
        ]
        if forms:
            rows.append((who, E_INVAL, RAW, lambda: bodies_planes(True, raw=RAW_BAD, n=0)))
        # -- 9. the planes decoders of stored bodies: elem_bytes (the wrapper), null pointers, caps, the codes, raw_planes, count == 0
        who = "ghf_decode_bodies_batch_planes_" + tail + "_seek"
        rows += [
            (who, E_INVAL, ELEM, lambda forms=forms: seek_planes(forms, e=3, rp=None)),  # ORDER: the wrapper checks first
            (who, E_INVAL, CAPS, lambda forms=forms: seek_planes(forms, caps=None, cd=codes + 8)),
            (who, E_INVAL, "the code array is null or not 16-byte aligned", lambda forms=forms: seek_planes(forms, cd=None, n=0)),
        ]
        if forms:
            rows.append((who, E_INVAL, RAW, lambda: seek_planes(True, raw=RAW_BAD, n=0)))
    rows += [
        # -- 9. the flat decoder of stored bodies
        ("ghf_decode_bodies_batch_shared_seek", E_INVAL, BARE, lambda: seek_flat(rp=None, cd=None)),
        ("ghf_decode_bodies_batch_shared_seek", E_INVAL, "the code array is null or not 16-byte aligned", lambda: seek_flat(cd=code + 8, n=0)),
        # -- 10. ghf_batch_seek_pack: null index, elem_bytes, index, null pointers, count == 0
        ("ghf_batch_seek_pack", E_INVAL, "elem_bytes must be 1, 2, 4 or 8", lambda: seek_pack(e=3, ix=few)),
        ("ghf_batch_seek_pack", E_INVAL, COVER_SLOTS + " (use ghf_batch_index_alloc)", lambda: seek_pack(ix=few, nb=None)),
        ("ghf_batch_seek_pack", E_INVAL, BARE, lambda: seek_pack(ix=None, e=3)),
        # -- 11. ghf_batch_planes_raw_auto: elem_bytes, d_codes, null pointers
        ("ghf_batch_planes_raw_auto", E_INVAL, ELEM, lambda: raw_auto(e=3, cd=None)),
        ("ghf_batch_planes_raw_auto", E_INVAL, CODES, lambda: raw_auto(cd=codes + 8, d_h=None)),
        # -- 12. ghf_build_codes: one bare verdict for all of its arguments
        ("ghf_build_codes", E_INVAL, BARE, lambda: build_codes(n=9, flags=4)),
        ("ghf_build_codes", E_INVAL, BARE, lambda: build_codes(n=0, flags=4)),
    ]
    return [(who, status, "" if what is None else who + ": " + what, call) for who, status, what, call in rows]


def test_two_faults_give_the_status_and_the_message_of_the_first_and_leave_the_context_usable(env):
    ghf, ctx, torch, g = env
    L = ctx.L
    cases = build_cases(ghf, ctx, torch, g)
    assert len({who for who, _, _, _ in cases}) == 20  # every entry point of the family that takes a context and can leave a message
    wrong = []
    for i, (who, status, message, call) in enumerate(cases):
        assert L.ghf_clear_status(ctx.h) == OK  # forgets the last message
        rc = call()
        said = L.ghf_last_error(ctx.h).decode(errors="replace")
        print("row %2d %-44s -> %d %r" % (i, who, rc, said))
        if (rc, said) != (status, message):
            wrong.append((i, who, (rc, said), (status, message)))
    assert not wrong, "rows with another verdict: %r" % (wrong,)
    # nothing was queued and nothing latched
    assert L.ghf_clear_status(ctx.h) == OK
    ctx.sync()
    for r, n in ((g.flat, 3), (g.flat_back, 3), (g.planes, 3 * E), (g.planes_back, 3)):
        assert r["status"].cpu().tolist() == [OK] * n  # no refused call touched a status array
    # the context is still usable: the 65-byte item through the shared calls, with the arrays the table stood on
    one = lambda t: t[1:2].contiguous()
    f = g.flat
    ip, ib, op, oc = one(f["in_ptrs"]), one(f["in_bytes"]), one(f["out_ptrs"]), one(f["out_caps"])
    ob = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    back = torch.full((128,), 0xA5, dtype=torch.uint8, device="cuda")
    bp, bc = torch.tensor([back.data_ptr() + 16], dtype=torch.int64).cuda(), torch.tensor([65], dtype=torch.int64).cuda()
    bb, bs = torch.zeros_like(ob), torch.full_like(st, -1)
    rc = L.ghf_compress_batch_shared(ctx.h, ip.data_ptr(), ib.data_ptr(), 65, 1, g.d_code.data_ptr(), op.data_ptr(), oc.data_ptr(), ob.data_ptr(),
                                     C.byref(g.bidx), st.data_ptr())
    assert rc == OK, L.ghf_last_error(ctx.h).decode(errors="replace")
    rc = L.ghf_decode_batch_shared(ctx.h, op.data_ptr(), ob.data_ptr(), g.d_code.data_ptr(), C.byref(g.bidx), ib.data_ptr(), 1, bp.data_ptr(),
                                   bc.data_ptr(), bb.data_ptr(), bs.data_ptr())
    assert rc == OK, L.ghf_last_error(ctx.h).decode(errors="replace")
    ctx.sync()
    assert st.cpu().tolist() == [OK] == bs.cpu().tolist() and bb.cpu().tolist() == [65]
    h = back.cpu().numpy()
    assert np.array_equal(h[16 : 16 + 65], g.datas[1])
    assert np.all(h[:16] == 0xA5) and np.all(h[16 + 65 :] == 0xA5)
