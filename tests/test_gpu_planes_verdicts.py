"""GPU: the verdict of the byte-plane host drivers on a call with TWO faults (DESIGN.md sections 14, 17 - 21, 23).

The refusal tests of the family give one fault per call and look at the status.  Which of two faults a driver reports -- the
order of its checks -- and the text it leaves for ghf_last_error are part of what a caller sees, and they are pinned here:
every row of the table in build_cases names a driver's entry point, breaks two of its arguments, and gives the status AND the message of the
fault the driver meets first.  The expected values were read off the drivers' check order; a refused call returns before
anything is queued, so the whole table costs one good compress of each kind and a few hundred host calls.

Three orders are easy to tidy away by accident and have rows of their own (marked ORDER below): the sparse range reports a
short `cap` before it looks at sparse_planes / raw_planes, a rank info that ghf_sparse_rank_parse did not fill in
(GHF_E_FORMAT) before a stream's symbol count (GHF_E_INVAL), and GHF_OK for count == 0 only after every check.  The
messages carry the prefix of the entry point that was called, also where the forms range hands a tensor of dense planes on to
the dense range (marked PREFIX)."""
import ctypes as C

import numpy as np
import pytest

import pkgload

pytestmark = pytest.mark.gpu

OK, E_INVAL, E_EMPTY, E_CAP, E_FORMAT = 0, 1, 3, 5, 6
E, N = 4, 4097  # one element past a seek block
SPARSE = 0b0100  # plane 2 is stored as mask + values in the sparse compress
FIRST, COUNT = 5, 4090  # a range that crosses the seek block's edge


def tensor_bytes():
    """N elements of E bytes: planes 0, 1 and 3 are noise, plane 2 is zero but for every seventh element"""
    rng = np.random.default_rng(20)
    a = rng.integers(0, 256, size=(N, E), dtype=np.uint8)
    a[:, 2] = 0
    a[::7, 2] = rng.integers(1, 256, size=a[::7, 2].size, dtype=np.uint8)
    return a.reshape(-1)


class Good:
    """what the refused calls are built around: a dense and a sparse compress of one tensor, with side-cars, seek tables and
    the rank table of the sparse plane"""

    def __init__(self, ghf, ctx, torch):
        self.data = tensor_bytes()
        self.d_in = torch.from_numpy(self.data).cuda()
        self.d_base = torch.zeros_like(self.d_in)
        # dense: E streams of N symbols
        self.dense_idx = ctx.planes_index_alloc(N, E)
        self.dense = ctx.compress_planes_coded(self.d_in, E, indexes=self.dense_idx)
        # sparse: 2 E slots; slot 2 is plane 2's mask, slot E + 2 its values
        self.sparse = ctx.compress_planes_sparse_ranked(self.d_in, E, sparse_planes=SPARSE, indexes=True)
        ctx.sync()
        assert self.sparse["sparse_planes"] == SPARSE and 0 < self.sparse["n_vals"][2] < N
        self.n_vals = self.sparse["n_vals"]
        self.slot = self.dense["slot_bytes"]
        assert self.slot == self.sparse["slot_bytes"]
        self.dense_sizes = [int(v) for v in self.dense["out_bytes"].cpu().numpy()]
        self.sparse_sizes = [int(v) for v in self.sparse["out_bytes"].cpu().numpy()]
        rsb = self.sparse["rank_slot_bytes"]
        self.rank_host = np.ascontiguousarray(self.sparse["ranks"][2 * rsb : 2 * rsb + ghf.sparse_rank_bytes(N)].cpu().numpy())
        self.rank_info = ghf.sparse_rank_parse(self.rank_host)
        assert self.rank_info.n_vals == self.n_vals[2]
        # seek tables of every stored stream
        self.dense_tables = [ctx.seek_pack(self.dense_idx[p]) for p in range(E)]
        self.sparse_tables = [ctx.seek_pack(ix) if ix.n_symbols else None for ix in self.sparse["indexes"]]
        ctx.sync()
        self.dense_infos = [ghf.seek_parse(t.cpu().numpy()) for t in self.dense_tables]
        self.sparse_infos = [None if t is None else ghf.seek_parse(t.cpu().numpy()) for t in self.sparse_tables]

    def free(self, ctx):
        ctx.planes_index_free(self.dense_idx)
        ctx.planes_index_free(self.sparse["indexes"])


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


def copy_of(arr):
    out = type(arr)()
    C.memmove(out, arr, C.sizeof(arr))
    return out


def with_item(arr, j, **fields):
    """a copy of a ctypes array, item j changed: a plain value, or the named fields of a structure"""
    out = copy_of(arr)
    if "value" in fields:
        out[j] = fields["value"]
    else:
        for k, v in fields.items():
            setattr(out[j], k, v)
    return out


def build_cases(ghf, ctx, torch, g):
    """-> [(label, status, message without its prefix or the whole message, thunk)]"""
    L, h = ctx.L, ctx.h
    vp, sz = C.c_void_p, C.c_size_t
    AUTO = ghf.SPARSE_AUTO
    slot = g.slot
    inp, bas = g.d_in.data_ptr(), g.d_base.data_ptr()
    g.out = torch.zeros(2 * E * slot + 64, dtype=torch.uint8, device="cuda")
    g.nb = torch.zeros(16, dtype=torch.int64, device="cuda")
    g.codes = torch.zeros((2 * E, C.sizeof(ghf.Code)), dtype=torch.uint8, device="cuda")
    g.rank_out = torch.zeros(E * g.sparse["rank_slot_bytes"] + 64, dtype=torch.uint8, device="cuda")
    g.back = torch.zeros(N * E + 64, dtype=torch.uint8, device="cuda")
    out, nb, codes, ranks_out, back = (t.data_ptr() for t in (g.out, g.nb, g.codes, g.rank_out, g.back))
    rank_slot = g.sparse["rank_slot_bytes"]
    chosen_raw, chosen, out_vals = C.c_uint(0), C.c_uint(0), (sz * E)()

    # ---- the compress drivers
    def coded(d_in=inp, n=N, e=E, d_c=codes, flags=ghf.PLANES_BUILD_CODES, d_o=out, slot_=slot, ix=None):
        return L.ghf_compress_planes_coded(h, d_in, n, e, d_c, flags, d_o, slot_, nb, ix)

    def coded_delta(d_in=inp, d_b=bas, n=N, e=E, d_c=codes, flags=ghf.PLANES_BUILD_CODES, d_o=out, slot_=slot, ix=None):
        return L.ghf_compress_planes_delta(h, d_in, d_b, n, e, d_c, flags, d_o, slot_, nb, ix)

    def sparse(d_in=inp, n=N, e=E, m=SPARSE, d_o=out, slot_=slot):
        return L.ghf_compress_planes_sparse(h, d_in, n, e, m, d_o, slot_, nb, codes, None, C.byref(chosen), out_vals)

    def ranked(n=N, e=E, m=SPARSE, slot_=slot, d_r=ranks_out, rslot=rank_slot):
        return L.ghf_compress_planes_sparse_ranked(h, inp, n, e, m, out, slot_, nb, codes, None, C.byref(chosen), out_vals, d_r, rslot)

    def forms(d_b=None, n=N, e=E, raw=0, m=0, slot_=slot, d_r=None, rslot=rank_slot):
        return L.ghf_compress_planes_forms(h, inp, d_b, n, e, raw, m, out, slot_, nb, codes, None, d_r, rslot, C.byref(chosen_raw),
                                           C.byref(chosen), out_vals)

    # ---- the whole-tensor decoders
    d_ptrs = (vp * E)(*[g.dense["out"][p * slot :].data_ptr() for p in range(E)])
    d_sizes = (sz * E)(*g.dense_sizes)
    d_codes = g.dense["codes"].data_ptr()
    s_ptrs = (vp * (2 * E))(*[g.sparse["out"][j * slot :].data_ptr() for j in range(2 * E)])
    s_sizes = (sz * (2 * E))(*g.sparse_sizes)
    s_codes = g.sparse["codes"].data_ptr()
    s_idx = g.sparse["indexes"]
    s_vals = (sz * E)(*g.n_vals)

    def dec(p=d_ptrs, ix=g.dense_idx, n=N, e=E, d_o=back, cap=N * E):
        return L.ghf_decode_planes(h, p, d_sizes, d_codes, ix, n, e, d_o, cap, nb)

    def dec_delta(ix=g.dense_idx, d_b=bas, n=N, e=E, d_o=back, cap=N * E):
        return L.ghf_decode_planes_delta(h, d_ptrs, d_sizes, d_codes, ix, d_b, n, e, d_o, cap, nb)

    def dec_sparse(p=s_ptrs, ix=s_idx, m=SPARSE, nv=s_vals, n=N, e=E, d_o=back, cap=N * E):
        return L.ghf_decode_planes_sparse(h, p, s_sizes, s_codes, ix, m, nv, n, e, d_o, cap, nb)

    def dec_forms(p=s_ptrs, s=s_sizes, ix=s_idx, raw=0, m=SPARSE, nv=s_vals, n=N, e=E, d_o=back, cap=N * E):
        return L.ghf_decode_planes_forms(h, p, s, s_codes, ix, None, raw, m, nv, n, e, d_o, cap, nb)

    # ---- the range decoders
    d_infos = (ghf.SeekInfo * E)(*g.dense_infos)
    d_tabs = (vp * E)(*[t.data_ptr() for t in g.dense_tables])
    d_tbytes = (sz * E)(*[ghf.seek_bytes(N)] * E)
    s_infos = (ghf.SeekInfo * (2 * E))(*[ghf.SeekInfo() if i is None else i for i in g.sparse_infos])
    s_tabs = (vp * (2 * E))(*[None if t is None else t.data_ptr() for t in g.sparse_tables])
    s_tbytes = (sz * (2 * E))(*[0 if i is None else ghf.seek_bytes(i.n_symbols) for i in g.sparse_infos])
    r_infos = (ghf.SparseRankInfo * E)()
    r_infos[2] = g.rank_info
    r_ptrs = (vp * E)()
    r_ptrs[2] = g.rank_host.ctypes.data

    def rng(ix=g.dense_idx, infos=None, tabs=None, tbytes=None, e=E, first=FIRST, count=COUNT, d_o=back, cap=COUNT * E):
        return L.ghf_decode_planes_range(h, d_ptrs, d_sizes, d_codes, ix, infos, tabs, tbytes, e, first, count, d_o, cap)

    def rng_delta(ix=None, infos=d_infos, tabs=d_tabs, tbytes=d_tbytes, d_b=bas, first=FIRST, count=COUNT, cap=COUNT * E):
        return L.ghf_decode_planes_range_delta(h, d_ptrs, d_sizes, d_codes, ix, infos, tabs, tbytes, d_b, E, first, count, back, cap)

    def rng_sparse(p=s_ptrs, ix=s_idx, infos=None, tabs=None, tbytes=None, ri=r_infos, rp=r_ptrs, m=SPARSE, n=N, first=FIRST, count=COUNT,
                   d_o=back, cap=COUNT * E):
        return L.ghf_decode_planes_sparse_range(h, p, s_sizes, s_codes, ix, infos, tabs, tbytes, ri, rp, m, n, E, first, count, d_o, cap)

    def rng_forms(ix=s_idx, infos=None, tabs=None, tbytes=None, ri=r_infos, rp=r_ptrs, raw=0, m=SPARSE, n=N, first=FIRST, count=COUNT,
                  cap=COUNT * E):
        return L.ghf_decode_planes_forms_range(h, s_ptrs, s_sizes, s_codes, ix, infos, tabs, tbytes, ri, rp, None, raw, m, n, E, first,
                                               count, back, cap)

    # the dense tensor in the arrays of 2 E slots that the forms calls take
    f_ptrs = (vp * (2 * E))(*list(d_ptrs))
    f_sizes = (sz * (2 * E))(*g.dense_sizes)
    f_idx = (ghf.Index * (2 * E))()
    C.memmove(f_idx, g.dense_idx, C.sizeof(g.dense_idx))
    g.forms_dense = (f_ptrs, f_sizes, f_idx)

    def rng_forms_dense(first=FIRST, count=COUNT, cap=COUNT * E):
        return L.ghf_decode_planes_forms_range(h, f_ptrs, f_sizes, d_codes, f_idx, None, None, None, None, None, None, 0, 0, N, E, first,
                                               count, back, cap)

    ALIGN = "d_in, d_base, d_out, d_codes and slot_bytes must be multiples of 16"
    SLOT = "slot_bytes below ghf_planes_slot_bytes(n_elems)"
    SPARSE_IN = "sparse_planes is GHF_SPARSE_AUTO alone or has bits below elem_bytes only"
    SPARSE_BACK = "sparse_planes has bits below elem_bytes only (the mask the compress call reported)"
    RAW_BACK = "raw_planes has bits below elem_bytes only, none of them a sparse plane's"
    ONE_OF = "exactly one of indexes / (h_infos, h_table_ptrs, h_table_bytes) must be given"
    SEEK = "the seek table does not have the size its header implies"
    rows = [
        # -- compress_planes_coded: elem_bytes, alignment, flags, overflow, indexes, empty, slot
        ("ghf_compress_planes_coded", E_INVAL, "elem_bytes must be 2, 4 or 8", lambda: coded(e=3, d_in=inp + 8)),
        ("ghf_compress_planes_coded", E_INVAL, "unknown flags", lambda: coded(flags=1 << 7, slot_=slot - 16)),
        ("ghf_compress_planes_coded", E_INVAL, "an index does not match n_elems (use ghf_index_alloc)", lambda: coded(n=0, ix=g.dense_idx)),
        ("ghf_compress_planes_coded", E_EMPTY, "no elements", lambda: coded(n=0, slot_=0)),
        ("ghf_compress_planes_delta", E_INVAL, ALIGN, lambda: coded_delta(d_b=bas + 8, n=0)),
        ("ghf_compress_planes_delta", E_INVAL, "unknown flags", lambda: coded_delta(flags=2, ix=with_item(g.dense_idx, 1, n_symbols=N + 1))),
        # -- compress_planes_sparse: ..., alignment, ranks, sparse_planes, overflow, empty, slot, rank slot
        ("ghf_compress_planes_sparse", E_INVAL, ALIGN, lambda: sparse(d_o=out + 8, m=1 << E)),
        ("ghf_compress_planes_sparse", E_INVAL, SPARSE_IN, lambda: sparse(m=AUTO | 1, n=0)),
        ("ghf_compress_planes_sparse_ranked", E_INVAL, "d_ranks and rank_slot_bytes must be multiples of 16", lambda: ranked(rslot=8, slot_=slot - 16)),
        ("ghf_compress_planes_sparse_ranked", E_CAP, SLOT, lambda: ranked(slot_=slot - 16, rslot=16)),
        ("ghf_compress_planes_sparse_ranked", E_EMPTY, "no elements", lambda: ranked(n=0, rslot=16)),
        # -- ghf_compress_planes_forms: ..., alignment, ranks, sparse_planes, raw_planes, overflow, empty, slot, rank slot
        ("ghf_compress_planes_forms", E_INVAL, SPARSE_IN, lambda: forms(m=1 << E, raw=1 << E)),
        ("ghf_compress_planes_forms", E_INVAL, "raw_planes is GHF_RAW_AUTO alone or has bits below elem_bytes only, none of them a sparse plane's",
         lambda: forms(raw=SPARSE, m=SPARSE, slot_=slot - 16)),
        ("ghf_compress_planes_forms", E_CAP, SLOT, lambda: forms(m=SPARSE, slot_=slot - 16, d_r=ranks_out, rslot=16)),
        ("ghf_compress_planes_forms", E_INVAL, ALIGN, lambda: forms(d_b=bas + 8, raw=1 << E)),
        # -- decode_planes: elem_bytes, stream pointers, d_out / d_base, overflow, indexes, empty, cap
        ("ghf_decode_planes", E_INVAL, "a stream pointer is null or not 16-byte aligned", lambda: dec(p=with_item(d_ptrs, 1, value=d_ptrs[1] + 8), d_o=back + 8)),
        ("ghf_decode_planes", E_INVAL, "an index does not cover exactly n_elems symbols", lambda: dec(ix=with_item(g.dense_idx, 3, n_symbols=N + 1), cap=N * E - 1)),
        ("ghf_decode_planes", E_INVAL, "an index does not cover exactly n_elems symbols", lambda: dec(n=0)),
        ("ghf_decode_planes_delta", E_INVAL, "d_out and d_base must be 16-byte aligned", lambda: dec_delta(d_b=bas + 8, n=0, ix=None)),
        ("ghf_decode_planes_delta", E_EMPTY, "no elements", lambda: dec_delta(n=0, ix=None, cap=0)),
        # -- decode_planes_sparse: elem_bytes, sparse_planes, raw_planes, value counts, stream pointers, d_out / d_base, overflow,
        #    indexes, raw sizes, empty, cap
        ("ghf_decode_planes_sparse", E_INVAL, SPARSE_BACK, lambda: dec_sparse(m=AUTO, p=with_item(s_ptrs, 1, value=None))),
        ("ghf_decode_planes_sparse", E_INVAL, "a plane has more values than elements", lambda: dec_sparse(nv=with_item(s_vals, 2, value=N + 1), p=with_item(s_ptrs, 1, value=None))),
        ("ghf_decode_planes_sparse", E_INVAL, "an index does not cover exactly the symbols of its stream",
         lambda: dec_sparse(ix=with_item(s_idx, E + 2, n_symbols=g.n_vals[2] + 1), cap=N * E - 1)),
        ("ghf_decode_planes_forms", E_INVAL, RAW_BACK, lambda: dec_forms(raw=SPARSE, d_o=back + 8)),
        ("ghf_decode_planes_forms", E_INVAL, "a raw plane does not have n_elems bytes", lambda: dec_forms(raw=0b0001, s=with_item(s_sizes, 0, value=N + 1), cap=N * E - 1)),
        ("ghf_decode_planes_forms", E_INVAL, "a stream pointer is null or not 16-byte aligned", lambda: dec_forms(p=with_item(s_ptrs, E + 2, value=None), cap=N * E - 1)),
        # -- decode_planes_range: elem_bytes, one of indexes / tables, pointers, d_out / d_base, indexes, first + count, overflow,
        #    seek tables, cap, count == 0
        ("ghf_decode_planes_range", E_INVAL, "elem_bytes must be 2, 4 or 8", lambda: rng(e=3, infos=d_infos, tabs=d_tabs, tbytes=d_tbytes)),
        ("ghf_decode_planes_range", E_INVAL, ONE_OF, lambda: rng(infos=d_infos, tabs=d_tabs, tbytes=d_tbytes, d_o=back + 8)),
        ("ghf_decode_planes_range", E_INVAL, "the planes disagree on n_symbols", lambda: rng(ix=with_item(g.dense_idx, 1, n_symbols=N + 1), cap=COUNT * E - 1)),
        ("ghf_decode_planes_range", E_INVAL, "first + count exceeds n_elems", lambda: rng(first=N, count=1, cap=0)),
        ("ghf_decode_planes_range_delta", E_FORMAT, SEEK, lambda: rng_delta(tbytes=with_item(d_tbytes, 1, value=d_tbytes[1] + 16), cap=COUNT * E - 1)),
        ("ghf_decode_planes_range_delta", E_INVAL, "a table pointer is null or not 16-byte aligned", lambda: rng_delta(tabs=with_item(d_tabs, 3, value=None), first=N, count=1)),
        # -- decode_planes_sparse_range: what the dense range asks, then sparse_planes, raw_planes, raw sizes, the rank tables, the
        #    streams' symbol counts with the values slots, count == 0
        ("ghf_decode_planes_sparse_range", E_CAP, "output capacity below count * elem_bytes", lambda: rng_sparse(cap=COUNT * E - 1, m=AUTO)),  # ORDER
        ("ghf_decode_planes_sparse_range", E_FORMAT, "a rank info is not what ghf_sparse_rank_parse fills in",  # ORDER
         lambda: rng_sparse(ri=with_item(r_infos, 2, version=0), ix=with_item(s_idx, 0, n_symbols=N + 1))),
        ("ghf_decode_planes_sparse_range", E_INVAL, "a values stream does not have the symbols its rank table counts",  # ORDER: count == 0
         lambda: rng_sparse(count=0, ri=with_item(r_infos, 2, n_vals=g.n_vals[2] - 1))),
        ("ghf_decode_planes_sparse_range", E_INVAL, "a stream or table pointer is null or not 16-byte aligned", lambda: rng_sparse(p=with_item(s_ptrs, 1, value=None), d_o=back + 8)),
        ("ghf_decode_planes_sparse_range", E_INVAL, "sparse planes need their rank tables", lambda: rng_sparse(ri=None, rp=None, ix=with_item(s_idx, 0, n_symbols=N + 1))),
        ("ghf_decode_planes_sparse_range", E_INVAL, "a rank table is not one of n_elems elements", lambda: rng_sparse(n=N - 1, first=0, count=16, ri=with_item(r_infos, 2, version=0))),
        ("ghf_decode_planes_forms_range", E_CAP, "output capacity below count * elem_bytes", lambda: rng_forms(cap=COUNT * E - 1, raw=1 << E)),  # ORDER
        ("ghf_decode_planes_forms_range", E_INVAL, RAW_BACK, lambda: rng_forms(raw=1 << E, ri=None, rp=None)),
        ("ghf_decode_planes_forms_range", E_FORMAT, SEEK,
         lambda: rng_forms(ix=None, infos=s_infos, tabs=s_tabs, tbytes=with_item(s_tbytes, 0, value=s_tbytes[0] + 16), cap=COUNT * E - 1)),
        ("ghf_decode_planes_forms_range", E_INVAL, "a mask stream does not have ghf_sparse_mask_bytes(n_elems) symbols",
         lambda: rng_forms(count=0, ix=with_item(s_idx, 2, n_symbols=s_idx[2].n_symbols + 1))),
        # a tensor of dense planes only, which the forms range hands on to the dense range: the messages both ranges share keep
        # the prefix of the call that was made (PREFIX)
        ("ghf_decode_planes_forms_range", E_INVAL, "first + count exceeds n_elems", lambda: rng_forms_dense(first=N, count=1, cap=0)),
        ("ghf_decode_planes_forms_range", E_CAP, "output capacity below count * elem_bytes", lambda: rng_forms_dense(cap=COUNT * E - 1)),
    ]
    return [(who, status, who + ": " + what, call) for who, status, what, call in rows]


def test_two_faults_give_the_status_and_the_message_of_the_first_and_leave_the_context_usable(env):
    ghf, ctx, torch, g = env
    L = ctx.L
    cases = build_cases(ghf, ctx, torch, g)
    assert len({who for who, _, _, _ in cases}) == 13  # every driver, through each of its doors
    wrong = []
    for i, (who, status, message, call) in enumerate(cases):
        assert L.ghf_clear_status(ctx.h) == OK  # forgets the last message
        rc = call()
        said = L.ghf_last_error(ctx.h).decode(errors="replace")
        print("row %2d %-36s -> %d %r" % (i, who, rc, said))
        if (rc, said) != (status, message):
            wrong.append((i, who, (rc, said), (status, message)))
    assert not wrong, "rows with another verdict: %r" % (wrong,)
    # nothing was queued and nothing latched
    assert L.ghf_clear_status(ctx.h) == OK
    ctx.sync()
    # the context is still usable: a dense tensor through the forms range, which hands it on to the dense range
    f_ptrs, f_sizes, f_idx = g.forms_dense
    g.back.fill_(0xA5)
    rc = L.ghf_decode_planes_forms_range(ctx.h, f_ptrs, f_sizes, g.dense["codes"].data_ptr(), f_idx, None, None, None, None, None, None, 0, 0,
                                         N, E, FIRST, COUNT, g.back.data_ptr(), COUNT * E)
    assert rc == OK, L.ghf_last_error(ctx.h).decode(errors="replace")
    ctx.sync()
    assert np.array_equal(g.back[: COUNT * E].cpu().numpy(), g.data[FIRST * E : (FIRST + COUNT) * E])
    assert bool((g.back[COUNT * E :] == 0xA5).all().item())
