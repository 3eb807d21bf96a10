"""GPU: every batch byte-plane kernel against its twin -- the `_shared` entry and the `_forms` entry with raw_planes == 0
give the same verdict for every item, in the same order of precedence, and the same bytes ("what the
`_shared` call of the same name gives in every output array").

The four pairs are ghf_compress_batch_planes_shared / _forms, ghf_decode_batch_planes_shared / _forms ("live"),
ghf_decode_bodies_batch_planes_shared / _forms ("bodies") and ghf_decode_bodies_batch_planes_shared_seek / _forms_seek
("seek"), each for E in {2, 4, 8}; the last two also with d_out_ptrs null (sizes only).  One batch per E holds items that
succeed -- 1 element, 17 elements, one element more than a round of the live and the bodies decoder, one element more than
a round of the run-record decoder: the smallest shapes at which the plane loop and a round's closing barrier both run --
and one item for each way to fail: a null stream pointer, a misaligned one, a cap one byte short, a truncated stream,
planes whose counts disagree, a damaged record header.  A second call hands every decoder a broken codes[1]: GHF_E_FORMAT
on every item.  The helpers are those of tests/test_gpu_batch_forms.py."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import test_gpu_batch_forms as tf
from test_gpu_batch_forms import E_CAP, E_CORRUPT, E_EMPTY, E_FORMAT, E_INVAL, GUARD, OK, env  # noqa: F401  (env: the fixture)

pytestmark = pytest.mark.gpu

ES = [2, 4, 8]
# csrc/ghf_batch_core.h: the symbols of one plane that one round of each decoder stages
K_BATCH_DEC_ROUND_BYTES, K_IMG_STAGE_BYTES, K_BATCH_SEEK_ROUND_BYTES = 16 * 1024, 16 * 1024, 32 * 1024
GOOD_ELEMS = [1, 17, K_BATCH_DEC_ROUND_BYTES + 1, K_BATCH_SEEK_ROUND_BYTES + 1]
assert K_IMG_STAGE_BYTES + 1 in GOOD_ELEMS
VICTIM_ELEMS = 300
NULL_PTR, MISALIGNED, CAP_SHORT, TRUNCATED, DISAGREE, BAD_HEADER = range(len(GOOD_ELEMS), len(GOOD_ELEMS) + 6)
COUNT = BAD_HEADER + 1
DECODERS = [("live", True), ("bodies", True), ("bodies", False), ("seek", True), ("seek", False)]


class World:
    """the batch of one width, packed by ghf_compress_batch_planes_shared, with its run records"""

    def __init__(self, env, e):
        ghf, ctx, torch = env
        self.env, self.e, self.count, self.max_item = env, e, COUNT, GOOD_ELEMS[-1] * e
        elems = GOOD_ELEMS + [VICTIM_ELEMS] * (COUNT - len(GOOD_ELEMS))
        self.datas = [dg.make(["zipf", "text", "sym16", "uniform"][k % 4], n * e, seed=2500 + 16 * e + k) for k, n in enumerate(elems)]
        self.inp = tf.Inputs(torch, self.datas)
        d_hists = ctx.histogram_batch_planes([torch.from_numpy(d).cuda() for d in self.datas], e, flags=tf.COVER_ALL)
        self.d_codes = ctx.build_codes(d_hists)
        ctx.sync()
        self.h_codes = [ghf.Code.from_buffer_copy(row.tobytes()) for row in self.d_codes.cpu().numpy()]
        self.packed = tf.Packed(env, self.inp, self.d_codes, e, self.max_item).run()
        assert np.all(self.packed.h_status == OK)
        self.rec = ctx.batch_seek_pack(self.packed.bidx, self.inp.in_bytes, elem_bytes=e)
        ctx.sync()
        assert not self.rec["status"].any().item()


_worlds = {}


def world(env, e):
    if e not in _worlds:
        _worlds[e] = World(env, e)
    return _worlds[e]


@pytest.fixture(scope="module", autouse=True)
def _free_worlds():
    yield
    for w in _worlds.values():
        w.packed.free()
    _worlds.clear()


class Args:
    """what the decoders of world `w` are handed: the packed batch with one item damaged for each failing verdict"""

    def __init__(self, w):
        torch, e, b = w.env[2], w.e, w.packed
        self.ptrs = [int(x) for x in b.out_ptrs.cpu().tolist()]
        self.sizes = [int(x) for x in b.h_bytes]
        self.caps = [int(s) for s in w.inp.sizes]
        self.rec = w.rec["rec"].clone()  # the records, so that one header can be damaged
        move = self.rec.data_ptr() - w.rec["rec"].data_ptr()
        self.rec_ptrs = [int(x) + move for x in w.rec["rec_ptrs"].cpu().tolist()]
        self.rec_bytes = [int(x) for x in w.rec["rec_bytes"].cpu().tolist()]
        self.ptrs[NULL_PTR * e + 1] = 0
        self.ptrs[MISALIGNED * e + e - 1] += 8
        self.caps[CAP_SHORT] -= 1
        self.sizes[TRUNCATED * e] //= 2
        src = 1 * e + 1  # plane 1 of the item of 17 elements in the place of plane 1 of one of 300
        for a in (self.ptrs, self.sizes, self.rec_ptrs, self.rec_bytes):
            a[DISAGREE * e + 1] = a[src]
        self.rec[self.rec_ptrs[BAD_HEADER * e] - self.rec.data_ptr()] ^= 0xFF  # the first byte of the magic of plane 0
        w.env[1].sync()


def verdicts(kind, write):
    want = [OK] * COUNT
    want[NULL_PTR] = want[MISALIGNED] = E_INVAL
    if write:
        want[CAP_SHORT] = E_CAP
    if kind != "seek" or write:  # the sizes-only pass of the run-record decoder does not read the streams
        want[TRUNCATED] = E_CORRUPT
    want[DISAGREE] = E_CORRUPT
    if kind == "seek":
        want[BAD_HEADER] = E_FORMAT
    return want


def decode(w, kind, forms, write, a, d_codes):
    """one call of the `_shared` entry (forms False) or of the `_forms` entry with raw_planes == 0; every output sits at an
    unaligned address between guard bytes.  -> (item_status, out_bytes, the whole output buffer, the items' offsets in it)"""
    ghf, ctx, torch = w.env
    e, L, count = w.e, ghf.lib(), w.count
    stride = (w.max_item + 15 & ~15) + 64
    d_out = torch.full((count * stride + 64,), GUARD, dtype=torch.uint8).cuda()
    offs = [i * stride + 17 + (i % 15) for i in range(count)]
    out_ptrs, out_caps = tf.i64(torch, [d_out.data_ptr() + o for o in offs]), tf.i64(torch, a.caps)
    out_bytes = torch.full((count,), -1, dtype=torch.int64).cuda()
    status = torch.full((count,), -1, dtype=torch.int32).cuda()
    sp, sb = tf.i64(torch, a.ptrs), tf.i64(torch, a.sizes)
    raw = (0,) if forms else ()
    tail = (out_ptrs.data_ptr() if write else None, out_caps.data_ptr(), out_bytes.data_ptr(), status.data_ptr())
    if kind == "live":
        f = L.ghf_decode_batch_planes_forms if forms else L.ghf_decode_batch_planes_shared
        n_elems = tf.i64(torch, [s // e for s in w.inp.sizes])
        rc = f(ctx.h, sp.data_ptr(), sb.data_ptr(), d_codes.data_ptr(), C.byref(w.packed.bidx), n_elems.data_ptr(), count, e, *raw, *tail)
    elif kind == "bodies":
        f = L.ghf_decode_bodies_batch_planes_forms if forms else L.ghf_decode_bodies_batch_planes_shared
        rc = f(ctx.h, sp.data_ptr(), sb.data_ptr(), d_codes.data_ptr(), count, e, *raw, *tail)
    else:
        f = L.ghf_decode_bodies_batch_planes_forms_seek if forms else L.ghf_decode_bodies_batch_planes_shared_seek
        rp, rb = tf.i64(torch, a.rec_ptrs), tf.i64(torch, a.rec_bytes)
        rc = f(ctx.h, sp.data_ptr(), sb.data_ptr(), rp.data_ptr(), rb.data_ptr(), d_codes.data_ptr(), count, e, *raw, *tail)
    assert rc == 0, rc
    ctx.sync()  # raises if the context's status word was latched: per-item failures must not do that
    return status.cpu().numpy(), out_bytes.cpu().numpy(), d_out.cpu().numpy(), offs


def bad_code_1(w):
    """the world's codes with codes[1] replaced by one whose Kraft sum is above 1"""
    bad = tf.bad_codes(w.h_codes[1], w.env[0].Code.from_buffer_copy)[1][1]
    return tf.codes_to_device(w.env[2], [bad if q == 1 else c for q, c in enumerate(w.h_codes)])


@pytest.mark.parametrize("kind,write", DECODERS)
@pytest.mark.parametrize("e", ES)
def test_decoder_and_its_twin_give_every_item_the_same_verdict_and_bytes(env, e, kind, write):
    w = world(env, e)
    a = Args(w)
    ps, pb, pout, offs = decode(w, kind, False, write, a, w.d_codes)
    ts, tb, tout, _ = decode(w, kind, True, write, a, w.d_codes)
    print("parent", ps.tolist(), pb.tolist(), "\ntwin  ", ts.tolist(), tb.tolist())
    assert ps.tolist() == verdicts(kind, write)
    assert ts.tolist() == ps.tolist() and tb.tolist() == pb.tolist()
    for i, d in enumerate(w.datas):
        assert int(pb[i]) == (d.size if ps[i] == OK else 0), i
        if ps[i] == OK and write:
            assert np.array_equal(pout[offs[i] : offs[i] + d.size], d), i
            assert np.array_equal(tout[offs[i] : offs[i] + d.size], d), i
    if not write:
        assert np.all(pout == GUARD) and np.all(tout == GUARD)


@pytest.mark.parametrize("kind,write", DECODERS)
@pytest.mark.parametrize("e", ES)
def test_a_broken_code_1_is_format_on_every_item_of_decoder_and_twin(env, e, kind, write):
    w = world(env, e)
    a, d_bad = Args(w), bad_code_1(w)
    for forms in (False, True):
        status, out_bytes, out, _ = decode(w, kind, forms, write, a, d_bad)
        assert status.tolist() == [E_FORMAT] * COUNT and not out_bytes.any(), forms  # in front of every verdict of an item
        assert np.all(out == GUARD), forms


@pytest.mark.parametrize("e", ES)
def test_packer_and_its_twin_give_every_slot_the_same_verdict_bytes_and_index(env, e):
    ghf, ctx, torch = env
    w = world(env, e)
    good = [w.datas[0], w.datas[1], dg.make("zipf", 4097 * e, seed=77 + e)]  # the last: one element more than a round of the packer
    victim = w.datas[NULL_PTR]
    datas = good + [np.zeros(0, dtype=np.uint8), None, dg.make("uniform", 7 * e + 1, seed=1), victim, victim, victim]
    EMPTY, NULL_IN, RAGGED, NULL_OUT, MIS_OUT, SHORT = range(3, 9)
    inp = tf.Inputs(torch, datas)
    bound = ghf.compress_batch_planes_shared_bound(w.max_item, e)
    sizes = tf.Packed(env, inp, w.d_codes, e, w.max_item).run()
    caps = [bound] * (len(datas) * e)
    caps[SHORT * e + 1] = int(sizes.h_bytes[SHORT * e + 1]) - 1
    sizes.free()
    want = [s for s in [OK, OK, OK, E_EMPTY, E_INVAL, E_INVAL, OK, OK, OK] for _ in range(e)]
    want[NULL_OUT * e] = want[MIS_OUT * e + e - 1] = E_INVAL
    want[SHORT * e + 1] = E_CAP
    for d_codes, want in ((w.d_codes, want), (bad_code_1(w), [E_FORMAT if j % e == 1 else s for j, s in enumerate(want)])):
        runs = []
        for raw in (None, 0):
            b = tf.Packed(env, inp, d_codes, e, w.max_item, raw=raw, caps=caps)
            ptrs = [int(x) for x in b.out_ptrs.cpu().tolist()]
            ptrs[NULL_OUT * e] = 0
            ptrs[MIS_OUT * e + e - 1] += 8
            b.out_ptrs = tf.i64(torch, ptrs)
            runs.append(b.run())
            b.free()
        p, t = runs
        print("parent", p.h_status.tolist(), p.h_bytes.tolist(), "\ntwin  ", t.h_status.tolist(), t.h_bytes.tolist())
        assert p.h_status.tolist() == want
        assert t.h_status.tolist() == want and np.array_equal(t.h_bytes, p.h_bytes)
        assert np.array_equal(t.h_out, p.h_out)  # every body, and every guard byte around them
        assert np.array_equal(t.h_chunk, p.h_chunk) and np.array_equal(t.h_seg, p.h_seg)
        assert all((s == OK) == (n > 0) for s, n in zip(p.h_status, p.h_bytes))
