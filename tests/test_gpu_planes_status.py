"""GPU: the status guard of the six merge kernels of golden-huffman_amd/csrc/ghf_planes.hip (merge_body), each width, reached
through the decode call that queues it:

    ghf_decode_planes                k_planes_merge<E>
    ghf_decode_planes_delta          k_planes_merge_delta<E>
    ghf_decode_planes_range          k_planes_merge_range<E>
    ghf_decode_planes_range_delta    k_planes_merge_range_delta<E>
    ghf_decode_planes_forms          k_planes_merge_from<E, false / true>        (plane 0 raw; without and with a base)
    ghf_decode_planes_forms_range    k_planes_merge_range_from<E, false / true>

The last dense plane's side-car lies by one bit, as in test_a_lying_side_car_leaves_the_output_alone_and_in_place_the_base of
tests/test_gpu_planes_delta.py and test_gpu_planes_forms.py (whose tensors, compress helpers and guard helpers these are):
the decoder's end-to-end check of the segment latches GHF_E_CORRUPT and the merge queued behind it must store nothing.  The
ranges start 5 bytes into a 16-byte vector of every plane, so they run the skewed kernels; a range decodes only the blocks
it covers, so for them the lie sits in block 1 and not in block 4."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_planes_delta as tpd
import test_gpu_planes_forms as tf
from test_gpu_planes_forms import env  # noqa: F401  (the fixture: ghf, a context, torch)

pytestmark = pytest.mark.gpu

OK, E_CORRUPT = tf.OK, tf.E_CORRUPT
PAD = tf.PAD
N = 65536 + 3
FIRST, COUNT = 4101, 4099
assert FIRST % 16 and FIRST // 4096 == 1 and (FIRST + COUNT - 1) // 4096 == 2
CALLS = ("decode_planes", "decode_planes_delta", "decode_planes_range", "decode_planes_range_delta", "decode_planes_forms",
         "decode_planes_forms_base", "decode_planes_forms_range", "decode_planes_forms_range_base")


class Stored:
    """the stepped pair of tests/test_gpu_planes_delta.py stored once in every way the calls read: the planes of `new`, the
    planes of new ^ base, and both again with plane 0 raw"""

    def __init__(self, ghf, ctx, torch, e):
        self.e = e
        self.new, self.base = tpd.stepped(N, e)
        d_new = tf.to_dev(torch, self.new)
        self.idx = ctx.planes_index_alloc(N, e)
        self.r = ctx.compress_planes(d_new, e, n_elems=N, indexes=self.idx)
        self.r_delta, _, _, self.idx_delta, self.d_base = tpd.compressed(ghf, ctx, torch, e, N)
        self.d_base_of_range = self.d_base[FIRST * e : (FIRST + COUNT) * e].clone()  # indexed like the output, and aligned
        self.r_forms = [tf.compress_forms(ghf, ctx, torch, d_new, b, e, N, 0b1, 0) for b in (None, self.d_base)]
        ctx.sync()

    def free(self, ctx):
        for idx in (self.idx, self.idx_delta, self.r_forms[0]["indexes"], self.r_forms[1]["indexes"]):
            ctx.planes_index_free(idx)

    def side_cars(self, call):
        return (self.r_forms["base" in call]["indexes"] if "forms" in call else self.idx_delta if "delta" in call else self.idx)

    def decode(self, ctx, call, indexes, out):
        e, ranged = self.e, "range" in call
        cap = (COUNT if ranged else N) * e
        if "forms" in call:
            r = self.r_forms["base" in call]
            base = None if "base" not in call else self.d_base_of_range if ranged else self.d_base
            sizes = [int(v) for v in tf.host(r["out_bytes"])]
            if ranged:
                ctx.decode_planes_forms_range(tf.slots_of(r), sizes, r["codes"], 0b1, 0, [None] * e, N, e, FIRST, COUNT, indexes=indexes,
                                              d_base=base, d_out=out, cap=cap)
            else:
                ctx.decode_planes_forms(tf.slots_of(r), sizes, r["codes"], 0b1, 0, r["n_vals"], N, e, indexes=indexes, d_base=base,
                                        d_out=out, cap=cap)
            return
        r = self.r_delta if "delta" in call else self.r
        slots = [r["out"][p * r["slot_bytes"] : (p + 1) * r["slot_bytes"]] for p in range(e)]
        sizes = [int(v) for v in tf.host(r["out_bytes"])]
        if call == "decode_planes":
            ctx.decode_planes(slots, sizes, r["codes"], N, e, indexes=indexes, d_out=out, cap=cap)
        elif call == "decode_planes_delta":
            ctx.decode_planes_delta(slots, sizes, r["codes"], self.d_base, N, e, indexes=indexes, d_out=out, cap=cap)
        elif call == "decode_planes_range":
            ctx.decode_planes_range(slots, sizes, r["codes"], e, FIRST, COUNT, indexes=indexes, d_out=out, cap=cap)
        else:
            ctx.decode_planes_range_delta(slots, sizes, r["codes"], self.d_base_of_range, e, FIRST, COUNT, indexes=indexes, d_out=out,
                                          cap=cap)


_stored = {}


@pytest.fixture(scope="module")
def stored(env):  # noqa: F811
    ghf, ctx, torch = env

    def get(e):
        if e not in _stored:
            _stored[e] = Stored(ghf, ctx, torch, e)
        return _stored[e]

    yield get
    for w in _stored.values():
        w.free(ctx)
    _stored.clear()


def lying(ghf, ctx, torch, idx, j, block):
    """a copy of the side-cars `idx` whose entry j puts the end of segment 63 of `block` one bit late (and the device arrays
    that entry points to, to be kept alive)"""
    chunk, seg = ctx.index_to_host(idx[j])
    seg = seg.copy()
    seg[block * 64 + 63] += 1
    keep = tf.to_dev(torch, chunk.view(np.uint8)), tf.to_dev(torch, seg.view(np.uint8))
    bad = (ghf.Index * len(idx))()
    C.memmove(bad, idx, C.sizeof(bad))
    bad[j].d_chunk_bit, bad[j].d_seg_bit = keep[0].data_ptr(), keep[1].data_ptr()
    return bad, keep


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("e", tf.WIDTHS)
def test_behind_a_lying_side_car_no_merge_kernel_stores_a_byte(env, stored, e, call):  # noqa: F811
    ghf, ctx, torch = env
    w = stored(e)
    ranged = "range" in call
    nbytes = (COUNT if ranged else N) * e
    want = w.new[FIRST * e : (FIRST + COUNT) * e] if ranged else w.new
    idx = w.side_cars(call)
    bad, keep = lying(ghf, ctx, torch, idx, e - 1, 1 if ranged else 4)
    buf = tf.guarded(torch, nbytes)
    w.decode(ctx, call, bad, buf[PAD:])
    assert ctx.L.ghf_sync(ctx.h) == E_CORRUPT
    assert tf.untouched(torch, buf)  # the pads too
    assert ctx.L.ghf_clear_status(ctx.h) == OK
    w.decode(ctx, call, idx, buf[PAD:])  # the true side-cars, on the same context
    assert ctx.L.ghf_sync(ctx.h) == OK
    assert np.array_equal(tf.host(buf[PAD : PAD + nbytes]), want) and tf.guards_intact(buf, nbytes)
    del keep
