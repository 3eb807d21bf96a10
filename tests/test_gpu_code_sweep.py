"""GPU: every code shape of tests/code_sweep.py through every kernel family that takes a caller's code.

Nothing expected comes from the library: the codes are orc.build_code's, an item's image is the code's header followed by
orc_encode_body, run records and seek tables and side-cars are summed from the oracle's code lengths (code_sweep.record_of,
range_worlds.expected_table, code_sweep.expected_index), typed tensors are numpy interleavings.  Every output is compared
byte for byte and sits between guard bytes that are checked afterwards; inputs sit at odd addresses (the Inputs packing of
the batch tests).  The call helpers are those of the batch and planes test modules, imported as they are.

The ids say where to look.  The staged and the shared-code family run once per group of the pool, `c<decoder class>-
len<min>..<max>-b<live-symbol bucket>` (the groups are pinned in tests/golden/golden_code_sweep.json; at most PER_GROUP
codes each, which keeps an id in tens of milliseconds; the 20 003-symbol item of every 32-bit code takes the staged path in
ids of its own); the two per-item-table families take a whole decoder class in one
launch; the typed families run per element width and per decoder class of plane 0 (plane p has class (that + p) % 6).
A failure names the code's label and the item, e.g. `chain/fib/k32/first :: deep/4097`: code_sweep.pool() and
code_sweep.items() give that case alone.  GHF_CODE_SWEEP_PER_GROUP raises the draw of 4 codes per group for a longer local
run (the CPU pins hold for 4)."""
import json
import os

import numpy as np
import pytest

import code_sweep as cs
import pkgload
from guarded import GUARD, PAD, Arena, first_diff  # noqa: F401
import test_gpu_batch_bodies as t_bodies
import test_gpu_batch_images as t_images
import test_gpu_batch_planes as t_planes
import test_gpu_batch_seek as t_seek
import test_gpu_batch_shared as t_shared

pytestmark = pytest.mark.gpu

OK = 0
PER_GROUP = int(os.environ.get("GHF_CODE_SWEEP_PER_GROUP", cs.PER_GROUP))
CLASSES = (0, 1, 2, 3, 4, 5)
MAX_SYMBOLS = 6 * 4096  # a side-car slice for the longest item: 6 blocks and 384 segments, so every slice is 16-byte aligned
CARS = 16               # slices: two per item of a code, one per plane of a tensor
assert MAX_SYMBOLS >= cs.BOUND_EXACT_N
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_code_sweep.json")) as _f:
    _pins = json.load(_f)
GROUPS = [tuple(g) for g in _pins["groups"]]  # (min_len, max_len, decoder class, bucket); test_code_sweep_cpu pins them
# the staged family costs the most per code: it takes a group in halves, every second code each
HALVES = [(g, k) for g, size in zip(GROUPS, _pins["group_sizes"]) for k in range(2 if size > 1 else 1)]


def group_id(g):
    return "c%d-len%d..%d-b%d" % (g[2], g[0], g[1], g[3])


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    pkg = pkgload.load()
    ctx = pkg.ghf.Context(0)
    yield pkg.ghf, ctx, torch
    ctx.close()


@pytest.fixture(scope="module")
def cars(env):
    """CARS side-car slices of MAX_SYMBOLS symbols; ghf.batch_index_item cuts an ordinary ghf_index out of one"""
    ghf, ctx, torch = env
    bidx = ctx.batch_index_alloc(CARS, MAX_SYMBOLS)
    yield bidx
    ctx.batch_index_free(bidx)


@pytest.fixture(scope="module", autouse=True)
def sweep():
    """the pool, its items and the typed cases, made once before the first id runs"""
    pool = cs.pool(PER_GROUP)
    assert sorted({e.group for e in pool}) == GROUPS
    for e in pool:
        cs.items(e, PER_GROUP)
    for w in cs.WIDTHS:
        cs.typed_cases(w, PER_GROUP)
    return pool


@pytest.fixture(scope="module", autouse=True)
def warm(env, cars, sweep):
    """the first launch of a kernel loads its code object: both per-group families run once on the first code here, so
    that no id's time depends on the order in which the ids run"""
    e = sweep[0]
    staged_code(env, cars, e, items_of(e))
    shared_code_batch(env, e)


def entries_of(variant):
    out = [e for e in cs.pool(PER_GROUP) if e.variant == variant]
    assert out, variant
    return out


def entries_in(group):
    out = [e for e in cs.pool(PER_GROUP) if e.group == group]
    assert out, group
    return out


def items_of(entry):
    return cs.items(entry, PER_GROUP)


def to_dev(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def emit_cap(image_bytes):
    """the smallest capacity ghf_encode_emit takes for an image of this size: through the 16-byte unit that holds its end bit"""
    return ((8 * image_bytes >> 7) + 1) << 4


def cars_to_host(ghf, ctx, cars):
    """every slice of `cars` -> (chunk_bit u64[CARS, blocks], seg_bit u32[CARS, segs]); synchronises"""
    chunk = np.zeros((CARS, cars.blocks_per_item), dtype=np.uint64)
    seg = np.zeros((CARS, cars.segs_per_item), dtype=np.uint32)
    L = ghf.lib()
    assert L.ghf_copy_d2h(ctx.h, chunk.ctypes.data, cars.d_chunk_bit, chunk.nbytes) == 0
    assert L.ghf_copy_d2h(ctx.h, seg.ctypes.data, cars.d_seg_bit, seg.nbytes) == 0
    ctx.sync()
    return chunk, seg


def check_car(chunk, seg, k, data, entry, where):
    want_chunk, want_seg = cs.expected_index(data, entry.length, entry.first_bit)
    assert np.array_equal(chunk[k, : want_chunk.size], want_chunk) and np.array_equal(seg[k, : want_seg.size], want_seg), where


# ------------------------------------------------------------------------------ 1. the staged flat path
def staged_code(env, cars, e, its):
    """items of one code: everything is queued into one arena, one copy brings it back"""
    ghf, ctx, torch = env
    assert 2 * len(its) <= CARS
    d_code = t_shared.code_to_device(torch, e.code)
    inp = t_shared.Inputs(torch, [it.data for it in its])
    offs = (inp.in_ptrs.cpu().numpy() - inp.d_in.data_ptr()).tolist()
    a, plan = Arena(), []
    for it in its:
        image, table = it.image, it.table
        r = {"image": image, "table": table, "info": ghf.seek_parse(table)}
        assert r["info"].n_symbols == it.n and table.size == ghf.seek_bytes(it.n), it
        r["stream"], r["tab"] = a.add(emit_cap(image.size)), a.add(table.size)
        # the decoders' outputs: 16-byte stores, and the byte-store path
        r["car"], r["exp"], r["k6"] = a.add(it.n), a.add(it.n, skew=3), a.add(it.n, skew=9)
        r["rng"] = [[a.add(count, skew=(first + 5 * j + 3 * s) % 16) for s in (0, 1)] for j, (first, count) in enumerate(it.ranges)]
        plan.append(r)
    a.alloc(torch)
    meta = torch.full((len(its), 8), -1, dtype=torch.int64, device="cuda")
    for i, (it, o, r) in enumerate(zip(its, offs, plan)):
        assert o % 2 == 1
        d_in, n, nb, info = inp.d_in[o : o + it.n], it.n, int(r["image"].size), r["info"]
        ix0, ix1 = ghf.batch_index_item(cars, 2 * i, n), ghf.batch_index_item(cars, 2 * i + 1, n)
        d_stream, d_table = a.view(r["stream"]), a.view(r["tab"])
        ctx.encode_plan(d_in, d_code, total=meta[i, 0:1])
        ctx.encode_emit(d_in, d_code, d_stream, flags=ghf.EMIT_HEADER | ghf.EMIT_LAST, index=ix0, end=meta[i, 1:3])
        ctx.decode(d_stream, nb, d_code, ix0, d_out=a.view(r["car"]), nbytes=meta[i, 3:4])
        ctx.seek_pack(ix0, d_table=d_table)
        ctx.seek_expand(info, d_table, d_stream, nb, d_code, index=ix1)
        ctx.decode(d_stream, nb, d_code, ix1, d_out=a.view(r["exp"]), nbytes=meta[i, 4:5])
        for (first, count), (by_car, by_table) in zip(it.ranges, r["rng"]):
            ctx.decode_range(d_stream, nb, d_code, first, count, index=ix0, d_out=a.view(by_car))
            ctx.decode_range(d_stream, nb, d_code, first, count, info=info, d_table=d_table, d_out=a.view(by_table))
        ctx.decode(d_stream, nb, d_code, None, d_out=a.view(r["k6"]), nbytes=meta[i, 5:6])  # K6 rebuilds the side-car (synchronises)
    ctx.sync()
    clean = a.fetch()
    chunk, seg = cars_to_host(ghf, ctx, cars)
    h_meta = meta.cpu().tolist()
    for i, (it, r) in enumerate(zip(its, plan)):
        m, n, nb = h_meta[i], it.n, int(r["image"].size)
        assert m[0] == int(e.length[it.data].sum()) and m[1:3] == [8 * nb, nb], (it, "encode_plan / encode_emit", m)
        got = a.got(r["stream"], nb)
        assert np.array_equal(got, r["image"]), (it, "encode_emit", first_diff(got, r["image"]))
        check_car(chunk, seg, 2 * i, it.data, e, (it, "encode_emit's side-car"))
        check_car(chunk, seg, 2 * i + 1, it.data, e, (it, "seek_expand's side-car"))
        assert np.array_equal(a.got(r["tab"]), r["table"]), (it, "seek_pack", first_diff(a.got(r["tab"]), r["table"]))
        assert m[3:6] == [n, n, n], (it, "decoded sizes", m)
        for what, k in (("decode with the side-car", "car"), ("decode after seek_expand", "exp"), ("decode without side-car (K6)", "k6")):
            assert np.array_equal(a.got(r[k]), it.data), (it, what, first_diff(a.got(r[k]), it.data))
        for (first, count), regions in zip(it.ranges, r["rng"]):
            want = it.data[first : first + count]
            for what, k in zip(("side-car", "table"), regions):
                assert np.array_equal(a.got(k), want), (it, "decode_range from the " + what, first, count, first_diff(a.got(k), want))
    assert clean, (e.label, "guard bytes")


@pytest.mark.parametrize("half", HALVES, ids=lambda h: group_id(h[0]) + "-" + "ab"[h[1]])
def test_staged_flat_path(env, cars, half):
    """ghf_encode_plan + ghf_encode_emit(HEADER | LAST, index) under the pool code, ghf_decode with that side-car, with the one
    ghf_seek_expand makes of the packed table, and with none (K6); ghf_seek_pack; ghf_decode_range from both sources"""
    group, k = half
    mine = entries_in(group)[k :: 2 if (group, 1) in HALVES else 1]
    assert mine, half
    for e in mine:
        staged_code(env, cars, e, [it for it in items_of(e) if it.mode != "deepest"])


@pytest.mark.parametrize("group", [g for g in GROUPS if g[1] == 32], ids=group_id)
def test_staged_flat_path_of_the_item_that_fills_the_bound(env, cars, group):
    """the same calls on the 20 003 deepest symbols of every 32-bit code, in ids of their own: a stream of nothing but equal
    32-bit codes is the slowest K6 has to find its way through"""
    for e in entries_in(group):
        its = [it for it in items_of(e) if it.mode == "deepest"]
        assert len(its) == 1, e.label
        staged_code(env, cars, e, its)


# ------------------------------------------------------------------------------ 2. per-item tables
def class_images(variant):
    its = [it for e in entries_of(variant) for it in items_of(e)]
    return its, [it.image for it in its]


@pytest.mark.parametrize("variant", CLASSES)
def test_images_batch_with_per_item_tables(env, variant):
    """every header || body image of the class in one ghf_decode_images_batch launch: the sizes-only pass with d_codes,
    which must be the host parser's tables byte for byte, then the decode pass"""
    ghf, ctx, torch = env
    its, images = class_images(variant)
    im = t_images.Images(torch, images)
    status, nbytes, _, _, codes = t_images.run(env, im, want_codes=True)
    for i, it in enumerate(its):
        assert (int(status[i]), int(nbytes[i])) == (OK, it.n), (it, "sizes pass", int(status[i]), int(nbytes[i]))
        want, hs = ghf.parse_header(images[i])
        assert hs == it.entry.header.size and codes[i].tobytes() == bytes(want), (it, "d_codes")
    status, nbytes, outs, guards, _ = t_images.run(env, im, caps=[it.n for it in its])
    for i, it in enumerate(its):
        assert (int(status[i]), int(nbytes[i])) == (OK, it.n), (it, "decode pass", int(status[i]), int(nbytes[i]))
        assert np.array_equal(outs[i], it.data), (it, first_diff(outs[i], it.data))
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (it, "guard bytes")


@pytest.mark.parametrize("variant", CLASSES)
def test_decode_batch_with_per_item_tables(env, variant):
    """the same images in one ghf_decode_batch launch: item i with its own tables (the oracle's) and a side-car slice that
    is written here from the oracle's code lengths"""
    ghf, ctx, torch = env
    its, images = class_images(variant)
    count, max_item = len(its), max(it.n for it in its)
    im = t_images.Images(torch, images)
    d_codes = t_seek.codes_to_device(torch, [it.entry.code for it in its])
    bidx = ctx.batch_index_alloc(count, max_item)
    try:
        chunk = np.zeros(count * bidx.blocks_per_item, dtype=np.uint64)
        seg = np.zeros(count * bidx.segs_per_item, dtype=np.uint32)
        for i, it in enumerate(its):
            c, s = cs.expected_index(it.data, it.entry.length, it.entry.first_bit)
            chunk[i * bidx.blocks_per_item :][: c.size] = c
            seg[i * bidx.segs_per_item :][: s.size] = s
        L = ghf.lib()
        assert L.ghf_copy_h2d(ctx.h, bidx.d_chunk_bit, chunk.ctypes.data, chunk.nbytes) == 0
        assert L.ghf_copy_h2d(ctx.h, bidx.d_seg_bit, seg.ctypes.data, seg.nbytes) == 0
        ctx.sync()
        a = Arena()
        regions = [a.add(it.n, skew=1 + i % 15) for i, it in enumerate(its)]
        a.alloc(torch)
        out_ptrs = t_images.i64(torch, [a.view(r).data_ptr() for r in regions])
        sizes = t_images.i64(torch, [it.n for it in its])
        r = ctx.decode_batch(im.ptrs, im.bytes, d_codes, bidx, sizes, out_ptrs=out_ptrs, out_caps=sizes)
        ctx.sync()
        clean = a.fetch()
        status, nbytes = r["status"].cpu().numpy(), r["out_bytes"].cpu().numpy()
        for i, it in enumerate(its):
            assert (int(status[i]), int(nbytes[i])) == (OK, it.n), (it, int(status[i]), int(nbytes[i]))
            assert np.array_equal(a.got(regions[i]), it.data), (it, first_diff(a.got(regions[i]), it.data))
        assert clean, "guard bytes"
    finally:
        ctx.batch_index_free(bidx)


# ------------------------------------------------------------------------------ 3. one shared code per batch
def shared_code_batch(env, e):
    ghf, ctx, torch = env
    its = items_of(e)
    datas, bodies, records = [it.data for it in its], [it.body for it in its], [it.record for it in its]
    want_sizes = [it.n for it in its]
    max_item = max(want_sizes)
    bound = ghf.compress_batch_shared_bound(max_item)
    assert all(b.size <= bound for b in bodies), e.label
    if e.max_len == 32:
        assert its[-1].mode == "deepest" and bodies[-1].size == bound, its[-1]  # the body that fills the bound to the byte
    d_code = t_shared.code_to_device(torch, e.code)
    inp = t_shared.Inputs(torch, datas)
    caps = [bodies[i].size if i % 3 == 0 else bound for i in range(len(its))]  # "nothing at or beyond the cap" bites
    b = t_shared.Shared(ghf, ctx, torch, inp, d_code, max_item, caps=caps).run()
    try:
        for i, it in enumerate(its):
            assert (int(b.h_status[i]), int(b.h_bytes[i])) == (OK, bodies[i].size), (it, "compress", int(b.h_status[i]), int(b.h_bytes[i]))
            assert np.array_equal(b.body(i), bodies[i]), (it, "compress", first_diff(b.body(i), bodies[i]))
            assert np.all(b.slot(i)[caps[i] :] == GUARD), (it, "compress wrote at or beyond its cap")
        # the live side-car
        status, out_bytes, outs, guards = t_shared.decode_shared(b)
        for i, it in enumerate(its):
            assert (int(status[i]), int(out_bytes[i])) == (OK, it.n), (it, "decode_batch_shared", int(status[i]), int(out_bytes[i]))
            assert np.array_equal(outs[i], it.data), (it, "decode_batch_shared", first_diff(outs[i], it.data))
            assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (it, "decode_batch_shared: guard bytes")
        # the run records of that side-car
        status, rec_bytes, slots = t_seek.pack(env, b.bidx, inp.in_bytes)
        for i, it in enumerate(its):
            rec = records[i]
            assert (int(status[i]), int(rec_bytes[i])) == (OK, rec.size), (it, "batch_seek_pack", int(status[i]), int(rec_bytes[i]))
            assert rec.size == ghf.batch_seek_bytes(it.n), it
            assert np.array_equal(slots[i][: rec.size], rec), (it, "batch_seek_pack", first_diff(slots[i][: rec.size], rec))
            assert np.all(slots[i][rec.size :] == GUARD), (it, "batch_seek_pack wrote behind its record")
    finally:
        b.free()
    # from nothing but the bodies; from the bodies and their records (the oracle's bytes, in buffers of their own)
    bo = t_bodies.Bodies(torch, bodies)
    ro = t_seek.Packed(torch, records)
    passes = [("decode_bodies_batch_shared", lambda caps: t_bodies.run(env, bo, d_code, caps=caps)),
              ("decode_bodies_batch_shared_seek", lambda caps: t_seek.run(env, bo, ro, d_code, caps=caps))]
    for what, call in passes:
        status, nbytes, _, _ = call(None)
        assert status.tolist() == [OK] * len(its) and nbytes.tolist() == want_sizes, (e.label, what, "sizes pass", status.tolist(), nbytes.tolist())
        status, nbytes, outs, guards = call(want_sizes)
        for i, it in enumerate(its):
            assert (int(status[i]), int(nbytes[i])) == (OK, it.n), (it, what, int(status[i]), int(nbytes[i]))
            assert np.array_equal(outs[i], it.data), (it, what, first_diff(outs[i], it.data))
            assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (it, what + ": guard bytes")


@pytest.mark.parametrize("group", GROUPS, ids=group_id)
def test_shared_code_batches(env, group):
    """per code one batch of its items: ghf_compress_batch_shared (the cap exactly the body on every third slot),
    ghf_decode_batch_shared, ghf_batch_seek_pack, ghf_decode_bodies_batch_shared and .._seek with their sizes-only passes"""
    for e in entries_in(group):
        shared_code_batch(env, e)


# ------------------------------------------------------------------------------ 4. typed tensors, one code per byte plane
def plane_cars(ghf, cars, e, n):
    return (ghf.Index * e)(*[ghf.batch_index_item(cars, p, n) for p in range(e)])


def slot_bytes_for(ghf, t):
    """a slot for any plane's image: the library's own bound counts 9 bits per symbol, a caller's code may take 32"""
    need = max(emit_cap(t.image(p).size) for p in range(t.e))
    return max(ghf.planes_slot_bytes(t.n), need + 15 & ~15)


class TypedRun:
    """what the coded and the delta form share: the E codes and side-cars, an arena with the slots of the images, the
    seek tables and one output per range and source"""

    def __init__(self, env, cars, t):
        self.env, self.t = env, t
        ghf, ctx, torch = env
        e, n = t.e, t.n
        self.d_codes = t_seek.codes_to_device(torch, [en.code for en in t.entries])
        self.idx = plane_cars(ghf, cars, e, n)
        self.images, self.tables = [t.image(p) for p in range(e)], [t.table(p) for p in range(e)]
        self.sizes = [int(im.size) for im in self.images]
        self.infos = [ghf.seek_parse(tab) for tab in self.tables]
        self.slot = slot_bytes_for(ghf, t)
        self.a = a = Arena()
        self.r_slots = a.add(e * self.slot)
        self.r_tabs = [a.add(tab.size) for tab in self.tables]
        self.r_full = [a.add(n * e), a.add(n * e)]
        self.r_rng = [[a.add(count * e), a.add(count * e)] for first, count in t.ranges]
        a.alloc(torch)
        self.d_out = a.view(self.r_slots)
        self.streams = [self.d_out[p * self.slot : (p + 1) * self.slot] for p in range(e)]
        self.d_tables = [a.view(r) for r in self.r_tabs]
        self.sources = (("side-cars", {"indexes": self.idx}), ("seek tables", {"infos": self.infos, "d_tables": self.d_tables}))

    def pack_tables(self):
        for p in range(self.t.e):
            self.env[1].seek_pack(self.idx[p], d_table=self.d_tables[p])

    def check(self, cars, r, what, full, want_full, want_range):
        """after the last call: sizes, images, side-cars, tables, the two whole outputs, the ranges, the guard bytes"""
        ghf, ctx, torch = self.env
        t, a = self.t, self.a
        ctx.sync()
        clean = a.fetch()
        chunk, seg = cars_to_host(ghf, ctx, cars)
        sizes = [int(v) for v in r["out_bytes"].cpu().numpy()]
        for p in range(t.e):
            assert sizes[p] == self.sizes[p], (t, what, "plane %d" % p, sizes[p], self.sizes[p])
            got = a.got(self.r_slots)[p * self.slot :][: self.sizes[p]]
            assert np.array_equal(got, self.images[p]), (t, what, "plane %d" % p, first_diff(got, self.images[p]))
            check_car(chunk, seg, p, t.planes[p], t.entries[p], (t, what, "side-car of plane %d" % p))
            got = a.got(self.r_tabs[p])
            assert np.array_equal(got, self.tables[p]), (t, what, "seek_pack of plane %d" % p, first_diff(got, self.tables[p]))
        for (name, nb), k in zip(full, self.r_full):
            assert int(nb.item()) == t.n * t.e and np.array_equal(a.got(k), want_full), (t, name, first_diff(a.got(k), want_full))
        for (first, count), regions in zip(t.ranges, self.r_rng):
            want = want_range[first * t.e : (first + count) * t.e]
            for (src, _), k in zip(self.sources, regions):
                assert np.array_equal(a.got(k), want), (t, what, "range from " + src, first, count, first_diff(a.got(k), want))
        assert clean, (t, what, "guard bytes")


def typed_coded(env, cars, t):
    ghf, ctx, torch = env
    e, n = t.e, t.n
    w = TypedRun(env, cars, t)
    r = ctx.compress_planes_coded(to_dev(torch, t.tensor), e, d_codes=w.d_codes, flags=0, n_elems=n, d_out=w.d_out, slot_bytes=w.slot,
                                  indexes=w.idx)
    w.pack_tables()
    _, nb_car = ctx.decode_planes(w.streams, w.sizes, w.d_codes, n, e, indexes=w.idx, d_out=w.a.view(w.r_full[0]))
    for (first, count), regions in zip(t.ranges, w.r_rng):
        for (_, src), k in zip(w.sources, regions):
            ctx.decode_planes_range(w.streams, w.sizes, w.d_codes, e, first, count, d_out=w.a.view(k), **src)
    _, nb_k6 = ctx.decode_planes(w.streams, w.sizes, w.d_codes, n, e, indexes=None, d_out=w.a.view(w.r_full[1]))  # (synchronises)
    w.check(cars, r, "compress_planes_coded", (("decode_planes with side-cars", nb_car), ("decode_planes without side-cars", nb_k6)),
            t.tensor, t.tensor)


def typed_delta(env, cars, t):
    ghf, ctx, torch = env
    e, n = t.e, t.n
    w = TypedRun(env, cars, t)
    d_base = to_dev(torch, t.base)
    # the base elements of every range, each part at a 16-byte aligned address of one upload
    at, cuts = 0, []
    for first, count in t.ranges:
        cuts.append((at, count * e))
        at += count * e + 15 & ~15
    h_parts = np.zeros(at, dtype=np.uint8)
    for (o, k), (first, count) in zip(cuts, t.ranges):
        h_parts[o : o + k] = t.base[first * e : (first + count) * e]
    d_parts = to_dev(torch, h_parts)
    r = ctx.compress_planes_delta(to_dev(torch, t.new), d_base, e, d_codes=w.d_codes, flags=0, n_elems=n, d_out=w.d_out,
                                  slot_bytes=w.slot, indexes=w.idx)
    w.pack_tables()
    _, nb_out = ctx.decode_planes_delta(w.streams, w.sizes, w.d_codes, d_base, n, e, indexes=w.idx, d_out=w.a.view(w.r_full[0]))
    in_place = w.a.view(w.r_full[1])
    in_place.copy_(d_base)
    _, nb_in = ctx.decode_planes_delta(w.streams, w.sizes, w.d_codes, in_place, n, e, indexes=w.idx, d_out=in_place)
    for (first, count), regions, (o, k) in zip(t.ranges, w.r_rng, cuts):
        for (_, src), reg in zip(w.sources, regions):
            ctx.decode_planes_range_delta(w.streams, w.sizes, w.d_codes, d_parts[o : o + k], e, first, count, d_out=w.a.view(reg), **src)
    w.check(cars, r, "compress_planes_delta", (("decode_planes_delta out of place", nb_out), ("decode_planes_delta in place", nb_in)),
            t.new, t.new)


def typed_batch(env, cars, t):
    """the tensor, its first half and its first element as one batch under the case's E codes"""
    ghf, ctx, torch = env
    e = t.e
    counts = sorted({t.n, max(t.n // 2, 1), 1}, reverse=True)
    datas = [np.ascontiguousarray(t.tensor[: k * e]) for k in counts]
    planes = [[np.ascontiguousarray(d[p::e]) for p in range(e)] for d in datas]
    bodies = [cs.orc_body(pl[p], t.entries[p].code) for pl in planes for p in range(e)]                # by slot
    records = [cs.orc_record(pl[p], t.entries[p].length) for pl in planes for p in range(e)]
    max_item = t.n * e
    bound = ghf.compress_batch_planes_shared_bound(max_item, e)
    assert all(b.size <= bound for b in bodies), t
    d_codes = t_seek.codes_to_device(torch, [en.code for en in t.entries])
    inp = t_planes.Inputs(torch, datas)
    caps = [bodies[j].size if j % 3 == 0 else bound for j in range(len(bodies))]
    b = t_planes.Planes(ghf, ctx, torch, inp, d_codes, e, max_item, caps=caps).run()
    want_bytes = [d.size for d in datas]
    try:
        for j, body in enumerate(bodies):
            where = (t, "item %d plane %d" % divmod(j, e))
            assert (int(b.h_status[j]), int(b.h_bytes[j])) == (OK, body.size), (where, "compress", int(b.h_status[j]), int(b.h_bytes[j]))
            assert np.array_equal(b.body(j), body), (where, "compress", first_diff(b.body(j), body))
            assert np.all(b.slot(j)[caps[j] :] == GUARD), (where, "compress wrote at or beyond its cap")
        status, nbytes, _, _ = t_planes.decode(b, live=False, sizes_only=True)
        assert status.tolist() == [OK] * len(datas) and nbytes.tolist() == want_bytes, (t, "bodies decoder, sizes pass", status.tolist(), nbytes.tolist())
        for what, live in (("decode_batch_planes_shared", True), ("decode_bodies_batch_planes_shared", False)):
            status, nbytes, outs, guards = t_planes.decode(b, live=live)
            for i, d in enumerate(datas):
                assert (int(status[i]), int(nbytes[i])) == (OK, d.size), (t, what, "item %d" % i, int(status[i]), int(nbytes[i]))
                assert np.array_equal(outs[i], d), (t, what, "item %d" % i, first_diff(outs[i], d))
                assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (t, what, "item %d" % i, "guard bytes")
        status, rec_bytes, slots = t_seek.pack(env, b.bidx, inp.in_bytes, e=e)
        for j, rec in enumerate(records):
            where = (t, "item %d plane %d" % divmod(j, e))
            assert (int(status[j]), int(rec_bytes[j])) == (OK, rec.size), (where, "batch_seek_pack", int(status[j]), int(rec_bytes[j]))
            assert np.array_equal(slots[j][: rec.size], rec), (where, "batch_seek_pack", first_diff(slots[j][: rec.size], rec))
            assert np.all(slots[j][rec.size :] == GUARD), (where, "batch_seek_pack wrote behind its record")
    finally:
        b.free()
    bo, ro = t_seek.Packed(torch, bodies), t_seek.Packed(torch, records)
    status, nbytes, _, _ = t_seek.run(env, bo, ro, d_codes, e=e)
    assert status.tolist() == [OK] * len(datas) and nbytes.tolist() == want_bytes, (t, "planes seek decoder, sizes pass", status.tolist(), nbytes.tolist())
    status, nbytes, outs, guards = t_seek.run(env, bo, ro, d_codes, caps=want_bytes, e=e)
    for i, d in enumerate(datas):
        assert (int(status[i]), int(nbytes[i])) == (OK, d.size), (t, "planes seek decoder", "item %d" % i, int(status[i]), int(nbytes[i]))
        assert np.array_equal(outs[i], d), (t, "planes seek decoder", "item %d" % i, first_diff(outs[i], d))
        assert np.all(guards[i][0] == GUARD) and np.all(guards[i][1] == GUARD), (t, "planes seek decoder", "item %d" % i, "guard bytes")


TYPED = {"coded": typed_coded, "delta": typed_delta, "batch": typed_batch}


@pytest.mark.parametrize("lead", CLASSES, ids=["c%d" % c for c in CLASSES])
@pytest.mark.parametrize("e", cs.WIDTHS)
@pytest.mark.parametrize("family", list(TYPED))
def test_typed(env, cars, family, e, lead):
    """coded: ghf_compress_planes_coded with the caller's E codes, ghf_decode_planes with and without side-cars,
    ghf_decode_planes_range from side-cars and from seek tables.  delta: ghf_compress_planes_delta with the same codes,
    ghf_decode_planes_delta out of place and in place, ghf_decode_planes_range_delta.  batch: ghf_compress_batch_planes_shared,
    both plane decoders, ghf_batch_seek_pack and the planes seek decoder.  `lead`: the decoder class of plane 0"""
    cases = [t for t in cs.typed_cases(e, PER_GROUP) if t.variants[0] == lead]
    assert len(cases) >= cs.TYPED_CASES // 6
    for t in cases:
        TYPED[family](env, cars, t)
