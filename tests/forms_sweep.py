"""Every code shape for the forms, sparse-range and gather calls (numpy and the oracle only; no GPU, no numpy RNG: every
choice comes from datagen.splitmix64 through hist_families.words, as in tests/code_sweep.py, so the cases can never change).

tests/code_sweep.py drives the pool codes through the kernels that decode whole streams.  Three bit walkers take a caller's
code too and are not among them: k_seek_expand_streams (the sparse range calls from seek tables), and the gather walker on
dense planes and on the mask and values streams of sparse ones.  Here a tensor's stored streams are coded under pool codes:

  sparse plane   mask code A: any pool code; the mask is mb bytes drawn over A's live symbols (code_sweep.draw).  Values code
                 B: any pool code with a non-zero live byte symbol; the values are popcount(mask) bytes drawn over B's live
                 symbols without 0.  The plane is sparse_range_model.merge(mask, vals, n).  A mask of zeros (always so under a
                 code whose only live symbol is 0) is the all-zero plane: n_vals == 0, no values stream (form `z`)
  dense plane    n bytes drawn over a pool code's live symbols (form `d`);  raw plane: n splitmix64 bytes (form `w`)
  n              8 (mb - 1) + t, t = 8 in even cases, else the widest last mask byte of the tensor's sparse planes (at least
                 1): the pad bits are clear by construction and half the tensors are ragged

cases(e)       -> [Case] * FORMS_CASES: name, e, k, n, planes [Plane], tensor, base, new (= base ^ tensor), raw / sparse (the
                  two masks of planes), ranges [(first, count)] * 4, row_elems, firsts (stride 1, descending, the first repeated)
Plane          -> form, kind, data; main (the Stream of a dense plane or of a mask), values (Stream or None), mask, vals, rank
Stream         -> entry (the pool Entry), data, body (orc_encode_body), image (header || body), table (range_worlds.
                  expected_table), index (code_sweep.expected_index): all from the oracle's code lengths
typed_rows(e)  -> per code_sweep.typed_cases(e) tensor: (tensor, raw mask, row_elems, firsts) for ghf_decode_planes_gather
values_left_out() -> the labels of the pool codes that cannot be a values code: no non-zero live symbol; nothing else is skipped
sha256()       -> one digest over every case, pinned with coverage() in golden/golden_forms_sweep.json

How the codes are chosen: plane 0's first stream has decoder class k % 6 (the ids of tests/test_gpu_forms_sweep.py), the
values of a sparse plane 0 class (k + 3) % 6; every other stream takes the next max_len of its role's cycle through 1..32,
which runs on across the widths.  Plane 0 is sparse in cases 0..5, 12..17, 24..29 and dense in the others, so at every width
each role meets every class there.  At E = 2 a tensor is one sparse and one dense plane and has no room for a raw one."""
import functools
import hashlib

import numpy as np

import code_sweep as cs
import gather_forms_model as fm
import hist_families as hf
import range_worlds as rw
import sparse_range_model as srm

FORMS_CASES = 36
WIDTHS = cs.WIDTHS
MASK_BYTES = (1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 4613, 8191, 8192, 8257)
MASK_BYTES_MAX = 8257   # three rank blocks, the last one ragged; at most 66 056 elements
ROW_ELEMS_MAX = fm.SPARSE_MAX_ROW_ELEMS
TYPED_ROW_ELEMS_MAX = 4096
RANK = srm.RANK_ELEMS
ROLES = ("mask", "values", "dense")
ROLE_START = {"mask": 0, "values": 11, "dense": 22}  # where each role's cycle through max_len 1..32 begins
ZERO_CASE = 7           # cases k % 12 == 7: the last sparse plane's mask code has 0 as its only live symbol
# the planes behind plane 0 (which is `s` or `d`), rotated by k // 3; every third case holds a raw plane where there is room
TAILS = {2: {"s": ("d", "d"), "d": ("s", "s")},
         4: {"s": ("dsd", "dws"), "d": ("ssd", "wss")},
         8: {"s": ("dsdsdsd", "dwsdswd"), "d": ("sdsdsds", "swsdsws")}}
SEED_FORMS, SEED_FORMS_BASE, SEED_FORMS_RANGE, SEED_FORMS_ROWS, SEED_TYPED_ROWS = 0x5EED6000, 0x5EED7000, 0x5EED8000, 0x5EED9000, 0x5EEDA000


class NoZero:
    """a pool entry as code_sweep.draw sees it, with symbol 0 taken out of its live symbols"""

    def __init__(self, entry):
        self.length = entry.length
        self.live = entry.live[entry.live != 0]
        lens = self.length[self.live]
        self.deepest = int(self.live[np.flatnonzero(lens == lens.max())[-1]])


class Stream:
    """a byte string stored under a pool code: every stored byte is the oracle's"""

    def __init__(self, entry, data):
        self.entry, self.n = entry, int(data.size)
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.data.setflags(write=False)
        self.body = cs.orc_body(self.data, entry.code)
        self.image = np.concatenate((entry.header, self.body))
        self.table = rw.expected_table(self.data, entry.length, entry.first_bit)

    @property
    def index(self):
        return cs.expected_index(self.data, self.entry.length, self.entry.first_bit)

    def model(self, table=None):
        """the stream as gather_model.row_verdict takes it"""
        return {"table": self.table if table is None else table, "true_table": self.table, "stream": self.image,
                "stream_bytes": int(self.image.size), "length": [int(v) for v in self.entry.code.length],
                "codeword": [int(v) for v in self.entry.code.codeword], "code_ok": True, "data": self.data}


class Plane:
    def __init__(self, form, data, main=None, values=None, mask=None, vals=None):
        self.form, self.data, self.main, self.values, self.mask, self.vals = form, data, main, values, mask, vals
        self.kind = {"w": "raw", "d": "dense"}.get(form, "sparse")
        self.n_vals = int(vals.size) if self.kind == "sparse" else 0
        self.rank = srm.table_of(data) if self.kind == "sparse" else None
        data.setflags(write=False)

    @property
    def labels(self):
        return "/".join([self.form] + [s.entry.label for s in (self.main, self.values) if s is not None])

    def model(self, vals_stream=None):
        """the plane as gather_forms_model takes it"""
        if self.kind == "raw":
            return "raw", self.data
        if self.kind == "dense":
            return "dense", self.main.model()
        return "sparse", {"mask": self.mask, "vals": self.vals, "cum": srm.cum_in(self.rank), "n_vals": self.n_vals,
                          "mask_stream": self.main.model(),
                          "vals_stream": (self.values.model() if self.values else None) if vals_stream is None else vals_stream}


class Case:
    def __init__(self, e, k, n, planes, base, ranges, row_elems, firsts):
        self.e, self.k, self.n, self.planes, self.ranges, self.row_elems, self.firsts = e, k, n, planes, ranges, row_elems, firsts
        self.forms = "".join(p.form for p in planes)
        self.name = "E%d/case%02d/%s/n%d" % (e, k, self.forms, n)
        self.tensor = np.stack([p.data for p in planes], axis=1).reshape(-1)  # byte p of element k = planes[p][k]
        self.base = base
        self.new = base ^ self.tensor
        for a in (self.tensor, self.base, self.new):
            a.setflags(write=False)
        self.raw = sum(1 << i for i, p in enumerate(planes) if p.kind == "raw")
        self.sparse = sum(1 << i for i, p in enumerate(planes) if p.kind == "sparse")
        self.lead = planes[0].main.entry.variant  # the decoder class of plane 0's first stream

    def slots(self):
        """the 2 e stored slots: a Stream, a raw plane's bytes, or None"""
        e = self.e
        out = [None] * (2 * e)
        for i, p in enumerate(self.planes):
            out[i] = p.data if p.kind == "raw" else p.main
            out[e + i] = p.values
        return out

    def streams(self):
        return [s for s in self.slots() if isinstance(s, Stream)]

    def model_planes(self):
        return [p.model() for p in self.planes]

    def __repr__(self):
        return "%s :: %s" % (self.name, " | ".join(p.labels for p in self.planes))


# ---------------------------------------------------------------- which codes
def class_of(max_len):
    return rw.decoder_class(1, max_len)[0]


def has_values(entry):
    return bool(np.any(entry.live != 0))


def values_left_out():
    return [en.label for en in cs.pool() if not has_values(en)]


@functools.lru_cache(maxsize=None)
def _by_len():
    """role -> max_len -> [pool entries that may take the role]"""
    out = {r: {} for r in ROLES}
    for en in cs.pool():
        for r in ROLES:
            if r != "values" or has_values(en):
                out[r].setdefault(en.max_len, []).append(en)
    return out


def zero_only():
    return [en for en in cs.pool() if en.live.tolist() == [0]]


class _Chooser:
    """the next code of a role: by decoder class for plane 0, else by the role's cycle through max_len 1..32"""

    def __init__(self):
        self.at = dict(ROLE_START)

    def of_class(self, role, cls, turn, w):
        lens = [L for L in range(1, 33) if class_of(L) == cls]
        return self._pick(role, lens[turn % len(lens)], w)

    def next(self, role, w):
        L = 1 + self.at[role] % 32
        self.at[role] += 1
        return self._pick(role, L, w)

    @staticmethod
    def _pick(role, L, w):
        members = _by_len()[role][L]
        return members[int(w % np.uint64(len(members)))]


# ---------------------------------------------------------------- ranges and rows
def ranges_for(n, seed):
    """four (first, count): a drawn one, one of count 1, the whole tensor, and -- where n > 32768 -- one that starts in rank
    block 0 and ends in block 1"""
    a, b, c, d, f = (int(x) for x in hf.words(seed, 5))
    first = a % n
    out = [(first, 1 + b % (n - first)), (c % n, 1), (0, n)]
    if n > RANK:
        lo = d % RANK
        end = RANK + 1 + f % (min(n, 2 * RANK) - RANK)
        out.append((lo, end - lo))
    else:
        out.append((0, n))
    for lo, k in out:
        assert 0 <= lo and 1 <= k and lo + k <= n
    return out


def rows_for(n, seed, cap, edge):
    """-> (row_elems, firsts): row_elems = min(n, a drawn 1..cap); the firsts 0, n - row_elems, two drawn ones and -- with
    `edge` -- the row that straddles element 32768 where it fits; descending, the first of them repeated"""
    a, b, c = (int(x) for x in hf.words(seed, 3))
    row_elems = min(n, 1 + a % cap)
    room = n - row_elems + 1
    firsts = [0, n - row_elems, b % room, c % room]
    if edge and 0 <= RANK - row_elems // 2 and RANK - row_elems // 2 + row_elems <= n:
        firsts.append(RANK - row_elems // 2)
    firsts = sorted(dict.fromkeys(firsts), reverse=True)
    return row_elems, firsts + firsts[:1]


# ---------------------------------------------------------------- the cases
def _case(e, k, choose):
    seed = SEED_FORMS + 0x10000 * e + 256 * k
    w = hf.words(seed, 4 * e + 2)
    lead = "s" if (k // 6) % 2 == 0 else "d"
    tail = TAILS[e][lead][k % 3 == 2]
    turn = (k // 3) % len(tail)
    forms = lead + tail[turn:] + tail[:turn]
    mb = MASK_BYTES[k] if k < len(MASK_BYTES) else 1 + int(w[4 * e] % np.uint64(MASK_BYTES_MAX))
    sparse_planes = [p for p, f in enumerate(forms) if f == "s"]
    # the codes, in plane order; then the masks, which decide n
    codes, masks = {}, {}
    for p, f in enumerate(forms):
        if f == "s":
            if p == 0:
                a, b = choose.of_class("mask", k % 6, k // 6 + e, w[4 * p]), choose.of_class("values", (k + 3) % 6, k // 6 + e, w[4 * p + 1])
            else:
                a, b = choose.next("mask", w[4 * p]), choose.next("values", w[4 * p + 1])
            if k % 12 == ZERO_CASE and p == sparse_planes[-1]:
                zs = zero_only()
                a = zs[(k // 12 + e) % len(zs)]
            codes[p] = (a, b)
            masks[p] = cs.draw(a, cs.MODES[int(w[4 * p + 2] % np.uint64(4))], mb, seed + 8 + p)
        elif f == "d":
            codes[p] = (choose.of_class("dense", k % 6, k // 6 + e, w[4 * p]) if p == 0 else choose.next("dense", w[4 * p]),)
    t = 8 if k % 2 == 0 else max(1, max(int(m[-1]).bit_length() for m in masks.values()))
    n = 8 * (mb - 1) + t
    planes = []
    for p, f in enumerate(forms):
        mode = cs.MODES[int(w[4 * p + 3] % np.uint64(4))]
        if f == "s":
            a, b = codes[p]
            mask = masks[p]
            nv = int(np.unpackbits(mask, bitorder="little")[:n].sum())
            vals = cs.draw(NoZero(b), mode, nv, seed + 40 + p) if nv else np.zeros(0, dtype=np.uint8)
            data = srm.merge(mask, vals, n)
            planes.append(Plane("s" if nv else "z", data, main=Stream(a, mask), values=Stream(b, vals) if nv else None, mask=mask, vals=vals))
        elif f == "d":
            data = cs.draw(codes[p][0], mode, n, seed + 40 + p)
            planes.append(Plane("d", data, main=Stream(codes[p][0], data)))
        else:
            planes.append(Plane("w", hf.words(seed + 40 + p, -(-n // 8)).view(np.uint8)[:n].copy()))
    base = hf.words(SEED_FORMS_BASE + 4096 * e + k, -(-n * e // 8)).view(np.uint8)[: n * e].copy()
    row_elems, firsts = rows_for(n, SEED_FORMS_ROWS + 4096 * e + k, ROW_ELEMS_MAX, True)
    return Case(e, k, n, planes, base, ranges_for(n, SEED_FORMS_RANGE + 4096 * e + k), row_elems, firsts)


@functools.lru_cache(maxsize=None)
def _cases():
    choose = _Chooser()  # the cycles run on from width to width
    return {e: [_case(e, k, choose) for k in range(FORMS_CASES)] for e in WIDTHS}


def cases(e):
    return _cases()[e]


@functools.lru_cache(maxsize=None)
def typed_rows(e):
    """the rows ghf_decode_planes_gather is asked for on code_sweep.typed_cases(e): (tensor, raw mask, row_elems, firsts); in
    every third case plane k % e is passed raw, as its own bytes"""
    out = []
    for k, t in enumerate(cs.typed_cases(e)):
        row_elems, firsts = rows_for(t.n, SEED_TYPED_ROWS + 4096 * e + k, TYPED_ROW_ELEMS_MAX, False)
        out.append((t, 1 << (k % e) if k % 3 == 2 else 0, row_elems, firsts))
    return out


# ---------------------------------------------------------------- what is covered, and the digest
def coverage():
    """role x max_len over the three widths together, role x decoder class per width, and what else the CPU test pins"""
    by_len = {r: [0] * 33 for r in ROLES}
    by_class = {r: {e: [0] * 6 for e in WIDTHS} for r in ROLES}
    forms = {e: {} for e in WIDTHS}
    ragged = 0
    for e in WIDTHS:
        for c in cases(e):
            ragged += c.n % 8 != 0
            for p in c.planes:
                forms[e][p.form] = forms[e].get(p.form, 0) + 1
                for role, s in (("dense", p.main if p.kind == "dense" else None), ("mask", p.main if p.kind == "sparse" else None),
                                ("values", p.values)):
                    if s is not None:
                        by_len[role][s.entry.max_len] += 1
                        by_class[role][e][s.entry.variant] += 1
    return {"max_len": {r: by_len[r][1:] for r in ROLES}, "classes": {r: {str(e): by_class[r][e] for e in WIDTHS} for r in ROLES},
            "forms": {str(e): dict(sorted(forms[e].items())) for e in WIDTHS}, "ragged": ragged,
            "largest_n": max(c.n for e in WIDTHS for c in cases(e))}


def sha256():
    m = hashlib.sha256()
    for e in WIDTHS:
        for c in cases(e):
            m.update(repr(c).encode())
            m.update(c.tensor.tobytes())
            m.update(c.base.tobytes())
            for p in c.planes:
                if p.kind == "sparse":
                    m.update(p.mask.tobytes())
                    m.update(p.vals.tobytes())
            m.update(np.asarray(c.ranges, dtype="<i8").tobytes())
            m.update(np.asarray([c.row_elems] + c.firsts, dtype="<i8").tobytes())
        for t, raw, row_elems, firsts in typed_rows(e):
            m.update(t.name.encode())
            m.update(np.asarray([raw, row_elems] + firsts, dtype="<i8").tobytes())
    return m.hexdigest()
