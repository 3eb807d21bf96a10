"""What ghf_compress_planes_forms must store, from numpy and oracle.compress alone: the choice rule
restated, and the expected content of every slot.  Shared by tests/test_planes_forms_cpu.py and tests/test_gpu_planes_forms.py.

A plane is a byte string.  Its DENSE form is oracle.compress(plane), its SPARSE form the two strings of DESIGN.md section 20
(mask = packbits(plane != 0) LSB first, values = plane[plane != 0]), each compressed by itself, its RAW form the plane."""
import numpy as np

from oracle import oracle as orc

AUTO = 0x80000000
TWO_HEADERS = 2 * (1040 + 8 * 1)  # 2 * ghf_header_bytes(1): what a sparse plane stores before its first payload bit


def normal_elems(n, e, seed=7):
    """n seeded standard-normal values as bytes: bf16 (the upper half of the fp32 value) / fp32 / fp64"""
    x = np.random.default_rng(seed).standard_normal(n)
    if e == 8:
        return x.view(np.uint8).copy()
    f = x.astype(np.float32)
    if e == 4:
        return f.view(np.uint8).copy()
    return (f.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8).copy()


def planes_of(a, e):
    return [np.ascontiguousarray(a[p::e]) for p in range(e)]


def sparse_form(x):
    nz = x != 0
    return np.packbits(nz, bitorder="little"), np.ascontiguousarray(x[nz])


_images = {}


def image(s):
    """oracle.compress of a byte string, once per distinct string"""
    key = (s.size, s.tobytes())
    if key not in _images:
        _images[key] = orc.compress(s)
    return _images[key]


def choose(planes, raw, sparse):
    """the masks the call reports for a request (raw, sparse), each a bit mask or AUTO"""
    n = planes[0].size
    raw_chosen = 0 if raw == AUTO else raw
    sparse_chosen = 0 if sparse == AUTO else sparse
    sparse_pays = raw != AUTO or n > TWO_HEADERS
    for p, pl in enumerate(planes):
        zeros = n - int(np.count_nonzero(pl))
        if sparse == AUTO and not (raw_chosen >> p) & 1 and sparse_pays and zeros >= n - n // 4:
            sparse_chosen |= 1 << p
        if raw == AUTO and not (sparse_chosen >> p) & 1 and image(pl).size >= n:
            raw_chosen |= 1 << p
    return raw_chosen, sparse_chosen


class Stored:
    """the expected slots of one tensor: kind[j] in ("raw", "image", None), data[j] the bytes slot j begins with, symbols[j]
    what the stream decodes to (None for a raw or empty slot), tables[j] the code as a dict (images only)"""

    def __init__(self, src, e, raw=AUTO, sparse=0, tables=True):
        self.e, self.n = e, src.size // e
        self.planes = planes_of(src, e)
        self.raw, self.sparse = choose(self.planes, raw, sparse)
        assert self.raw & self.sparse == 0
        self.n_vals = [int(np.count_nonzero(pl)) for pl in self.planes]
        self.kind, self.data, self.symbols, self.tables = [None] * (2 * e), [None] * (2 * e), [None] * (2 * e), [None] * (2 * e)
        for p, pl in enumerate(self.planes):
            if (self.raw >> p) & 1:
                self.kind[p], self.data[p] = "raw", pl
            elif (self.sparse >> p) & 1:
                m, v = sparse_form(pl)
                self._image(p, m, tables)
                if v.size:
                    self._image(e + p, v, tables)
            else:
                self._image(p, pl, tables)
        self.sizes = [0 if d is None else int(d.size) for d in self.data]

    def _image(self, j, s, tables):
        self.kind[j], self.data[j], self.symbols[j] = "image", image(s), int(s.size)
        if tables:
            self.tables[j] = orc.build_code(orc.histogram(s)).as_dict()

    @property
    def total(self):
        return sum(self.sizes)
