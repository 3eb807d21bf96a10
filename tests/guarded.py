"""The guarded device arena of the sweep modules (tests/test_gpu_code_sweep.py, tests/test_gpu_crs_sweep.py): every output
of a case sits between guard bytes in one device buffer, one copy brings everything back."""
import numpy as np

GUARD = 0xA5
PAD = 64


def first_diff(got, want):
    if got.size != want.size:
        return "sizes %d / %d" % (got.size, want.size)
    d = np.flatnonzero(got != want)
    return "equal" if d.size == 0 else "first difference at byte %d of %d" % (int(d[0]), got.size)


class Arena:
    """one device buffer of GUARD bytes with the outputs of a case in it: region k starts `skew` bytes behind a 16-byte
    boundary and has at least PAD guard bytes on either side; one copy brings everything back"""

    def __init__(self):
        self.at, self.regions = PAD, []

    def add(self, nbytes, skew=0):
        off = self.at + skew
        self.regions.append((off, int(nbytes)))
        self.at = (off + int(nbytes) + 15 & ~15) + PAD
        return len(self.regions) - 1

    def alloc(self, torch):
        self.d = torch.full((self.at,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.d.data_ptr() % 16 == 0
        return self

    def view(self, k):
        off, n = self.regions[k]
        return self.d[off : off + n]

    def fetch(self):
        """-> whether every byte outside the regions is still GUARD"""
        self.h = self.d.cpu().numpy()
        outside = np.ones(self.h.size, dtype=bool)
        for off, n in self.regions:
            outside[off : off + n] = False
        return bool(np.all(self.h[outside] == GUARD))

    def got(self, k, n=None):
        off, size = self.regions[k]
        return self.h[off : off + (size if n is None else n)]
