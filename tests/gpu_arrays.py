"""Arrays in HBM for the edge tests of the product kernels (tests/test_formats_edges_gpu.py, tests/test_bsr_edges_gpu.py): inputs a chosen number of
elements behind an aligned address, and an output that is longer than a launch may write and prefilled with a NaN that no product can produce
(format_cases.SENTINEL_BITS), compared on the 64 bits of every element."""
import numpy as np

import format_cases as fc
from lis_amd import DeviceArray as DA


def dev(arr, dtype=None, shift=0):
    """the array in HBM, `shift` elements behind an allocation's (256 B aligned) start: (owner, address)"""
    arr = np.ascontiguousarray(arr, dtype)
    host = np.zeros(arr.size + shift, arr.dtype)
    host[shift:] = arr.ravel()
    d = DA.from_host(host) if host.size else DA(0, arr.dtype)
    return d, d.ptr + shift * arr.dtype.itemsize


class Out:
    """y in HBM: n elements `shift` elements behind an aligned address, Y_PAD more behind them, the sentinel everywhere"""

    def __init__(self, n, shift=0):
        self.n, self.shift = n, shift
        self.d = DA(shift + n + fc.Y_PAD, np.float64)
        self.ptr = self.d.ptr + 8 * shift
        self.reset()

    def reset(self):
        self.d.upload(fc.sentinel(self.d.count))

    def bits(self):
        return self.d.to_host().view(np.uint64)

    def holds(self, ref, what, rb=0, re=None, special=False):
        """rows [rb, re) hold ref's bits, everything else the sentinel.  special: where ref is NaN any NaN but the sentinel will do (a NaN's
        sign and payload are the hardware's), every other element bit for bit"""
        re = len(ref) if re is None else re
        want = fc.bits(fc.sentinel(self.d.count)).copy()
        want[self.shift + rb:self.shift + re] = fc.bits(ref[rb:re])
        got = self.bits()
        if special:
            nan = np.zeros(self.d.count, bool)
            nan[self.shift + rb:self.shift + re] = np.isnan(ref[rb:re])
            assert np.all(np.isnan(got.view(np.float64)[nan]) & (got[nan] != fc.SENTINEL_BITS)), what
            got, want = got[~nan], want[~nan]
        bad = np.flatnonzero(got != want)
        assert not len(bad), (what, "elements", bad[:8].tolist(), [hex(v) for v in got[bad[:4]]], [hex(v) for v in want[bad[:4]]])
