"""Guarded device windows for the tests of the device-resident entry points (imported like
field_edges.py; no conftest).

A Window is a slice of one DeviceBuffer laid out, in rows of `width` words, as

    GUARD rows of SENTINEL | off rows of SENTINEL (padding) | the payload | GUARD rows of SENTINEL

and has a `.ptr`, so it passes wherever zkalgebra.py takes a DeviceBuffer.  GUARD = 256 rows is one
workgroup's worth: a kernel that overruns its array by a whole wavefront or block still lands inside
the same allocation, where check() turns it into a failed assertion.  off in {0, 1, 3} rows keeps the
payload 32-byte aligned (the 16-byte vector and nontemporal accesses stay legal) but takes it off the
64-, 128- and 256-byte boundaries of the allocation.  A payload that was not uploaded holds the
sentinel too, so a row a kernel should have written and did not is seen as well.
"""
import contextlib

import numpy as np

GUARD = 256
OFFS = (0, 1, 3)
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


class Window:
    def __init__(self, zk, payload, off=0, width=4):
        """payload: an (n, width) uint64 array to upload, or a row count (the rows hold the sentinel)"""
        assert off in OFFS
        if isinstance(payload, (int, np.integer)):
            data, rows = None, int(payload)
        else:
            data = np.ascontiguousarray(payload, dtype=np.uint64).reshape(-1, width)
            rows = data.shape[0]
        self.rows, self.width, self.off = rows, width, off
        self.lo = GUARD + off  # first payload row
        img = np.full((self.lo + rows + GUARD, width), SENTINEL, dtype=np.uint64)
        if data is not None:
            img[self.lo:self.lo + rows] = data
        self.buf = zk.DeviceBuffer(img)
        self._like = img
        self.ptr = self.buf.ptr + self.lo * width * 8

    def _image(self):
        return self.buf.to_host(self._like)

    def read(self):
        """the payload rows as they are on the device now"""
        return self._image()[self.lo:self.lo + self.rows].copy()

    def check(self, what=""):
        """both guards and the padding still hold the sentinel"""
        img = self._image()
        for name, part, first in (("low guard / padding", img[:self.lo], -self.lo),
                                  ("high guard", img[self.lo + self.rows:], self.rows)):
            bad = np.nonzero((part != SENTINEL).any(axis=1))[0]
            assert not len(bad), (f"{what}: {name} overwritten (off {self.off}, {self.rows} rows), "
                                  f"rows relative to the payload: {[first + int(i) for i in bad[:8]]}")

    def untouched(self):
        """the payload still holds the sentinel in every word (nothing was written)"""
        return bool((self.read() == SENTINEL).all())

    def free(self):
        self.buf.free()
        self.ptr = None


class Pool:
    """hands out windows with off cycling over OFFS from `start` (successive windows of one call get
    different offsets), and checks or frees all of them at once"""

    def __init__(self, zk, start=0):
        self.zk, self.k, self.windows = zk, start, []

    def new(self, payload, width=4):
        w = Window(self.zk, payload, OFFS[self.k % len(OFFS)], width)
        self.k += 1
        self.windows.append(w)
        return w

    def check(self, what=""):
        for w in self.windows:
            w.check(what)

    def free(self):
        for w in self.windows:
            w.free()
        self.windows = []


@contextlib.contextmanager
def pool(zk, start=0):
    """with pool(gpu, k) as P: ... -- every window of P is freed on the way out, pass or fail"""
    p = Pool(zk, start)
    try:
        yield p
    finally:
        p.free()
