"""Guarded device buffers of the GPU tests: a vector, or a slab of rows, inside one allocation of the test's own whose every other
byte holds a fill pattern.  A kernel that writes outside its output changes the pattern (the guards of
tests/test_gpu_accuracy_contracts.py and tests/test_gpu_two_pass.py, fill 0xA5); a kernel that READS outside its input meets the
pattern — with a fill that is NaN (0xFF) or huge (0x7F) in every storage type the read reaches the result
(tests/test_gpu_poisoned_reads.py).  GUARD elements lie on either side, so an over-read of one lane's 64 bytes stays inside the
allocation.  No test."""
import types

import numpy as np

GUARD = 64


def pattern(count, dtype, fill):
    """`count` elements of dtype whose every byte is `fill`."""
    dtype = np.dtype(dtype)
    return np.frombuffer(np.full(count * dtype.itemsize, fill, dtype=np.uint8).tobytes(), dtype=dtype).copy()


def guarded(ctx, host, shift, fill=0xA5):
    """Device buffer of GUARD + shift + n + GUARD elements filled with a byte pattern, `host` written at element GUARD + shift;
    returns (buffer, view at that element)."""
    host = np.ascontiguousarray(host)
    n = host.shape[0]
    total = GUARD + shift + n + GUARD
    buf = ctx.empty(total, host.dtype)
    image = pattern(total, host.dtype, fill)
    image[GUARD + shift: GUARD + shift + n] = host
    buf.set(image)
    view = types.SimpleNamespace(ptr=buf.ptr + (GUARD + shift) * host.dtype.itemsize, dtype=host.dtype, shape=(n,))
    return buf, view


def unguard(buf, n, shift, fill=0xA5):
    """The n elements of the view, after asserting that every byte outside them still holds the pattern."""
    raw = buf.get()
    b = raw.view(np.uint8)
    isz = raw.dtype.itemsize
    lo, hi = (GUARD + shift) * isz, (GUARD + shift + n) * isz
    assert np.all(b[:lo] == fill) and np.all(b[hi:] == fill), "a kernel wrote outside its vector"
    return raw[GUARD + shift: GUARD + shift + n]


class GuardedSlab:
    """nb_alloc >= nb rows of ld >= n elements inside one guarded allocation, the first row at element GUARD + shift.  The data are
    the first n elements of the first nb rows; the row gaps [n, ld), the rows nb .. nb_alloc - 1 and both guards are the
    surroundings.  refill() writes surroundings and data anew at the same device addresses; rows() returns the data after
    asserting that the surroundings still hold the fill.  (nb = nb_alloc = 1, ld = n: a guarded vector.)"""

    def __init__(self, ctx, dtype, n, nb=1, ld=None, nb_alloc=None, shift=0):
        self.dtype = np.dtype(dtype)
        self.n, self.nb, self.shift = int(n), int(nb), int(shift)
        self.ld = self.n if ld is None else int(ld)
        self.nb_alloc = self.nb if nb_alloc is None else int(nb_alloc)
        assert self.ld >= self.n and self.nb_alloc >= self.nb
        self.first = GUARD + self.shift
        self.total = self.first + self.nb_alloc * self.ld + GUARD
        self.buf = ctx.empty(self.total, self.dtype)
        self.ptr = self.buf.ptr + self.first * self.dtype.itemsize
        self.shape = (self.n,) if self.nb_alloc == 1 else (self.nb_alloc, self.ld)
        self._data = np.zeros(self.total, dtype=bool)   # which elements of the allocation are data
        block = self._data[self.first: self.first + self.nb_alloc * self.ld].reshape(self.nb_alloc, self.ld)
        block[: self.nb, : self.n] = True

    def refill(self, fill, rows=None):
        """Every byte of the allocation := fill, then `rows` ((nb, n) or (n,)) into the data elements.  rows = None: a pure output,
        whose previous contents are the fill too."""
        image = pattern(self.total, self.dtype, fill)
        if rows is not None:
            image[self._data] = np.ascontiguousarray(rows, dtype=self.dtype).reshape(self.nb * self.n)
        self.buf.set(image)
        return self

    def rows(self, fill, what="a kernel wrote outside its output"):
        """The data as an (nb, n) array ((n,) for a vector), after asserting that every byte outside them holds the fill."""
        raw = self.buf.get()
        outside = raw[~self._data].view(np.uint8)
        assert np.all(outside == fill), what
        got = raw[self._data]
        return got if self.nb_alloc == 1 else got.reshape(self.nb, self.n)

    def free(self):
        self.buf.free()
