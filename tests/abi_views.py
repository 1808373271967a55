"""Views inside sentinel-filled device buffers for tests that call one C-ABI entry point directly
(test_gpu_ppf_kernels.py, test_gpu_table_kernel.py, the generator test of test_gpu_qmc.py,
test_gpu_stream_kernels.py, test_gpu_mvar_kernels.py, test_gpu_lhs_decode_kernels.py).

Every input and output of such a call is a strided view at an element offset inside a wider
buffer whose other elements hold one fixed NaN bit pattern; the buffers are compared as int64, so
a write before, after or into the gaps of a view shows, whatever value was written, and a read at
the wrong index (q[i] for q[i * stride], a per-row parameter at i * stride) meets a NaN.
"""

import ctypes

import numpy as np

SENT = 0x7FF8_0BAD_5EED_0001  # a quiet NaN with a payload no computation produces
PAD = 4096  # sentinel elements before and after every view


def _torch():
    import torch

    return torch


def bits(a):
    """The int64 image of a float64 (or int64) host array."""
    a = np.asarray(a)
    if a.dtype != np.int64:
        return np.array(a, dtype=np.float64).view(np.int64)
    return a.copy()


class View:
    """n elements at element offset `off` with stride `stride` inside a sentinel buffer with PAD
    (+ `tail`) sentinels after it.  `values`: a host array or a device tensor (float64 or int64)."""

    def __init__(self, n, off=0, stride=1, values=None, tail=0):
        from probabilit_amd import device

        torch = _torch()
        self.n, self.stride = int(n), int(stride)
        self.span = (self.n - 1) * self.stride + 1 if self.n else 0
        self.lo = PAD + off
        self.buf = torch.full((self.lo + self.span + PAD + tail,), SENT, dtype=torch.int64, device=device.device())
        if values is not None and self.n:
            if isinstance(values, torch.Tensor):
                v = values.to(device.device()).contiguous().view(torch.int64)
            else:
                v = torch.from_numpy(bits(values)).to(device.device())
            assert v.shape == (self.n,), (v.shape, self.n)
            self.dev().copy_(v)
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 8 * self.lo)

    def dev(self):
        """The view itself, as an int64 device tensor."""
        return self.buf[self.lo:self.lo + self.span:self.stride]

    def host(self, dtype=np.float64):
        return self.dev().cpu().numpy().view(dtype)

    def intact(self):
        """Every element outside the view still holds the sentinel."""
        torch = _torch()
        outside = torch.ones(self.buf.shape[0], dtype=torch.bool, device=self.buf.device)
        outside[self.lo:self.lo + self.span:self.stride] = False
        return bool((self.buf[outside] == SENT).all())

    def untouched(self):
        """The whole buffer, the view included, still holds the sentinel."""
        return bool((self.buf == SENT).all())


class Block(View):
    """A column-major output block of ncols columns x nrows rows with a leading dimension of
    nrows + 3, at element offset `off` inside a sentinel buffer, followed by `after` more sentinels
    inside the view (one whole column unless given): what a generator or sampler entry point writes
    through (q, ldq).  Everything is compared on the device, so a block of 10^8 elements costs no
    host copy."""

    def __init__(self, nrows, ncols, off=5, after=None):
        self.nrows, self.ncols, self.ld = int(nrows), int(ncols), int(nrows) + 3
        self.after = self.ld if after is None else int(after)
        super().__init__(self.ncols * self.ld + self.after, off=off)

    def cols(self):
        """The block itself, (ncols, nrows): an int64 device tensor over the buffer."""
        return self.dev()[:self.ncols * self.ld].reshape(self.ncols, self.ld)[:, :self.nrows]

    def rows(self, dtype=np.float64):
        """The block on the host, (nrows, ncols)."""
        return self.cols().cpu().numpy().view(dtype).T

    def assert_clean(self):
        """The three gap rows of every column, the column after the last and everything around the
        block still hold the sentinel."""
        v = self.dev()
        body = v[:self.ncols * self.ld].reshape(self.ncols, self.ld)
        assert bool((body[:, self.nrows:] == SENT).all()), "a gap row was written"
        assert bool((v[self.ncols * self.ld:] == SENT).all()), "the column after the last was written"
        assert self.intact(), "a write outside the block"

    def assert_bits(self, ref, what=""):
        """assert_clean, and the block equals the (nrows, ncols) host array `ref` (float64 or int64)
        bit for bit."""
        torch = _torch()
        self.assert_clean()
        ref = np.asarray(ref)
        assert ref.shape == (self.nrows, self.ncols), (ref.shape, self.nrows, self.ncols)
        want = torch.from_numpy(np.ascontiguousarray(bits(ref).T)).to(self.buf.device)
        self.assert_same(want, what)

    def assert_same(self, want, what=""):
        """The block equals the (ncols, nrows) int64 device tensor `want`."""
        torch = _torch()
        got = self.cols()
        assert tuple(want.shape) == tuple(got.shape), (tuple(want.shape), tuple(got.shape))
        ne = got != want
        if bool(ne.any()):
            c, r = (int(x) for x in torch.nonzero(ne)[0])
            raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at row {r} column {c}: "
                                 f"got {int(got[c, r]):#018x}, want {int(want[c, r]):#018x}")


SENT32 = -0x5EED_0BAD  # no stratum, rank or count is negative


class Block32:
    """Block's int32 sibling: a column-major block of ncols columns x nrows rows of int32 with a
    leading dimension of nrows + 3, at element offset `off` inside a buffer of SENT32, followed by
    `after` more sentinels (one whole column unless given): what an entry point writes through
    (strata, lds)."""

    def __init__(self, nrows, ncols, off=5, after=None):
        from probabilit_amd import device

        torch = _torch()
        self.nrows, self.ncols, self.ld = int(nrows), int(ncols), int(nrows) + 3
        self.after = self.ld if after is None else int(after)
        self.n = self.ncols * self.ld + self.after
        self.lo = PAD + off
        self.buf = torch.full((self.lo + self.n + PAD,), SENT32, dtype=torch.int32, device=device.device())
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * self.lo)

    def dev(self):
        return self.buf[self.lo:self.lo + self.n]

    def cols(self):
        """The block itself, (ncols, nrows): an int32 device tensor over the buffer."""
        return self.dev()[:self.ncols * self.ld].reshape(self.ncols, self.ld)[:, :self.nrows]

    def rows(self):
        """The block on the host, (nrows, ncols)."""
        return self.cols().cpu().numpy().T

    def untouched(self):
        return bool((self.buf == SENT32).all())

    def assert_clean(self):
        v = self.dev()
        body = v[:self.ncols * self.ld].reshape(self.ncols, self.ld)
        assert bool((body[:, self.nrows:] == SENT32).all()), "a gap row was written"
        assert bool((v[self.ncols * self.ld:] == SENT32).all()), "the column after the last was written"
        assert bool((self.buf[:self.lo] == SENT32).all()) and bool((self.buf[self.lo + self.n:] == SENT32).all()), \
            "a write outside the block"

    def assert_equal(self, ref, what=""):
        """assert_clean, and the block equals the (nrows, ncols) host integer array `ref`."""
        torch = _torch()
        self.assert_clean()
        ref = np.asarray(ref)
        assert ref.shape == (self.nrows, self.ncols), (ref.shape, self.nrows, self.ncols)
        want = torch.from_numpy(np.ascontiguousarray(ref.T).astype(np.int32)).to(self.buf.device)
        ne = self.cols() != want
        if bool(ne.any()):
            c, r = (int(x) for x in torch.nonzero(ne)[0])
            raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at row {r} column {c}: "
                                 f"got {int(self.cols()[c, r])}, want {int(want[c, r])}")


class Flag:
    """A device flag word that starts at 0, between two sentinel words."""

    def __init__(self):
        from probabilit_amd import device

        torch = _torch()
        self.buf = torch.tensor([-1, 0, -1], dtype=torch.int32, device=device.device())
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4)

    def value(self):
        h = self.buf.cpu().numpy()
        assert h[0] == -1 and h[2] == -1, "a write next to the flag word"
        return int(h[1])


def tile_to(pattern, n):
    """The first n elements of `pattern` repeated: a device float64 tensor."""
    from probabilit_amd import device

    torch = _torch()
    p = torch.from_numpy(np.array(pattern, dtype=np.float64)).to(device.device())
    return p.repeat(-(-n // p.shape[0]))[:n]


def tiles_equal_first(out_dev, period):
    """out_dev (int64 bits, length n) repeats its first `period` elements, bit for bit."""
    torch = _torch()
    n = out_dev.shape[0]
    first = out_dev[:period]
    k = n // period
    ok = bool((out_dev[:k * period].reshape(k, period) == first).all())
    return ok and bool(torch.equal(out_dev[k * period:], first[:n - k * period]))
