"""The K x K statistics and row-transform kernels against plain references, K = 1 .. 128.

One kernel per call, through HipPhases (column_sums, centered_gram, apply) and pbh_affine_rows:

    column sums     k_colsum + k_means
    centered Gram   k_gram_mfma (K <= 32), k_gram + k_gram_reduce over 3 / 6 / 10 tile pairs above
    step 3          k_transform_matrix + k_apply_mfma / k_apply_mfma_w2 (K <= 32), k_apply<64|128>
    affine rows     k_affine<8|32|128>

The (K, N) device block is a view into a wider buffer filled with a sentinel, so that the
column stride `ld` and the base address are chosen by the test: `dense` (ld = N, 16-byte
base), `padded` (ld = N + 1, 16-byte base) and `offset8` (ld even, base 8 bytes past a 16-byte
boundary).  Even ld on a 16-byte base takes the paired 16-byte accesses of k_gram_mfma and
k_apply_mfma_w2, everything else their one-row forms.

(a) Exact tests: integer-valued data, for which every summation order is exact in float64, so
    the kernels must reproduce int64 arithmetic bit for bit (assert_array_equal).
(b) Rounded tests: random float64 data against np.longdouble (80-bit) references.
    Column sums:  |dev - ref| <= n 2^-53 sum|x|, the worst case of any summation order.
    Gram:         |dev - ref| <= (n + 3) 2^-53 sum_r |(x_i - m_i)(x_j - m_j)|: two roundings of
                  the centered factors, one of the product, n of the additions.
    Step 3 and the affine rows have no a-priori bound that is tight (it carries the condition
    of L).  Their yardstick is measured: the deviation of the float64 numpy / scipy
    formulation (oracle/ic.py's solve_triangular + matmul; offset + ((X - shift) / scale) @ M)
    from the longdouble result, as the largest element error over the column's max |value|,
    maximised over the cases of a K class (the kernel that serves them).  The kernel is allowed
    8 x the yardstick: the MFMA path forms M = L^-T P^T first, the same O(k 2^-53 cond) order
    with another constant.

Values seen on an MI355X (yardstick; largest kernel deviation; the limit is 8 x the yardstick):
    step 3   K <= 32  (MFMA)           7.8e-16   1.4e-15
             K <= 64  (k_apply<64>)    1.1e-15   2.1e-15
             K <= 128 (k_apply<128>)   4.7e-15   6.3e-15   (both at (128, 129): cond(L) = 1.6e3)
    affine   K <= 8                    1.4e-16   1.6e-16
             K <= 32                   3.4e-16   3.4e-16
             K <= 128                  4.6e-16   4.6e-16
"""

import ctypes
import functools

import numpy as np
import pytest

from conftest import record

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = -777.25
TAIL = 64  # sentinel elements past the last column

KS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128]
K_ALL_N = [9, 32, 33, 65, 128]
LAYOUTS = ["dense", "padded", "offset8"]


def _ns(k):
    return sorted({k + 1, 127, 128, 129, 4096, 4097, 8191})


def _cases():
    """Every K at N in {129, 4097} with the three layouts; every N at K in K_ALL_N dense, and
    `padded` at the even N = 128, 4096 (the only cases with an odd ld and an even N)."""
    out = [(k, n, lay) for k in KS for n in (129, 4097) for lay in LAYOUTS]
    for k in K_ALL_N:
        out += [(k, n, "dense") for n in _ns(k) if n not in (129, 4097)]
        out += [(k, n, "padded") for n in (128, 4096)]
    return out


CASES = _cases()
APPLY_CASES = [(k, n, lay) for k, n, lay in CASES if k >= 2 and n > k]  # corrcoef must be positive definite
AFFINE_KS = [1, 8, 9, 32, 33, 128]
ORDERS = ["cols", "rows"]  # (rs, cs) = (1, ld) as the product calls it; (k, 1): a row-major (N, K) array


def _id(case):
    return "-".join(str(c) for c in case)


def apply_class(k):
    return "K<=32 mfma" if k <= 32 else "K<=64 k_apply<64>" if k <= 64 else "K<=128 k_apply<128>"


def affine_class(k):
    return "K<=8" if k <= 8 else "K<=32" if k <= 32 else "K<=128"


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------- references (host)
def gram_upper(A):
    """A A^T of a (k, n) matrix in its own dtype (longdouble or int64) from dot products of
    contiguous rows; the upper triangle is computed in row blocks and mirrored (the products
    commute exactly)."""
    k = A.shape[0]
    G = np.empty((k, k), dtype=A.dtype)
    for i in range(0, k, 16):
        G[i:i + 16, i:] = np.einsum("in,jn->ij", A[i:i + 16], A[i:])
    iu = np.triu_indices(k, 1)
    G.T[iu] = G[iu]
    return G


def tri_apply(S, L, P):
    """CS = P L^-1 S for a (k, n) block S: forward substitution with the rows of L (the
    triangular solve), then the product with the lower triangular P, in the dtype of S:
    longdouble, or int64 with a unit diagonal in L."""
    k = S.shape[0]
    D = np.empty_like(S)
    for j in range(k):
        D[j] = S[j] - np.einsum("m,mn->n", L[j, :j], D[:j])
        if S.dtype == LD:  # the integer L has a unit diagonal
            D[j] /= L[j, j]
    return np.stack([np.einsum("m,mn->n", P[j, :j + 1], D[:j + 1]) for j in range(k)])


@functools.lru_cache(maxsize=2)
def int_gram_ref(k, n):
    rng = np.random.default_rng([1, k, n])
    S = rng.integers(-8, 9, size=(k, n))
    m = rng.integers(-3, 4, size=k)
    D = S - m[:, None]
    G = gram_upper(D)
    return _ro(S.astype(np.float64), m.astype(np.float64), G)


def int_factors(k, seed):
    """L unit lower triangular with entries in {-1, 0, 1}, P lower triangular with entries in
    {0, 1, 2} and a positive diagonal.  The strict lower part N of L joins three index classes
    (entry (i, j) only where class(i) > class(j)), so N^3 = 0 and L^-1 = I - N + N^2 has entries
    of at most k: no intermediate of either formulation comes near 2^53."""
    rng = np.random.default_rng([2, k, seed])
    cls = rng.integers(0, 3, size=k)
    L = np.tril(rng.integers(-1, 2, size=(k, k)), -1) * (cls[:, None] > cls[None, :]) + np.eye(k, dtype=np.int64)
    P = np.tril(rng.integers(0, 3, size=(k, k)), -1) + np.diag(rng.integers(1, 3, size=k))
    return L.astype(np.int64), P.astype(np.int64)


@functools.lru_cache(maxsize=2)
def int_apply_ref(k, n):
    rng = np.random.default_rng([3, k, n])
    S = rng.integers(-4, 5, size=(k, n))
    L, P = int_factors(k, n)
    CS = tri_apply(S, L, P)
    # every intermediate of substitution-then-multiply and of (L^-T P^T)-then-multiply is bounded
    # by the same computation on a row of the largest |S| with the comparison matrix 2 I - |L|
    bound = tri_apply(np.full((k, 1), 4, dtype=np.int64), 2 * np.eye(k, dtype=np.int64) - np.abs(L), np.abs(P))
    assert 0 < int(bound.max()) < 2 ** 53 and int(np.abs(CS).max()) <= int(bound.max())
    return _ro(S.astype(np.float64), L.astype(np.float64), P.astype(np.float64), CS)


def spread_block(k, n, offset):
    """Columns with offsets offset * c (offset * (c + 1) when ill-conditioned: 1e6) plus a unit
    gamma spread."""
    rng = np.random.default_rng([4, k, n])
    x = rng.gamma(2.0, 1.0, size=(k, n))
    return x + (offset * np.arange(k) if offset < 1e6 else offset * (np.arange(k) + 1.0))[:, None]


@functools.lru_cache(maxsize=2)
def sums_ref(k, n, offset=10.0):
    """x, its longdouble column sums and sum|x|."""
    x = spread_block(k, n, offset)
    xl = x.astype(LD)
    return _ro(x, xl.sum(axis=1), np.abs(xl).sum(axis=1))


@functools.lru_cache(maxsize=2)
def gram_ref(k, n, offset=10.0):
    """x, the float64 means the kernel is given, the longdouble centered Gram and its sum|.|."""
    x, sums, _ = sums_ref(k, n, offset)
    means = (sums / n).astype(np.float64)
    A = x.astype(LD) - means.astype(LD)[:, None]
    return _ro(x, means, gram_upper(A), gram_upper(np.abs(A)))


def apply_inputs(k, n):
    from oracle.pipeline import cfg3_corr

    S = np.random.default_rng([5, k, n]).normal(size=(k, n))
    L = np.linalg.cholesky(np.corrcoef(S))
    P = np.linalg.cholesky(cfg3_corr(k))
    return S, L, P


def column_deviation(got, ref):
    """Largest element error over the column's max |ref|, (k, n) layout, in longdouble."""
    err = np.abs(got.astype(LD) - ref).max(axis=1)
    return float((err / np.abs(ref).max(axis=1)).max())


def affine_inputs(k, n):
    rng = np.random.default_rng([6, k, n])
    X = spread_block(k, n, 10.0)
    shift = X.mean(axis=1)
    scale = X.std(axis=1)
    M = rng.normal(size=(k, k)) / np.sqrt(k)
    return X, shift, scale, shift.copy(), M


def affine_numpy(X, shift, scale, offset, M):
    """(k, n) in, (k, n) out: offset + ((X - shift) / scale) @ M on the (n, k) array."""
    Xt = np.ascontiguousarray(X.T)
    return np.ascontiguousarray((offset + ((Xt - shift) / scale) @ M).T)


AFFINE_ROUNDED = [(k, 129) for k in KS] + [(k, 4097) for k in AFFINE_KS]


@pytest.fixture(scope="module")
def longdouble80():
    if not np.finfo(LD).eps < 2e-19:
        pytest.skip("np.longdouble is not the 80-bit extended type here")


@pytest.fixture(scope="module")
def apply_refs(longdouble80):
    """{(k, n): (S, L, P, longdouble CS)} and the yardstick per K class: the float64 oracle
    formulation's own deviation from the longdouble result."""
    import scipy.linalg

    refs, yard = {}, {}
    for k, n in sorted({(k, n) for k, n, _ in APPLY_CASES}):
        S, L, P = apply_inputs(k, n)
        ref = tri_apply(S.astype(LD), L.astype(LD), P.astype(LD))
        St = np.ascontiguousarray(S.T)
        oracle = scipy.linalg.solve_triangular(L, St.T, lower=True).T @ P.T  # oracle/ic.py: steps 3a, 3b
        dev = column_deviation(np.ascontiguousarray(oracle.T), ref)
        yard[apply_class(k)] = max(yard.get(apply_class(k), 0.0), dev)
        refs[(k, n)] = _ro(S, L, P, ref)
    record("kstats_yardsticks_apply", yard)
    yield refs, yard
    refs.clear()


@pytest.fixture(scope="module")
def affine_refs(longdouble80):
    refs, yard = {}, {}
    for k, n in AFFINE_ROUNDED:
        X, shift, scale, offset, M = affine_inputs(k, n)
        Xt = np.ascontiguousarray(X.T).astype(LD)
        V = (Xt - shift.astype(LD)) / scale.astype(LD)
        Ml = M.astype(LD)
        ref = np.ascontiguousarray(np.stack([V @ Ml[:, j] for j in range(k)]) + offset.astype(LD)[:, None])
        dev = column_deviation(affine_numpy(X, shift, scale, offset, M), ref)
        yard[affine_class(k)] = max(yard.get(affine_class(k), 0.0), dev)
        refs[(k, n)] = (X, shift, scale, offset, M, ref)
    record("kstats_yardsticks_affine", yard)
    yield refs, yard
    refs.clear()


SEEN = {}  # largest kernel deviation per (kind, K class), recorded by the last test


def _seen(kind, cls, dev):
    SEEN[f"{kind} {cls}"] = max(SEEN.get(f"{kind} {cls}", 0.0), dev)


# ---------------------------------------------------------------------------- device blocks
class Block:
    """A (k, n) float64 view with a chosen column stride and base alignment inside a buffer of
    sentinels."""

    def __init__(self, k, n, layout):
        import torch

        from probabilit_amd import device

        self.k, self.n = k, n
        self.lead = 1 if layout == "offset8" else 0
        self.ld = {"dense": n, "padded": n + 1, "offset8": n + (n & 1)}[layout]
        self.buf = torch.full((self.lead + k * self.ld + TAIL,), SENTINEL, dtype=torch.float64,
                              device=device.device())
        self.view = self.buf[self.lead:self.lead + k * self.ld].view(k, self.ld)[:, :n]
        assert self.buf.data_ptr() % 16 == 0
        assert self.view.data_ptr() % 16 == (8 if layout == "offset8" else 0)
        assert self.view.stride(0) == self.ld and self.view.stride(1) == 1
        assert self.view.stride(0) % 2 == {"dense": n % 2, "padded": (n + 1) % 2, "offset8": 0}[layout]

    def load(self, host):
        import torch

        self.view.copy_(torch.from_numpy(np.array(host, dtype=np.float64)))  # a writable copy
        return self.view

    def whole(self):
        return self.buf.cpu().numpy()

    def outside(self):
        """The buffer's elements that do not belong to the view."""
        keep = np.ones(self.lead + self.k * self.ld + TAIL, dtype=bool)
        keep[self.lead:self.lead + self.k * self.ld].reshape(self.k, self.ld)[:, :self.n] = False
        return self.whole()[keep]

    def expected_whole(self, host):
        """The buffer's content if exactly the view holds `host` and nothing else was written."""
        e = np.full(self.lead + self.k * self.ld + TAIL, SENTINEL)
        e[self.lead:self.lead + self.k * self.ld].reshape(self.k, self.ld)[:, :self.n] = host
        return e


@pytest.fixture(scope="module")
def ph(gpu):
    from probabilit_amd.distributed import HipPhases

    return HipPhases()


def _dev(a):
    from probabilit_amd import device

    return device.to_device(np.array(a, dtype=np.float64))  # a writable copy


def _host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------- (a) exact
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_spike_gram_and_sums(ph, case):
    """One non-zero row r, S[c, r] = c + 1, zero means: Gram = outer(1..k, 1..k) and the column
    sums 1..k, whichever row it is (a dropped or duplicated row, swapped columns or a wrong tile
    pair changes an entry)."""
    k, n, layout = case
    b = Block(k, n, layout)
    S = b.view
    S.zero_()
    ramp = np.arange(1.0, k + 1)
    col, zero = _dev(ramp), _dev(np.zeros(k))
    for r in sorted({0, 1, 63, 64, 127, 128, n - 2, n - 1} & set(range(n))):
        S[:, r] = col
        sums, gram = _host(ph.column_sums(S)), _host(ph.centered_gram(S, zero))
        S[:, r] = 0.0
        np.testing.assert_array_equal(sums, ramp, err_msg=f"column sums, spike at row {r}")
        np.testing.assert_array_equal(gram, np.outer(ramp, ramp), err_msg=f"Gram, spike at row {r}")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_integer_gram(ph, case):
    """Integers in [-8, 8] and integer `means` in [-3, 3] that are not the true means (the kernel
    must use what it is given): (S - m)(S - m)^T exactly, and exactly symmetric."""
    k, n, layout = case
    S, m, G = int_gram_ref(k, n)
    gram = _host(ph.centered_gram(Block(k, n, layout).load(S), _dev(m)))
    np.testing.assert_array_equal(gram, gram.T)
    np.testing.assert_array_equal(gram, G.astype(np.float64))
    np.testing.assert_array_equal(_host(ph.column_sums(Block(k, n, layout).load(S))), S.sum(axis=1))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_identity_apply(ph, case):
    """L = P = I leaves random float64 scores bit-identical and writes nothing outside the view."""
    k, n, layout = case
    S = np.random.default_rng([7, k, n]).normal(size=(k, n))
    b = Block(k, n, layout)
    ph.apply(b.load(S), np.eye(k), np.eye(k))
    np.testing.assert_array_equal(b.whole(), b.expected_whole(S))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_integer_apply(ph, case):
    """Integer L (unit lower triangular), P (lower triangular) and S: P L^-1 S exactly."""
    k, n, layout = case
    S, L, P, CS = int_apply_ref(k, n)
    b = Block(k, n, layout)
    ph.apply(b.load(S), L, P)
    np.testing.assert_array_equal(b.whole(), b.expected_whole(CS.astype(np.float64)))


def _affine(X, n, k, x_rs, x_cs, shift, scale, offset, M, Y, y_rs, y_cs):
    from probabilit_amd import _lib, device

    lib = _lib.load()
    nb = ctypes.c_size_t()
    _lib.check(lib.pbh_affine_workspace_size(k, ctypes.byref(nb)))
    ws = device.empty(int(nb.value), "uint8")
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (shift, scale, offset, M)]
    _lib.check(lib.pbh_affine_rows(X.data_ptr(), n, k, x_rs, x_cs, *[_lib.np_ptr(a) for a in arrs], Y.data_ptr(),
                                   y_rs, y_cs, ws.data_ptr(), nb.value, device.stream()), "pbh_affine_rows")


class Rows:
    """The (k, n) values as a row-major (N, K) array inside a buffer of sentinels: element
    (r, c) at r * k + c."""

    def __init__(self, k, n):
        import torch

        from probabilit_amd import device

        self.k, self.n = k, n
        self.buf = torch.full((n * k + TAIL,), SENTINEL, dtype=torch.float64, device=device.device())
        self.view = self.buf[:n * k].view(n, k)
        self.rs, self.cs = k, 1

    def load(self, host):
        import torch

        self.view.copy_(torch.from_numpy(np.array(host.T, dtype=np.float64, order="C")))
        return self.view

    def whole(self):
        return self.buf.cpu().numpy()

    def expected_whole(self, host):
        e = np.full(self.n * self.k + TAIL, SENTINEL)
        e[:self.n * self.k].reshape(self.n, self.k)[:] = host.T
        return e


def _holder(order, k, n):
    if order == "rows":
        return Rows(k, n)
    b = Block(k, n, "padded")
    b.rs, b.cs = 1, b.ld
    return b


@pytest.mark.parametrize("y_order", ORDERS)
@pytest.mark.parametrize("x_order", ORDERS)
@pytest.mark.parametrize("n", [129, 4097])
@pytest.mark.parametrize("k", AFFINE_KS)
def test_integer_affine(gpu, k, n, x_order, y_order):
    """Integer shift / offset / M and power-of-two scales: offset + ((X - shift) / scale) @ M
    exactly, with X and Y each column-major (1, ld) or row-major (k, 1)."""
    rng = np.random.default_rng([8, k, n])
    scale = 2.0 ** rng.integers(-2, 3, size=k)
    shift = rng.integers(-5, 6, size=k)
    X = shift[:, None] + rng.integers(-6, 7, size=(k, n)) * scale[:, None]  # (X - shift) / scale: integers
    offset = rng.integers(-9, 10, size=k)
    M = rng.integers(-3, 4, size=(k, k))
    V = np.rint((X - shift[:, None]) / scale[:, None]).astype(np.int64)
    ref = (offset[:, None] + M.T.astype(np.int64) @ V).astype(np.float64)
    x, y = _holder(x_order, k, n), _holder(y_order, k, n)
    x.load(X)
    _affine(x.view, n, k, x.rs, x.cs, shift, scale, offset, M, y.view, y.rs, y.cs)
    np.testing.assert_array_equal(y.whole(), y.expected_whole(ref))
    np.testing.assert_array_equal(x.whole(), x.expected_whole(X))


# ---------------------------------------------------------------------------- (b) rounded
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_column_sums_rounded(ph, longdouble80, case):
    k, n, layout = case
    x, sums, abs_sums = sums_ref(k, n)
    got = _host(ph.column_sums(Block(k, n, layout).load(x)))
    err = np.abs(got.astype(LD) - sums)
    bound = n * U * abs_sums
    assert (err <= bound).all(), f"column sums: worst error / bound {float((err / bound).max()):.3g}"


def _check_gram(ph, k, n, layout, offset):
    x, means, G, Gabs = gram_ref(k, n, offset)
    got = _host(ph.centered_gram(Block(k, n, layout).load(x), _dev(means)))
    np.testing.assert_array_equal(got, got.T)
    err = np.abs(got.astype(LD) - G)
    bound = (n + 3) * U * Gabs
    assert (err <= bound).all(), f"Gram: worst error / bound {float((err / bound).max()):.3g}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_centered_gram_rounded(ph, longdouble80, case):
    k, n, layout = case
    _check_gram(ph, k, n, layout, 10.0)


@pytest.mark.parametrize("layout", ["dense", "padded"])
@pytest.mark.parametrize("k", [8, 33])
def test_centered_gram_ill_conditioned(ph, longdouble80, k, layout):
    """Offsets 1e6 (c + 1) with unit spread: the case where centering matters."""
    _check_gram(ph, k, 4097, layout, 1e6)


@pytest.mark.parametrize("case", APPLY_CASES, ids=_id)
def test_apply_rounded(ph, apply_refs, case):
    k, n, layout = case
    refs, yard = apply_refs
    S, L, P, ref = refs[(k, n)]
    b = Block(k, n, layout)
    ph.apply(b.load(S), L, P)
    dev = column_deviation(_host(b.view), ref)
    _seen("apply", apply_class(k), dev)
    limit = 8 * yard[apply_class(k)]
    print(f"apply {case}: deviation {dev:.3g}, limit {limit:.3g}")
    assert dev <= limit, f"step 3 deviates {dev:.3g} from the longdouble result, limit {limit:.3g}"
    np.testing.assert_array_equal(b.outside(), SENTINEL)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kn", AFFINE_ROUNDED, ids=_id)
def test_affine_rounded(gpu, affine_refs, kn, order):
    k, n = kn
    refs, yard = affine_refs
    X, shift, scale, offset, M, ref = refs[kn]
    x, y = _holder(order, k, n), _holder(order, k, n)
    x.load(X)
    _affine(x.view, n, k, x.rs, x.cs, shift, scale, offset, M, y.view, y.rs, y.cs)
    got = _host(y.view)
    dev = column_deviation(got if order == "cols" else np.ascontiguousarray(got.T), ref)
    _seen("affine", affine_class(k), dev)
    limit = 8 * yard[affine_class(k)]
    print(f"affine {kn} {order}: deviation {dev:.3g}, limit {limit:.3g}")
    assert dev <= limit, f"affine rows deviate {dev:.3g} from the longdouble result, limit {limit:.3g}"


def test_record_kernel_deviations(gpu):
    """Keeps the largest step-3 / affine deviations per K class seen by the tests above."""
    record("kstats_kernel_deviations", SEEN)
