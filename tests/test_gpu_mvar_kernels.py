"""The fused multivariate samplers of csrc/pbh_mvar.hip at the C ABI, at their own launch boundaries:
k_mvn<true / false> (pbh_multivariate_normal), k_dirichlet (pbh_dirichlet), k_multinomial
(pbh_multinomial).

test_gpu_multivariate.py reaches these kernels through native.multivariate, which passes ld = n,
d in {1, 2, 3, 5, 33, 128} and fewer tiles than the grid cap.  Here every call writes a block at an
element offset inside a sentinel buffer with a leading dimension of nrows + 3 (abi_views.Block): the
gap rows, the column after the last and the padding must keep their sentinels.  The values are
checked

  * against scipy on the kernel's own uniforms (native.fill_uniform) under the gates of
    test_gpu_multivariate.py, at the d where the launch changes: the rows per block R (256, 192, 128,
    64) and, for the normal, the factor in LDS (d <= 64; at d = 64 tile + factor fill the 64 KiB
    exactly) or in global memory (d >= 65);
  * bit for bit against shard calls (row0) where the call has more tiles than the grid cap of 8192,
    so that a block strides to a second tile, with a window of the strided rows against scipy;
  * at row0 = 2^32 - 100, where the row counter carries into its high half inside one call.
"""

import numpy as np
import pytest
import scipy.special as sp
import scipy.stats as st

from abi_views import Block, Flag

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
GRID_CAP = 8192  # tile_grid of pbh_mvar.hip: blocks per launch
SAMPLERS = ("multivariate_normal", "dirichlet", "multinomial")


# ---------------------------------------------------------------- parameters and launches
def _mvn_params(d):
    rng = np.random.default_rng(100 + d)
    B = rng.normal(size=(d, d))
    return np.ascontiguousarray(rng.normal(scale=3.0, size=d)), B @ B.T / d + 0.1 * np.eye(d)


def _alpha(d):
    return np.random.default_rng(200 + d).choice([0.5, 1.0, 2.5, 7.0], size=d)


SMALL_P = {2: [0.98, 0.02], 3: [0.2, 0.0, 0.8], 5: [0.005, 0.98, 0.0, 0.01, 0.005]}


def _p(d):
    """probabilities with exact zeros (the first category, one in the middle, the one before the
    last) and one dominant category"""
    if d in SMALL_P:
        return np.array(SMALL_P[d])
    p = np.random.default_rng(300 + d).uniform(0.5, 1.5, size=d)
    p[[0, 1, d // 2, d - 2]] = 0.0
    p *= 0.1 / p.sum()
    p[1] = 0.9
    return p


def _kwargs(name, d, trials=1000):
    if name == "multivariate_normal":
        mean, cov = _mvn_params(d)
        return {"mean": mean, "cov": cov}
    if name == "dirichlet":
        return {"alpha": _alpha(d)}
    return {"n": trials, "p": _p(d)}


def _tables(name, kwargs):
    from probabilit_amd import native

    return native.multivariate_tables(name, getattr(st, name)(**kwargs))[1]


def _call(name, tables, seed, row0, n, d, out_ptr, ld, flag_ptr=None):
    """The entry point itself: its status."""
    from probabilit_amd import _lib, device

    lib = _lib.load()
    if name == "multivariate_normal":
        mean, A = tables
        return lib.pbh_multivariate_normal(seed, row0, n, d, _lib.np_ptr(mean), _lib.np_ptr(A), out_ptr, ld, flag_ptr,
                                           device.stream())
    if name == "dirichlet":
        return lib.pbh_dirichlet(seed, row0, n, d, _lib.np_ptr(tables[0]), out_ptr, ld, flag_ptr, device.stream())
    trials, pc = tables
    return lib.pbh_multinomial(seed, row0, n, d, trials, _lib.np_ptr(pc), out_ptr, ld, flag_ptr, device.stream())


def _block(name, tables, seed, row0, n, flag=None):
    """Rows [row0, row0 + n) into a clean block with ld = n + 3."""
    from probabilit_amd import _lib

    d = len(tables[-1])
    blk = Block(n, d)
    status = _call(name, tables, seed, row0, n, d, blk.ptr, blk.ld, flag.ptr if flag else None)
    assert status == 0, _lib.last_error()
    blk.assert_clean()
    return blk


# ---------------------------------------------------------------- the gates of test_gpu_multivariate.py
def _uniforms(seed, n, d, row0):
    from probabilit_amd import native

    U = native.fill_uniform(seed, n, d, row0=row0)
    return np.where(U == 0.0, 2.0 ** -53, U)


def _multinomial_by_scipy(U, trials, pc):
    """the sampler's sequential rule with scipy.stats.binom.ppf (rem == 0 -> 0)"""
    N, d = U.shape
    rem = np.full(N, float(trials))
    X = np.zeros((N, d), dtype=np.int64)
    for j in range(d - 1):
        k = np.zeros(N)
        live = rem > 0
        if live.any():
            k[live] = st.binom.ppf(U[live, j], rem[live], pc[j])
        X[:, j] = k
        rem -= k
    X[:, d - 1] = rem
    return X


def _check_against_scipy(name, kwargs, tables, X, seed, row0):
    """X: the (n, d) host rows [row0, row0 + n) of stream `seed`."""
    n, d = X.shape
    U = _uniforms(seed, n, d, row0)
    if name == "multivariate_normal":
        mean, A = tables
        X = X.view(np.float64)
        Z = sp.ndtri(U)
        ref = mean + Z @ A.T
        bound = 1e-10 * (np.abs(mean) + np.abs(Z) @ np.abs(A).T)
        assert (np.abs(X - ref) <= bound).all(), (np.abs(X - ref) / bound).max()
    elif name == "dirichlet":
        X = X.view(np.float64)
        G = st.gamma(kwargs["alpha"]).ppf(U)
        ref = G / G.sum(axis=1, keepdims=True)
        assert (np.abs(X - ref) <= 3e-10 * ref).all(), (np.abs(X - ref) / ref).max()
        assert (np.abs(X.sum(axis=1) - 1.0) <= 4 * d * EPS).all()
    else:
        trials, pc = tables
        ref = _multinomial_by_scipy(U, trials, pc)
        if not np.array_equal(X, ref):
            i, j = np.argwhere(X != ref)[0]
            raise AssertionError(f"row {row0 + i} component {j}: device {X[i, j]} scipy {ref[i, j]} at u={U[i, j]!r}")
        assert (X.sum(axis=1) == trials).all()


def _dtype(name):
    return np.int64 if name == "multinomial" else np.float64


@pytest.mark.parametrize("n", [63, 257])
@pytest.mark.parametrize("d", [8, 63, 64, 65, 127])
def test_multivariate_normal_at_the_lds_switch(gpu, d, n):
    """R = 256 (d = 8) and 64; the factor behind the tile in LDS up to d = 64, where the two fill
    the 64 KiB exactly, and read from global memory from d = 65."""
    kwargs = _kwargs("multivariate_normal", d)
    tables = _tables("multivariate_normal", kwargs)
    seed, row0 = 1000 * d + n, 12_345
    flag = Flag()
    blk = _block("multivariate_normal", tables, seed, row0, n, flag)
    _check_against_scipy("multivariate_normal", kwargs, tables, blk.rows(), seed, row0)
    assert flag.value() == 0


@pytest.mark.parametrize("n", [63, 257])
@pytest.mark.parametrize("d", [64, 65, 128])
def test_dirichlet_at_the_tile_heights(gpu, d, n):
    """R = 128 (d = 64) and 64 (d = 65; d = 128, where the tile is the 64 KiB exactly)."""
    kwargs = _kwargs("dirichlet", d)
    tables = _tables("dirichlet", kwargs)
    seed, row0 = 2000 * d + n, 12_345
    flag = Flag()
    blk = _block("dirichlet", tables, seed, row0, n, flag)
    _check_against_scipy("dirichlet", kwargs, tables, blk.rows(), seed, row0)
    assert flag.value() == 0


@pytest.mark.parametrize("n", [63, 257])
@pytest.mark.parametrize("trials", [1, 1000])
@pytest.mark.parametrize("d", [33, 128])
def test_multinomial_wide(gpu, d, trials, n):
    kwargs = _kwargs("multinomial", d, trials)
    assert (kwargs["p"] == 0.0).sum() >= 3 and kwargs["p"].max() == 0.9 and abs(kwargs["p"].sum() - 1.0) < 1e-12
    tables = _tables("multinomial", kwargs)
    seed, row0 = 3000 * d + 7 * trials + n, 12_345
    blk = _block("multinomial", tables, seed, row0, n)
    _check_against_scipy("multinomial", kwargs, tables, blk.rows(np.int64), seed, row0)


# ---------------------------------------------------------------- more tiles than blocks
@pytest.mark.parametrize("name,d,R", [("multivariate_normal", 1, 256), ("multivariate_normal", 2, 256),
                                      ("dirichlet", 2, 256), ("multinomial", 2, 256),
                                      ("multivariate_normal", 33, 192)])
def test_tile_stride_equals_shards(gpu, name, d, R):
    """n = 8192 R + 257: block 0 and block 1 stride to a second tile (k_mvn<true> reuses the factor
    it staged once; at d = 33 that factor is 33 x 40 doubles behind a tile of R = 192 rows).  R is
    the launch's rows per block (tile_rows of pbh_mvar.hip; multinomial: its block of 256).  Bit for
    bit the rows of two shard calls of at most 8192 tiles each, cut off every tile edge; the last 257
    rows, the strided ones, against scipy."""
    kwargs = _kwargs(name, d)
    tables = _tables(name, kwargs)
    if name == "multivariate_normal":  # R as pbh_multivariate_normal derives it: the factor fits LDS at these d
        abytes = d * (-(-d // 8) * 8) * 8
        assert R == min(256, (65536 - abytes) // (8 * d) // 64 * 64)
    n = GRID_CAP * R + 257
    seed, row0 = 99 + d, 1_000
    whole = _block(name, tables, seed, row0, n)
    cut = n // 2 + 3
    assert cut % R and -(-cut // R) <= GRID_CAP and -(-(n - cut) // R) <= GRID_CAP
    for r0, m in [(0, cut), (cut, n - cut)]:
        shard = _block(name, tables, seed, row0 + r0, m)
        shard.assert_same(whole.cols()[:, r0:r0 + m], f"{name} d={d}: shard of rows {r0} .. {r0 + m} vs the whole call")
        del shard
    tail = whole.cols()[:, n - 257:].cpu().numpy().view(_dtype(name)).T
    _check_against_scipy(name, kwargs, tables, tail, seed, row0 + n - 257)


# ---------------------------------------------------------------- the high half of the row counter
@pytest.mark.parametrize("name,d", [("multivariate_normal", 3), ("dirichlet", 3), ("multinomial", 5)])
def test_row0_carries_past_2_32(gpu, name, d):
    """Rows 2^32 - 100 .. 2^32 + 156 in one call: against scipy on fill_uniform at the same row0, and
    bit for bit the two calls that split it at 2^32."""
    import torch

    kwargs = _kwargs(name, d)
    tables = _tables(name, kwargs)
    seed, row0, n = 77, 2 ** 32 - 100, 257
    whole = _block(name, tables, seed, row0, n)
    _check_against_scipy(name, kwargs, tables, whole.rows(_dtype(name)), seed, row0)
    a, b = _block(name, tables, seed, row0, 100), _block(name, tables, seed, 2 ** 32, n - 100)
    whole.assert_same(torch.cat([a.cols(), b.cols()], dim=1), f"{name}: split at 2^32")


# ---------------------------------------------------------------- flags, empty calls, errors
def test_normal_nonfinite_flag(gpu):
    """A factor of 1e308 entries: a row with a normal beyond 1.8 overflows to an infinity or, where
    two of them cancel, a NaN.  The flag word is set, nothing next to it or outside the block is
    written; the finite call beside it leaves the flag 0."""
    d, n = 3, 257
    mean = np.zeros(d)
    for A, want in [(np.full((d, d), 1e308), 1), (np.eye(d), 0)]:
        flag = Flag()
        blk = _block("multivariate_normal", (mean, np.ascontiguousarray(A)), 5, 0, n, flag)
        assert flag.value() == want
        assert np.isfinite(blk.rows()).all() == (want == 0)


@pytest.mark.parametrize("name", SAMPLERS)
def test_empty_call_writes_nothing(gpu, name):
    tables = _tables(name, _kwargs(name, 3))
    blk, flag = Block(4, 3), Flag()
    assert _call(name, tables, 1, 0, 0, 3, blk.ptr, blk.ld, flag.ptr) == 0
    assert _call(name, tables, 1, 2 ** 40, 0, 3, None, 0, flag.ptr) == 0
    assert blk.untouched() and flag.value() == 0


@pytest.mark.parametrize("name", SAMPLERS)
def test_bad_geometry_is_an_error(gpu, name):
    """ld < nrows, d = 0 and d = 129: an error with a message, and no write."""
    from probabilit_amd import _lib

    n = 70
    tables = _tables(name, _kwargs(name, 3))
    wide = {"multivariate_normal": (np.zeros(129), np.eye(129)), "dirichlet": (np.ones(129),),
            "multinomial": (10.0, np.full(129, 0.5))}[name]
    blk, flag = Block(n, 3), Flag()
    for what, tb, d, ld in [("ld < nrows", tables, 3, n - 1), ("d = 0", tables, 0, blk.ld), ("d = 129", wide, 129, blk.ld)]:
        status = _call(name, tb, 1, 0, n, d, blk.ptr, ld, flag.ptr)
        assert status != 0, what
        assert _lib.last_error(), what
        assert blk.untouched() and flag.value() == 0, what
