"""CPU checks of the multivariate samplers (multivariate_normal, dirichlet, multinomial): the numpy
helpers of probabilit_amd.native, the per-row functions of csrc/pbh_mvar.h compiled for the host
(tests/native/multivariate_host.cpp) against scipy on uniforms numpy supplies, and the host-side
validation, which must raise before anything touches the device.

Gates (the project's): the normal quantile and gammaincinv are within 1e-10 relative of scipy's, so
a sum of normals is within 1e-10 of the sum of the terms' magnitudes and a ratio of gammas within
2e-10 plus rounding (3e-10); discrete outputs are exact.  The host build calls glibc's libm where
the device calls its own, so this pins the algorithms; tests/test_gpu_multivariate.py pins the
kernels."""

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.special as sp
import scipy.stats as st

from probabilit_amd import native
from probabilit_amd.modeling import Distribution

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "multivariate_host.cpp")
OUT = os.path.join(HERE, "native", "_build", "libpbh_multivariate_host.so")
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def mvh():
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "probabilit_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".inc"))]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                        "-I", csrc, "-I", os.path.join(ROOT, "include"), SRC, "-o", OUT], check=True, capture_output=True)
    return ctypes.CDLL(OUT)


def _uniforms(n, d, seed):
    """uniform draws plus both tails and the substitute for u == 0"""
    rng = np.random.default_rng(seed)
    U = rng.random((n, d))
    U[0, :] = 2.0 ** -53
    U[1, :] = 1.0 - 2.0 ** -53
    U[2, :] = 10.0 ** rng.uniform(-12, -1, d)
    U[3, :] = 1.0 - 10.0 ** rng.uniform(-12, -1, d)
    return np.ascontiguousarray(U)


# ---------------------------------------------------------------- numpy helpers
def test_mvn_factor_reproduces_cov():
    rng = np.random.default_rng(0)
    B = rng.normal(size=(5, 5))
    spd = B @ B.T + 0.5 * np.eye(5)
    v = rng.normal(size=(3, 2))
    psd = v @ v.T  # rank 2
    for cov in (spd, psd):
        A = native.mvn_factor(cov)
        assert A.shape == cov.shape
        assert np.abs(A @ A.T - cov).max() <= 1e-12 * np.linalg.norm(cov)
    assert native.mvn_factor(4.0).shape == (1, 1) and native.mvn_factor(4.0)[0, 0] == 2.0


def test_multinomial_conditionals():
    p = np.array([0.2, 0.3, 0.1, 0.4])
    want = np.clip(p / (1.0 - np.concatenate([[0.0], np.cumsum(p)[:-1]])), 0.0, 1.0)
    got = native.multinomial_conditionals(p)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_allclose(got, [0.2, 0.375, 0.2, 1.0], rtol=1e-15)
    short = np.array([0.25, 0.25, 0.5 - 2.0 ** -53])  # float sum 1 - 2^-53
    assert short.sum() == 1.0 - 2.0 ** -53
    zero = np.array([0.5, 0.0, 0.5, 0.0])
    for q in (short, zero, np.array([1.0, 0.0, 0.0]), np.array([0.1] * 10)):
        pc = native.multinomial_conditionals(q)
        assert pc.shape == q.shape and np.isfinite(pc).all() and (pc >= 0.0).all() and (pc <= 1.0).all()
    np.testing.assert_array_equal(native.multinomial_conditionals(zero), [0.5, 0.0, 1.0, 0.0])


# ---------------------------------------------------------------- per-row functions
def test_uniforms_are_counter_addressed(mvh):
    """u(i, j) depends on (seed, row0 + i, j) only, and lies in (0, 1)."""
    a, b = np.empty((300, 5)), np.empty((40, 5))
    mvh.mvh_uniforms(ctypes.c_ulonglong(9), ctypes.c_long(0), ctypes.c_long(300), 5, P(a.ctypes.data))
    mvh.mvh_uniforms(ctypes.c_ulonglong(9), ctypes.c_long(200), ctypes.c_long(40), 5, P(b.ctypes.data))
    np.testing.assert_array_equal(a[200:240], b)
    assert (a > 0.0).all() and (a < 1.0).all() and abs(a.mean() - 0.5) < 0.05


@pytest.mark.parametrize("d", [1, 2, 3, 9, 33, 128])
def test_mvn_rows_match_scipy(mvh, d):
    rng = np.random.default_rng(d)
    B = rng.normal(size=(d, d))
    cov = B @ B.T / d + 0.1 * np.eye(d)
    mean = np.ascontiguousarray(rng.normal(scale=3.0, size=d))
    A = native.mvn_factor(cov)
    U = _uniforms(65, d, d)
    out = np.empty_like(U)
    mvh.mvh_mvn(P(mean.ctypes.data), P(A.ctypes.data), d, P(U.ctypes.data), ctypes.c_long(U.shape[0]), P(out.ctypes.data))
    Z = sp.ndtri(U)
    ref = mean + Z @ A.T
    bound = 1e-10 * (np.abs(mean) + np.abs(Z) @ np.abs(A).T)
    assert (np.abs(out - ref) <= bound).all(), (np.abs(out - ref) / bound).max()


@pytest.mark.parametrize("guided", [0, 1])
@pytest.mark.parametrize("d", [2, 3, 33])
def test_dirichlet_rows_match_scipy(mvh, d, guided):
    rng = np.random.default_rng(10 + d)
    alpha = np.ascontiguousarray(rng.choice([0.5, 1.0, 2.5, 7.0], size=d))
    U = _uniforms(257, d, d)
    out, bad = np.empty_like(U), np.empty(U.shape[0], dtype=np.int32)
    mvh.mvh_dirichlet(P(alpha.ctypes.data), d, guided, P(U.ctypes.data), ctypes.c_long(U.shape[0]), P(out.ctypes.data),
                      P(bad.ctypes.data))
    G = st.gamma(alpha).ppf(U)
    ref = G / G.sum(axis=1, keepdims=True)
    assert not bad.any()
    assert (np.abs(out - ref) <= 3e-10 * ref).all(), (np.abs(out - ref) / ref).max()
    assert (np.abs(out.sum(axis=1) - 1.0) <= 4 * d * np.finfo(float).eps).all()


def test_dirichlet_underflow_is_flagged(mvh):
    """igami underflows to 0 for every component: the row is 0 / 0 and reported."""
    alpha = np.array([1e-300, 1e-300])
    U = np.ascontiguousarray(np.random.default_rng(1).random((8, 2)))
    out, bad = np.empty_like(U), np.empty(8, dtype=np.int32)
    mvh.mvh_dirichlet(P(alpha.ctypes.data), 2, 0, P(U.ctypes.data), ctypes.c_long(8), P(out.ctypes.data), P(bad.ctypes.data))
    assert bad.all() and np.isnan(out).all()


def multinomial_by_scipy(U, n, p):
    """the sampler's sequential rule with scipy.stats.binom.ppf"""
    pc = native.multinomial_conditionals(p)
    N, d = U.shape
    rem = np.full(N, float(n))
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


@pytest.mark.parametrize("n", [0, 1, 10, 1000])
@pytest.mark.parametrize("p", [[0.3, 0.7], [0.2, 0.0, 0.8], [0.005, 0.98, 0.005, 0.005, 0.005], [0.5, 0.5, 0.0],
                               [1.0]])
def test_multinomial_rows_equal_scipy(mvh, n, p):
    d = len(p)
    U = _uniforms(513, d, n + d)
    pc = native.multinomial_conditionals(p)
    out = np.empty(U.shape, dtype=np.int64)
    mvh.mvh_multinomial(ctypes.c_double(n), P(pc.ctypes.data), d, P(U.ctypes.data), ctypes.c_long(U.shape[0]),
                        P(out.ctypes.data))
    np.testing.assert_array_equal(out, multinomial_by_scipy(U, n, p))
    assert (out.sum(axis=1) == n).all() and (out >= 0).all()


# ---------------------------------------------------------------- validation, before any device call
@pytest.fixture
def no_device(monkeypatch):
    """every route to the device raises a marker error"""
    import probabilit_amd.device as dev

    def boom(*a, **k):
        raise AssertionError("the device was touched before validation")

    monkeypatch.setattr(dev, "device", boom)
    monkeypatch.setattr(dev, "stream", boom)


def test_bad_cov_raises_scipys_error(no_device):
    with pytest.raises(ValueError, match="positive semidefinite"):
        Distribution("multivariate_normal", mean=[0, 0], cov=[[1, 2], [2, 1]]).sample(5, random_state=0)
    with pytest.raises(ValueError, match="positive semidefinite"):
        Distribution("multivariate_normal", mean=[0, 0], cov=[[1, 2], [2, 1]]).sample_from_quantiles(np.full((5, 1), 0.5))


@pytest.mark.parametrize("name,kwargs", [("dirichlet", {"alpha": np.ones(129)}),
                                         ("multinomial", {"n": 5, "p": np.full(129, 1 / 129)}),
                                         ("multivariate_normal", {"mean": np.zeros(129), "cov": np.eye(129)})])
def test_too_many_components_raise(no_device, name, kwargs):
    with pytest.raises(ValueError, match="at most 128"):
        Distribution(name, **kwargs).sample(5, random_state=0)


def test_128_components_are_accepted():
    d, (alpha,) = native.multivariate_tables("dirichlet", st.dirichlet(np.ones(128)))
    assert d == 128 and alpha.shape == (128,)


def test_node_parameter_is_declined(no_device):
    loc = Distribution("norm")
    with pytest.raises(NotImplementedError, match="Node"):
        Distribution("multivariate_normal", mean=loc, cov=np.eye(2)).sample(5, random_state=0)
    with pytest.raises(NotImplementedError, match="Node"):
        Distribution("dirichlet", alpha=loc).sample(5, random_state=0)
