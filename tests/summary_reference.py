"""Exact references and a-priori error bounds for pbh_moments (shared by the summary kernel tests
and the inspection tests; not a test module).

Every finite double is an integer times a power of two, so the sums a moment is made of are
computed in Python integers without any rounding, centred about the very mean the kernel
returned (the header defines m_p about that mean).  The allowed error comes from the summation
shape documented beside pbh_moments' declaration, never from an observed error."""

from fractions import Fraction

import numpy as np

EPS = Fraction(1, 2 ** 52)


def _exact_ints(values):
    """(object array of Python ints X, shift s) with values == X * 2**s exactly."""
    m, e = np.frexp(np.asarray(values, dtype=np.float64))
    M = (m * 2.0 ** 53).astype(np.int64)  # exact: m has 53 significant bits
    e = e.astype(np.int64) - 53
    e[M == 0] = e[M != 0].min() if (M != 0).any() else 0
    s = int(e.min())
    return M.astype(object) * (2 ** (e - s).astype(object)), s


def header_terms(n):
    """L(n) and D as include/probabilit_hip.h states them (restated here on purpose: the test
    fails if native.moments_terms and the documented formula drift apart)."""
    tiles = -(-n // 2048)
    blocks = min(tiles, 1024)
    return 8 * -(-tiles // blocks) + -(-blocks // 256), 16


def check_moments(x, got, what=""):
    """got: the kernel's dict / row (mean, m2, m3, m4) for the finite float64 vector x.  Asserts
    |got - exact| <= (L + D + p + 1) eps mean(|x - mean|^p), p = 0 (terms |x|) for the mean itself."""
    n = len(x)
    L, D = header_terms(n)
    X, s = _exact_ints(np.append(x, got["mean"]))
    X, C = X[:-1], X[-1]
    scale = Fraction(2) ** s
    exact = Fraction(int(X.sum())) * scale / n
    bound = (L + D + 1) * EPS * Fraction(int(np.abs(X).sum())) * scale / n
    err = abs(Fraction(got["mean"]) - exact)
    print(f"{what} n={n} mean: error {float(err):.3e} bound {float(bound):.3e}")
    assert err <= bound, (what, "mean", float(err), float(bound))
    Dv = X - C
    D2 = Dv * Dv
    powers = {2: D2, 3: D2 * Dv, 4: D2 * D2}
    for p, P in powers.items():
        exact = Fraction(int(P.sum())) * scale ** p / n
        bound = (L + D + p + 1) * EPS * Fraction(int(np.abs(P).sum())) * scale ** p / n
        err = abs(Fraction(got[f"m{p}"]) - exact)
        print(f"{what} n={n} m{p}: error {float(err):.3e} bound {float(bound):.3e}")
        assert err <= bound, (what, f"m{p}", float(err), float(bound))
