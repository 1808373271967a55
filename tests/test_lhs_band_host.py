"""The band table of the reference-LHS device decode (band_table of csrc/pbh_lhs_dev.hip, read
through the host-only pbh_lhs_reference_band_table) against the sequential stream itself: no GPU.

The decode classifies every draw of a column against the band of states the column can be in at
that draw.  A band that is off centre or too narrow never gives a wrong matrix: the decode checks
itself and hands the call to the host shuffles, so only the device path is lost.  These tests look
at the table directly:

  mirror       tests/lhs_mirror.py, a plain Python random_interval on the paired 32-bit stream, is
               pinned to numpy's Generator.shuffle first (values and draws consumed, with and
               without a buffered half), so that it is a reference and not a restatement
  shape        tcap, nband and the room after the expected end
  centre       the table's expected steps against the exact inverse of
               D(s) = sum_{i = n-s .. n-1} (mask(i) + 1) / (i + 1)
  containment  the true steps done before every draw of real columns lie inside the interval
               draw_band computes from the table (restated here) at the default 6 sigma
"""

import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import lhs_mirror as lm

BLK, BAND = 4096, 1024  # kBlk, 1 << kBandLog of pbh_lhs_dev.hip


def band_table(n, sigmas=6.0):
    """(table (nband, 2), tcap) of pbh_lhs_reference_band_table."""
    from probabilit_amd import _lib

    lib = _lib.load()  # host-only entry point: no GPU is touched
    nband, tcap = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.pbh_lhs_reference_band_table(n, sigmas, None, 0, ctypes.byref(nband), ctypes.byref(tcap)))
    out = np.full((nband.value + 1, 2), -7.0)
    _lib.check(lib.pbh_lhs_reference_band_table(n, sigmas, _lib.np_ptr(out), nband.value, ctypes.byref(nband),
                                                ctypes.byref(tcap)))
    assert np.all(out[-1] == -7.0), "a write past the entries asked for"
    return out[:-1], tcap.value


def draw_band(table, n, tau):
    """draw_band of pbh_lhs_dev.hip for an array of draws tau: (inside, slo, shi), the steps done
    before the draw that the band holds (the kernel's ihi = n - 1 - slo, ilo = n - 1 - shi)."""
    tau = np.asarray(tau, dtype=np.int64)
    nband, N1 = table.shape[0], n - 1
    bi = tau >> 10
    f = (tau & (BAND - 1)).astype(np.float64) * (1.0 / BAND)
    b0 = table[np.minimum(bi, nband - 1)]
    b1 = table[np.minimum(bi + 1, nband - 1)]
    se = b0[:, 0] + (b1[:, 0] - b0[:, 0]) * f
    e = np.maximum(b0[:, 1], b1[:, 1]) + 2.0
    lo, hi = np.floor(se - e), np.ceil(se + e)
    inside = ~(lo > float(N1 - 1))
    slo = np.where(lo < 0.0, 0, lo).astype(np.int64)
    shi = np.where(hi > float(N1 - 1), N1 - 1, np.maximum(slo, hi.astype(np.int64)))
    return inside, slo, shi


def expected_draws(n):
    """D(0 .. n-1) in extended precision: D[s] = the expected draws of the first s steps."""
    i = np.arange(n - 1, 0, -1, dtype=np.int64)
    m1 = (1 << np.floor(np.log2(i)).astype(np.int64) + 1).astype(np.longdouble)
    terms = m1 / (i + 1).astype(np.longdouble)
    return np.concatenate([[np.longdouble(0)], np.cumsum(terms)])


# ---------------------------------------------------------------- the mirror against numpy
@pytest.mark.parametrize("has32", [0, 1])
@pytest.mark.parametrize("n", [2, 3, 17, 256, 257, 2900])
def test_mirror_matches_numpy_shuffle(n, has32):
    """The mirror's swap targets applied to arange(1, n + 1) equal Generator.shuffle from the same
    state, for three shuffles in a row: the second and third start where the mirror says the one
    before ended, so the draws consumed are pinned too."""
    seed = np.random.default_rng(1000 * n + has32)
    state, inc = int(seed.integers(0, 2**63)) << 64 | int(seed.integers(0, 2**63)), int(seed.integers(0, 2**62)) << 1 | 1
    buf32 = int(seed.integers(0, 2**32)) if has32 else 0
    g = lm.generator(state, inc, has32, buf32)
    cols = lm.columns(g, n, 3)
    for c, (start, end, steps, targets) in enumerate(cols):
        x = np.arange(1, n + 1)
        g.shuffle(x)
        np.testing.assert_array_equal(lm.apply_targets(targets), x, err_msg=f"n={n} has32={has32} column {c}")
        assert len(steps) == end - start and steps[0] == 0 and steps[-1] == n - 2
        assert all(b - a in (0, 1) for a, b in zip(steps, steps[1:]))
    # the generator after the three shuffles: the whole outputs taken and the half left over
    taken = cols[-1][1] - has32
    after = g.bit_generator.state
    ref = lm.generator(state, inc).bit_generator
    ref.advance((taken + 1) // 2)
    assert after["state"]["state"] == ref.state["state"]["state"]
    assert after["has_uint32"] == taken % 2


def test_expected_draws_exact():
    """The extended-precision D(s) against exact rationals."""
    n = 1000
    D = expected_draws(n)
    exact = Fraction(0)
    for s, i in enumerate(range(n - 1, 0, -1), start=1):
        exact += Fraction(lm.mask_of(i) + 1, i + 1)
        if s % 37 == 0 or s == n - 1:
            assert abs(float(D[s]) - float(exact)) <= 4e-16 * float(exact), s
    assert math.isclose(float(D[-1]), math.fsum((lm.mask_of(i) + 1) / (i + 1) for i in range(1, n)), rel_tol=1e-15)


# ---------------------------------------------------------------- the table
SIZES = [2, 3, 17, 255, 256, 257, 1000, 2790, 65537]


@pytest.mark.parametrize("sigmas", [6.0, 12.0, 1e5])
@pytest.mark.parametrize("n", SIZES + [1_000_003])
def test_band_table_shape(n, sigmas):
    table, tcap = band_table(n, sigmas)
    assert tcap % BLK == 0
    assert table.shape[0] == tcap // BAND + 2
    assert tcap >= float(expected_draws(n)[-1]) + BLK
    assert np.all(np.isfinite(table)) and np.all(table[:, 1] >= 16.0) and np.all(np.diff(table[:, 0]) >= 0.0)
    assert table[0, 0] == 0.0


@pytest.mark.parametrize("n", SIZES + [1_000_003, 2**24 + 1])
def test_band_table_centre(n):
    """For every entry k with tau = 1024 k < D(n - 1) the table's expected steps differ from the
    exact inverse of D at tau (D interpolated linearly between integer steps) by at most one step
    plus 1e-9 n.  The bound is derived: band_table inverts the closed form
    (m + 1) (H(hi + 1) - H(x)) of a mask range, which equals D at every integer x and is monotone
    between integers, so its inverse and the interpolated one lie between the same two integers;
    the rest is the digamma series and Newton's residual.

    Largest deviation observed: 0.0243 steps (n = 2790, tau = 4096, the entry inside the last
    mask ranges); 0.0033 at n = 2^24 + 1 and below 0.0003 at the other sizes, so the bound holds
    with the table as it is."""
    table, tcap = band_table(n)
    D = expected_draws(n)
    k = np.arange(table.shape[0])
    k = k[(k * BAND).astype(np.longdouble) < D[-1]]
    assert k.size >= 1
    tau = (k * BAND).astype(np.longdouble)
    s0 = np.searchsorted(D, tau, side="right") - 1  # D[s0] <= tau < D[s0 + 1]
    assert np.all(s0 >= 0) and np.all(s0 < n - 1)
    exact = s0 + ((tau - D[s0]) / (D[s0 + 1] - D[s0])).astype(np.float64)
    dev = np.abs(table[k, 0] - exact)
    print(f"n={n}: {k.size} entries, largest centre deviation {dev.max():.3g} steps at tau = {BAND * int(k[dev.argmax()])}")
    assert dev.max() <= 1.0 + 1e-9 * n, (n, float(dev.max()), int(k[dev.argmax()]))


SEEDS = list(range(20))


@pytest.mark.parametrize("n", SIZES)
def test_band_contains_true_states(n):
    """At the default 6 sigma, over 20 seeds: the steps done before every draw a column consumes
    lie inside draw_band's interval for that draw, and the column ends before tcap.  The words
    come from PCG64(seed) through the mirror alone.  (No seed had to be swapped.)"""
    table, tcap = band_table(n)
    for seed in SEEDS:
        g = np.random.Generator(np.random.PCG64(seed))
        end, steps, _ = lm.column(lm.words32(g, lm.draws_needed(n, 1)), n)
        assert end < tcap, (n, seed, end, tcap)
        steps = np.array(steps, dtype=np.int64)
        inside, slo, shi = draw_band(table, n, np.arange(end))
        bad = ~inside | (steps < slo) | (steps > shi)
        if bad.any():
            t = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"n={n} seed={seed}: {int(bad.sum())} draws outside the band, first at draw {t}: "
                                 f"{int(steps[t])} steps done, band [{int(slo[t])}, {int(shi[t])}]")


def test_band_width_is_six_sigma():
    """The half-width at 6 sigma is 6 standard deviations of the steps done, measured: over 400
    columns at n = 2790 the spread of the steps done at the table's draws is never above
    (half-width - 16) / 6 by more than its own sampling error (5 %, 10 % allowed)."""
    n, cols = 2790, 400
    table, tcap = band_table(n)
    taus = [BAND * k for k in range(1, 4)]
    at = np.empty((cols, len(taus)))
    for seed in range(cols):
        g = np.random.Generator(np.random.PCG64(10_000 + seed))
        end, steps, _ = lm.column(lm.words32(g, lm.draws_needed(n, 1)), n)
        assert end > taus[-1]
        at[seed] = [steps[t] for t in taus]
    sd = at.std(axis=0, ddof=1)
    claimed = (table[1:4, 1] - 16.0) / 6.0
    assert np.all(sd <= 1.10 * claimed), (sd, claimed)
    assert np.all(np.abs(at.mean(axis=0) - table[1:4, 0]) <= 1.0 + 4 * sd / math.sqrt(cols)), (at.mean(axis=0), table[1:4, 0])


# ---------------------------------------------------------------- refusals
def test_band_table_refusals():
    from probabilit_amd import _lib

    lib = _lib.load()
    nband, tcap = ctypes.c_int64(-5), ctypes.c_int64(-5)
    out = np.full(8, -7.0)
    nb, tc = ctypes.byref(nband), ctypes.byref(tcap)
    for args in [(1, 6.0, None, 0, nb, tc), (0, 6.0, None, 0, nb, tc), (2**31, 6.0, None, 0, nb, tc),
                 (1000, 0.0, None, 0, nb, tc), (1000, -1.0, None, 0, nb, tc), (1000, float("nan"), None, 0, nb, tc),
                 (1000, 6.0, None, 0, None, tc), (1000, 6.0, None, 0, nb, None), (1000, 6.0, None, 4, nb, tc),
                 (1000, 6.0, _lib.np_ptr(out), -1, nb, tc)]:
        assert lib.pbh_lhs_reference_band_table(*args) == _lib.ERR_INVALID, args
        assert "pbh_lhs_reference_band_table" in _lib.last_error()
        assert nband.value == -5 and tcap.value == -5 and np.all(out == -7.0)
    # fewer entries than the table has: only those are written
    assert lib.pbh_lhs_reference_band_table(1000, 6.0, _lib.np_ptr(out), 3, nb, tc) == _lib.OK
    assert nband.value == tcap.value // BAND + 2 and nband.value > 3
    assert np.all(out[:6] != -7.0) and np.all(out[6:] == -7.0)
    # n = 2: one step, one draw
    assert lib.pbh_lhs_reference_band_table(2, 6.0, None, 0, nb, tc) == _lib.OK
    assert tcap.value == BLK * 2 or tcap.value == BLK
