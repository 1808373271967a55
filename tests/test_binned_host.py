"""The host side of probabilit_amd.inspection's conditional statistics (no kernel is launched):
binned_finish and correlation_ratio over raw sums formed with numpy and math.fsum against
scipy.stats.binned_statistic, the edge builders against numpy, and every argument error."""

import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.stats

from binned_reference import U, correlation_ratio_bound, finish_bounds, raw_sums, reference_allowance
from conftest import ROOT

from probabilit_amd import inspection

STATISTICS = ("count", "sum", "mean", "std")
RNG = np.random.default_rng(23)
N = 4000
X0 = RNG.standard_normal(N)
X = X0.copy()
X[:5] = [np.nan, -7.0, 7.0, 2.5, -2.0]  # a NaN, rows outside, rows on the outer edges
# bins: ordinary ones, two that nothing falls in (2 and 5; scipy refuses a repeated edge, which
# tests/test_gpu_binned_kernels.py covers against np.histogram) and a one-row bin (4)
EDGES = np.array([-2.0, -0.5, 0.3, 0.3 + 1e-9, 1.0, 1.0 + 1e-9, 1.0 + 2e-9, 2.5])
X[5] = 1.0 + 5e-10  # the one row of bin 4
assert not ((X >= 1.0) & (X < 1.0 + 2e-9))[6:].any() and not ((X >= 0.3) & (X < 0.3 + 1e-9)).any()
VALUES = {
    "spread": 3.0 + 2.0 * RNG.standard_normal(N) + X0,
    "offset": 1e9 + RNG.standard_normal(N),
    "integers": RNG.integers(-3, 4, N).astype(np.float64),
}


def _finished(y, centre, statistic):
    count, s1, s2, a1 = raw_sums(X, y, EDGES, centre)
    return inspection.binned_finish(count, s1, s2, centre, statistic), finish_bounds(count, s1, s2, a1, centre)


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("data", list(VALUES))
@pytest.mark.parametrize("centred", [True, False])
def test_binned_finish_is_scipys(data, statistic, centred):
    """Within the bound the raw sums' roundings allow and scipy's own.  offset (1e9 + noise) about
    centre 0 is the case the centre exists for: std's bound is then wider than the std itself, so
    only the centred std is asked to agree."""
    y = VALUES[data]
    inside = np.isfinite(X)  # (scipy refuses a NaN in x)
    want = scipy.stats.binned_statistic(X[inside], y[inside], statistic, bins=EDGES)[0]
    centre = float(np.mean(y)) if centred else 0.0
    got, bounds = _finished(y, centre, statistic)
    assert got.dtype == np.float64 and got.shape == want.shape == (7,)
    count = raw_sums(X, y, EDGES, 0.0)[0]
    assert count[2] == 0 and count[5] == 0 and count[4] == 1 and count[6] >= 1
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if statistic in ("count", "sum"):
        assert got[2] == 0.0 and got[5] == 0.0
    else:
        assert np.isnan(got[2]) and np.isnan(got[5])
    tol = bounds[statistic] + reference_allowance(X, y, EDGES, statistic)
    err = np.abs(got - want)
    print(data, statistic, centred, "error", err, "bound", tol)
    if data == "offset" and statistic == "std" and not centred:
        has = count > 1
        assert (bounds["std"][has] > want[has]).all()  # the bound says nothing: the reason for the centre
        return
    has = count > 0
    assert (err[has] <= tol[has]).all()
    if statistic == "std":
        assert got[4] == 0.0  # one row: s2 and m1^2 are the same product


def test_centred_std_of_offset_data_is_tight():
    got, bounds = _finished(VALUES["offset"], float(np.mean(VALUES["offset"])), "std")
    has = raw_sums(X, X, EDGES, 0.0)[0] > 1
    assert (bounds["std"][has] < 1e-11).all() and (got[has] > 0.5).all()


def test_binned_finish_propagates_a_poisoned_bin_only():
    count, s1, s2 = np.array([3, 2, 0]), np.array([np.nan, 1.0, 0.0]), np.array([np.inf, 4.0, 0.0])
    for statistic in ("sum", "mean", "std"):
        got = inspection.binned_finish(count, s1, s2, 0.5, statistic)
        assert np.isnan(got[0]) and np.isfinite(got[1])
    assert inspection.binned_finish(count, s1, s2, 0.5, "count").tolist() == [3.0, 2.0, 0.0]
    assert inspection.binned_finish(count, s1, s2, 0.5, "sum")[1:].tolist() == [2.0, 0.0]
    assert inspection.binned_finish(count, s1, s2, 0.5, "mean")[1] == 1.0


def _eta2(x, y, edges):
    """Var(E[Y | X]) / Var(Y) over the rows inside the edges, in exact rational arithmetic."""
    from binned_reference import exact_correlation_ratio

    return exact_correlation_ratio(x, y, edges)


@pytest.mark.parametrize("data", list(VALUES))
@pytest.mark.parametrize("centred", [True, False])
def test_correlation_ratio(data, centred):
    y = VALUES[data]
    centre = float(np.mean(y)) if centred else 0.0
    count, s1, s2, a1 = raw_sums(X, y, EDGES, centre)
    got = inspection.correlation_ratio(count, s1, s2)
    want = _eta2(X, y, EDGES)
    bound = correlation_ratio_bound(count, s1, s2, a1) + U  # (the exact reference is rounded once)
    print(data, centred, got, want, bound)
    assert -bound <= got <= 1.0 + bound and abs(got - want) <= bound
    if data == "offset":  # without the centre the bound is wider than the ratio itself; with it, tight
        assert bound < 1e-9 * want if centred else bound > want
    if data == "spread":
        assert got > 0.1  # y = ... + x


def test_correlation_ratio_extremes():
    cr = inspection.correlation_ratio
    assert cr([2, 2], [2.0, -2.0], [2.0, 2.0]) == 1.0  # y = +-1 by bin: the bins explain everything
    assert cr([2, 2], [0.0, 0.0], [2.0, 2.0]) == 0.0  # equal conditional means
    assert np.isnan(cr([0, 0], [0.0, 0.0], [0.0, 0.0]))  # no rows
    assert np.isnan(cr([3, 1], [0.0, 0.0], [0.0, 0.0]))  # a constant y
    assert np.isnan(cr([3, 1], [np.nan, 0.0], [np.nan, 1.0]))
    assert cr([4, 0, 4], [4.0, 0.0, -4.0], [4.0, 0.0, 4.0]) == 1.0  # an empty bin takes no part
    with pytest.raises(ValueError, match="one length"):
        cr([1, 2], [1.0], [1.0, 2.0])


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("bins", [1, 2, 10, 32, 1024, np.int64(7)])
def test_uniform_edges_are_numpys(bins):
    x = VALUES["spread"]
    got = inspection.uniform_edges(bins, x.min(), x.max())
    assert got.tobytes() == np.histogram_bin_edges(x, bins=bins).tobytes()
    flat = inspection.uniform_edges(bins, 2.5, 2.5)  # a constant column: widened by 0.5
    assert flat.tobytes() == np.histogram_bin_edges(np.full(9, 2.5), bins=bins).tobytes()
    assert flat[0] == 2.0 and flat[-1] == 3.0


@pytest.mark.parametrize("n", [1, 2, 5, 64, 1000, 4001])
@pytest.mark.parametrize("bins", [1, 2, 3, 32, 100])
def test_quantile_edges_are_nearest_rank_order_statistics(n, bins):
    x = np.sort(np.random.default_rng(n * 1000 + bins).standard_normal(n))
    ranks = inspection.quantile_ranks(n, bins)
    assert ranks.dtype == np.int64 and len(ranks) == bins + 1 and ranks[0] == 0 and ranks[-1] == n - 1
    assert (np.diff(ranks) >= 0).all()
    want = np.quantile(x, np.arange(bins + 1) / bins, method="nearest")
    if n > 1:
        got = inspection.quantile_edges(x[ranks])
        assert got.tobytes() == want.tobytes() and got[0] == x.min() and got[-1] == x.max()
        if bins <= n - 1:  # equal probability: every bin's rows within one of n / bins (the last is closed)
            count = np.histogram(x, got)[0]
            assert np.abs(count - n / bins).max() <= 2.0  # (a rank rounds by 1/2 at each end; the last bin's + 1)
    else:
        got = inspection.quantile_edges(x[ranks])
        assert got[0] == x[0] - 0.5 and got[-1] == x[0] + 0.5


def test_quantile_edges_keep_ties_and_widen_a_constant():
    x = np.sort(np.array([0.0] * 50 + [1.0] * 30 + [2.0] * 20))
    e = inspection.quantile_edges(x[inspection.quantile_ranks(100, 10)])
    assert e.tolist() == [0.0] * 5 + [1.0] * 4 + [2.0] * 2  # repeated edges: empty bins
    assert np.histogram(x, e)[0].tolist() == [0, 0, 0, 0, 50, 0, 0, 0, 30, 20]
    e = inspection.quantile_edges([3.0, 3.0, 3.0, 3.0])
    assert e.tolist() == [2.5, 3.0, 3.0, 3.5]
    given = np.array([1.0, 1.0])
    assert inspection.quantile_edges(given).tolist() == [0.5, 1.5] and given.tolist() == [1.0, 1.0]  # a copy


# ---------------------------------------------------------------- argument errors
def test_host_argument_errors():
    i = inspection
    with pytest.raises(ValueError, match="count.*sum.*mean.*std"):
        i.binned_finish([1], [1.0], [1.0], 0.0, "median")
    with pytest.raises(ValueError, match="one shape"):
        i.binned_finish([1, 2], [1.0], [1.0], 0.0, "mean")
    with pytest.raises(ValueError, match="autodetected range of .* is not finite"):
        i.quantile_edges([0.0, 1.0, np.nan])
    with pytest.raises(ValueError, match="not finite"):
        i.quantile_edges([-np.inf, 1.0])
    with pytest.raises(ValueError, match="non-decreasing"):
        i.quantile_edges([0.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="at least two"):
        i.quantile_edges([0.0])
    with pytest.raises(ValueError, match="must be positive"):
        i.quantile_ranks(10, 0)
    with pytest.raises(TypeError):
        i.quantile_ranks(10, 2.5)
    with pytest.raises(ValueError, match="must be positive"):
        i.uniform_edges(0, 0.0, 1.0)
    with pytest.raises(TypeError, match="must be an integer"):
        i.uniform_edges(2.5, 0.0, 1.0)
    with pytest.raises(ValueError, match=r"autodetected range of \[0.0, inf\] is not finite"):
        i.uniform_edges(4, 0.0, np.inf)
    with pytest.raises(ValueError, match="autodetected range"):
        i.uniform_edges(4, np.nan, np.nan)


def test_device_calls_check_their_arguments_before_any_sample_is_read():
    """Nodes that were never sampled: what is wrong with the other arguments is said first where it
    can be, and otherwise the nodes raise as `.samples_` does."""
    from probabilit_amd.modeling import Distribution

    a, b = Distribution("norm"), Distribution("norm")
    for statistic in ("median", "min", "max", np.mean):
        with pytest.raises(ValueError, match="count.*sum.*mean.*std"):
            inspection.binned_statistic(a, b, statistic)
    with pytest.raises(ValueError, match="1 to 128 value nodes"):
        inspection.binned_statistic(a, [])
    with pytest.raises(ValueError, match="1 to 128 value nodes"):
        inspection.binned_statistic(a, [b] * 129)
    with pytest.raises(ValueError, match="1 to 128 inputs"):
        inspection.sensitivity(a)
    with pytest.raises(ValueError, match="1 to 128 inputs"):
        inspection.sensitivity(a, *[b] * 129)
    with pytest.raises(ValueError, match="'quantile' or 'uniform'"):
        inspection.sensitivity(a, b, binning="kmeans")
    for bins in (0, 1025, -1):
        with pytest.raises(ValueError, match="1 to 1024 bins"):
            inspection.sensitivity(a, b, bins=bins)
    with pytest.raises(TypeError, match="integer"):
        inspection.sensitivity(a, b, bins=2.5)
    with pytest.raises(AttributeError) as want:
        a.samples_
    for call in (lambda: inspection.binned_statistic(a, b), lambda: inspection.binned_statistic(a, [b, b]),
                 lambda: inspection.sensitivity(a, b)):
        with pytest.raises(AttributeError) as got:
            call()
        assert str(got.value) == str(want.value)


def test_row_sharded_samples_are_refused_as_elsewhere():
    """A node marked as one rank's shard of a process group is refused before its samples are
    touched."""
    from probabilit_amd.modeling import Distribution

    a, b = Distribution("norm"), Distribution("norm")
    for node in (a, b):
        node.__dict__["_smp"] = object()
        node.__dict__["_shard"] = (0, 2)
    for call in (lambda: inspection.binned_statistic(a, b), lambda: inspection.sensitivity(a, b)):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            call()


# ---------------------------------------------------------------- Sensitivity
def _sensitivity():
    labels, eta = ["x1", "x2", "x3"], [0.2, 0.7, np.nan]
    edges = [np.linspace(0.0, 1.0, 5)] * 3
    counts = [np.array([3, 0, 2, 5])] * 3
    means = [np.array([1.0, np.nan, 2.0, 4.0])] * 3
    return inspection.Sensitivity("y", labels, 10, edges, counts, means, means, eta)


def test_sensitivity_members_and_order():
    s = _sensitivity()
    assert s.output == "y" and s.labels == ["x1", "x2", "x3"] and s.count == 10
    assert len(s.edges) == len(s.counts) == len(s.conditional_mean) == len(s.conditional_std) == 3
    assert s.first_order.shape == (3,) and s.first_order.dtype == np.float64
    assert s.order().tolist() == [1, 0, 2]  # descending, NaN last


def test_sensitivity_draw():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    s = _sensitivity()
    fig = s.draw()
    try:
        assert len(fig.axes) == 4
        top = fig.axes[0]
        assert [t.get_text() for t in top.get_yticklabels()] == ["x2", "x1", "x3"]
        assert [p.get_width() for p in top.patches][:2] == [0.7, 0.2]
        for ax, label in zip(fig.axes[1:], ["x2", "x1", "x3"]):
            (line,) = ax.lines
            assert ax.get_xlabel() == label
            assert line.get_xdata().tolist() == [0.125, 0.625, 0.875] and line.get_ydata().tolist() == [1.0, 2.0, 4.0]
        mine = plt.figure()
        assert s.draw(fig=mine) is mine and len(mine.axes) == 4
    finally:
        plt.close("all")


def test_sensitivity_draw_without_matplotlib_says_so(monkeypatch):
    monkeypatch.setitem(sys.modules, "matplotlib", None)
    monkeypatch.setitem(sys.modules, "matplotlib.pyplot", None)
    with pytest.raises(ImportError, match="needs matplotlib"):
        _sensitivity().draw()


def test_all_is_unchanged_and_the_names_are_documented():
    assert inspection.__all__ == ["summary", "quantile", "histogram", "corrcoef", "treeprint", "plot"]
    for name in ("binned_statistic", "sensitivity", "Sensitivity"):
        assert name in inspection.__doc__ and hasattr(inspection, name)


def test_new_names_import_with_no_gpu_visible():
    code = ("import probabilit_amd.inspection as i, sys; "
            "assert 'torch' not in sys.modules or not sys.modules['torch'].cuda.is_initialized(); "
            "print(callable(i.binned_statistic), callable(i.sensitivity), isinstance(i.Sensitivity, type), "
            "i.binned_finish([2], [1.0], [1.0], 1.0, 'mean').tolist(), i.correlation_ratio([1, 1], [1.0, -1.0], "
            "[1.0, 1.0]))")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="",
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["True", "True", "True", "[1.5]", "1.0"]


def test_caps_mirror_the_header():
    import re

    from probabilit_amd import native
    from probabilit_amd.correlation import MAX_VARIABLES

    text = open(os.path.join(ROOT, "include", "probabilit_hip.h")).read()
    for name in ("MAX_BINS", "MAX_COLUMNS", "MAX_PAIRS"):
        value = int(re.search(rf"#define PBH_BINNED_{name}\s+(\d+)", text).group(1))
        assert getattr(native, f"BINNED_{name}") == value
    assert native.BINNED_MAX_COLUMNS == MAX_VARIABLES + 1 and native.BINNED_MAX_PAIRS == MAX_VARIABLES
