"""inspection.binned_statistic and inspection.sensitivity on sampled graphs: every answer is taken
from the device first, and only then are the samples downloaded to compare with
scipy.stats.binned_statistic and with the correlation ratio in exact arithmetic.

Tolerances.  Counts and edges are exact.  A floating-point statistic is compared within
  finish_bounds(...)[statistic] + reference_allowance(...)            (tests/binned_reference.py):
the first is the bound stated beside pbh_binned_sums in include/probabilit_hip.h (m u sum |y - c| on
s1, (m + 2) u sum (y - c)^2 on s2, for the m rows of a bin about the centre c the device used, the
column's pbh_moments mean) carried through binned_finish's few operations to first order, the second
what scipy's own serial sum / pairwise std may be off by.  eta^2 is compared with the exact rational
value within correlation_ratio_bound, the same two bounds carried through correlation_ratio."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from binned_reference import (U, correlation_ratio_bound, exact_correlation_ratio, finish_bounds,  # noqa: E402
                              raw_sums, reference_allowance)

from probabilit_amd import inspection  # noqa: E402
from probabilit_amd.modeling import Constant, Distribution, MultivariateDistribution, NoOp  # noqa: E402

N = 100_003
STATISTICS = ("count", "sum", "mean", "std")
XE = np.array([-6.0, -1.0, 0.5, 0.75, 1.0, 2.5, 9.0])
FORMS = {
    "default": dict(),
    "int": dict(bins=13),
    "int_with_range": dict(bins=13, range=(-1.0, 3.5)),
    "edges": dict(bins=XE),
    "edges_beside_a_range": dict(bins=XE, range=(0.0, 1.0)),  # (the range is ignored, as scipy does)
    "empty_range_is_widened": dict(bins=4, range=(1.0, 1.0)),
    "the_bin_cap": dict(bins=1024),
}


def _no_download(*nodes):
    for node in nodes:
        assert node.__dict__.get("_host") is None, f"{node}: inspection downloaded the samples"


def _constant_valued(n):
    """A node whose n samples are all 2.5 (a vector on the device, not a Constant)."""
    from probabilit_amd import device

    node = Distribution("norm")
    node._set_device(device.to_device(np.full(n, 2.5)))
    return node


def _against_scipy(got, x, y, statistic, centre, bins=10, range=None):
    import scipy.stats

    stat, edges = got
    want, wedges, _ = scipy.stats.binned_statistic(x, y, statistic, bins=bins, range=range)
    # scipy alone also takes a value just above the last edge, equal to it after rounding to `decimal`
    # digits, into the last bin: the data must hold none for scipy to agree with numpy
    decimal = int(-np.log10(np.diff(wedges).min())) + 6
    assert not ((x > wedges[-1]) & (np.around(x, decimal) == np.around(wedges[-1], decimal))).any()
    assert np.asarray(edges).tobytes() == wedges.tobytes()
    assert stat.dtype == np.float64 and stat.shape == want.shape
    assert np.array_equal(np.isnan(stat), np.isnan(want))
    if statistic == "count":
        assert np.array_equal(stat, want)
        return
    count, s1, s2, a1 = raw_sums(x, y, wedges, centre)
    tol = finish_bounds(count, s1, s2, a1, centre)[statistic] + reference_allowance(x, y, wedges, statistic)
    has = count > 0
    err = np.abs(stat - want)[has]
    print(statistic, "largest error", err.max(initial=0.0), "its bound", tol[has][err.argmax()] if len(err) else None)
    assert (err <= tol[has]).all()


@pytest.fixture(scope="module")
def graph(gpu):
    """A norm, a gamma, a poisson (int64), a comparison (bool), a constant-valued vector and a
    non-linear output, sampled once; what inspection says, taken before any download."""
    a, b = Distribution("norm", loc=1.0, scale=2.0), Distribution("gamma", a=2.0)
    p = Distribution("poisson", mu=3.5)
    comp = a > p
    total = a + b * b + p
    NoOp(total, comp).sample_device(N, random_state=7)
    flat = _constant_valued(N)
    nodes = dict(a=a, b=b, p=p, comp=comp, flat=flat, total=total)
    means = {k: inspection.summary(v)["mean"] for k, v in nodes.items()}
    bs = inspection.binned_statistic
    device = {
        "forms": {(f, s): bs(a, total, s, **kw) for f, kw in FORMS.items() for s in STATISTICS},
        "list": {s: bs(a, [total, b, p], s, bins=7) for s in STATISTICS},
        "one_in_a_list": bs(a, [total], "mean", bins=7),
        "discrete": {(f, s): bs(p, total, s, bins=bins) for f, bins in (("int", 9), ("edges", np.arange(0.0, 14.0)))
                     for s in STATISTICS},
        "cast": {s: bs(comp, p, s, bins=2) for s in STATISTICS},
        "flat": {s: bs(flat, total, s, bins=4) for s in STATISTICS},
        "self": bs(a, a, "mean", bins=11),
    }
    _no_download(*nodes.values())
    host = {name: np.asarray(node.samples_, dtype=np.float64) for name, node in nodes.items() if name != "flat"}
    host["flat"] = np.full(N, 2.5)
    return nodes, device, host, means


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("form", list(FORMS))
def test_binned_statistic_forms(graph, form, statistic):
    _, device, host, means = graph
    centre = 0.0 if statistic == "count" else means["total"]
    _against_scipy(device["forms"][(form, statistic)], host["a"], host["total"], statistic, centre, **FORMS[form])


@pytest.mark.parametrize("statistic", STATISTICS)
def test_binned_statistic_of_a_list_of_nodes(graph, statistic):
    import scipy.stats

    _, device, host, means = graph
    stat, edges = device["list"][statistic]
    want = scipy.stats.binned_statistic(host["a"], [host["total"], host["b"], host["p"]], statistic, bins=7)[0]
    assert stat.shape == want.shape == (3, 7)
    for row, name in enumerate(("total", "b", "p")):
        centre = 0.0 if statistic == "count" else means[name]
        _against_scipy((stat[row], edges), host["a"], host[name], statistic, centre, bins=7)
    one, _ = device["one_in_a_list"]
    assert one.shape == (1, 7)


@pytest.mark.parametrize("statistic", STATISTICS)
@pytest.mark.parametrize("form", ["int", "edges"])
def test_binned_statistic_by_a_discrete_node(graph, form, statistic):
    """poisson: every sample is an integer, many of them on an edge."""
    _, device, host, means = graph
    p = host["p"]
    bins = 9 if form == "int" else np.arange(0.0, 14.0)  # (integer edges: every sample below 14 is on one)
    assert (p == np.round(p)).all() and p.min() == 0.0
    _against_scipy(device["discrete"][(form, statistic)], p, host["total"], statistic,
                   0.0 if statistic == "count" else means["total"], bins=bins)


@pytest.mark.parametrize("statistic", STATISTICS)
def test_binned_statistic_of_bool_and_int64_nodes(graph, statistic):
    nodes, device, host, means = graph
    assert set(np.unique(host["comp"])) == {0.0, 1.0}
    _against_scipy(device["cast"][statistic], host["comp"], host["p"], statistic,
                   0.0 if statistic == "count" else means["p"], bins=2)


@pytest.mark.parametrize("statistic", STATISTICS)
def test_binned_statistic_by_a_constant_valued_node(graph, statistic):
    """Every sample is 2.5: the range is widened to [2, 3] as numpy and scipy widen it."""
    _, device, host, means = graph
    assert (host["flat"] == 2.5).all()
    stat, edges = device["flat"][statistic]
    assert edges.tolist() == [2.0, 2.25, 2.5, 2.75, 3.0]
    centre = 0.0 if statistic == "count" else means["total"]
    _against_scipy((stat, edges), host["flat"], host["total"], statistic, centre, bins=4)


def test_binned_statistic_of_a_node_by_itself(graph):
    _, device, host, means = graph
    _against_scipy(device["self"], host["a"], host["a"], "mean", means["a"], bins=11)


# ---------------------------------------------------------------- sensitivity
NS = 20_011


@pytest.fixture(scope="module")
def sens(gpu):
    a, b = Distribution("norm", loc=1.0, scale=2.0), Distribution("gamma", a=2.0)
    p = Distribution("poisson", mu=3.5)
    total = a + b * b + p
    total.sample_device(NS, random_state=11)
    flat = _constant_valued(NS)
    centre = inspection.summary(total)["mean"]
    got = {binning: inspection.sensitivity(total, a, b, p, flat, bins=32, binning=binning)
           for binning in ("quantile", "uniform")}
    one = inspection.sensitivity(total, b, bins=1)
    _no_download(a, b, p, flat, total)
    host = [np.asarray(node.samples_, dtype=np.float64) for node in (total, a, b, p)] + [np.full(NS, 2.5)]
    return (total, a, b, p, flat), got, one, host, centre


@pytest.mark.parametrize("binning", ["quantile", "uniform"])
def test_sensitivity_against_the_downloaded_columns(sens, binning):
    nodes, got, _, host, centre = sens
    s = got[binning]
    y = host[0]
    assert isinstance(s, inspection.Sensitivity) and s.count == NS
    assert s.labels == [str(node) for node in nodes[1:]] and s.output == str(nodes[0])
    assert s.first_order.shape == (4,)
    for k, x in enumerate(host[1:]):
        e = s.edges[k]
        if binning == "quantile":
            want_e = np.quantile(x, np.arange(33) / 32, method="nearest")
            if want_e[0] == want_e[-1]:
                want_e[0], want_e[-1] = want_e[0] - 0.5, want_e[-1] + 0.5
        else:
            want_e = np.histogram_bin_edges(x, bins=32)
        assert e.tobytes() == want_e.tobytes()
        assert s.counts[k].dtype == np.int64 and np.array_equal(s.counts[k], np.histogram(x, e)[0])
        assert s.counts[k].sum() == NS
        count, s1, s2, a1 = raw_sums(x, y, e, centre)
        bounds = finish_bounds(count, s1, s2, a1, centre)
        has = count > 0
        for name, field in (("mean", s.conditional_mean[k]), ("std", s.conditional_std[k])):
            want = inspection.binned_finish(count, s1, s2, centre, name)
            assert np.isnan(field[~has]).all() and (np.abs(field - want)[has] <= bounds[name][has]).all()
        if k == 3:  # the constant-valued input: one bin holds every row, which explains nothing
            assert (s.counts[k] > 0).sum() == 1 and s.first_order[k] == 0.0
            assert e[0] == 2.0 and e[-1] == 3.0
            continue
        want = exact_correlation_ratio(x, y, e)
        bound = correlation_ratio_bound(count, s1, s2, a1) + U
        print(binning, k, "eta2", s.first_order[k], "error", abs(s.first_order[k] - want), "bound", bound)
        assert abs(s.first_order[k] - want) <= bound and 0.0 < want < 1.0
    if binning == "quantile":  # the discrete input has ties: repeated edges, empty bins
        assert (np.diff(s.edges[2]) == 0).any() and (s.counts[2] == 0).any()
        assert np.abs(s.counts[0] - NS / 32).max() <= 2.0  # the continuous one: equal probability


def test_sensitivity_with_one_bin_explains_nothing(sens):
    _, _, one, host, _ = sens
    assert one.first_order.tolist() == [0.0] and one.counts[0].tolist() == [NS]
    assert one.edges[0].tolist() == [host[2].min(), host[2].max()]


@pytest.fixture(scope="module")
def normals(gpu):
    """Independent standard normals x1, x2, x3; a pair u1, u2 correlated 0.8."""
    x1, x2, x3, u1, u2 = (Distribution("norm") for _ in range(5))
    lin = x1 + 2 * x2 + 0 * x3
    prod = x1 * x2
    cprod = u1 * u2
    root = NoOp(lin, prod, cprod).correlate(u1, u2, corr_mat=np.array([[1.0, 0.8], [0.8, 1.0]]))
    root.sample_device(N, random_state=3)
    return dict(x1=x1, x2=x2, x3=x3, u1=u1, u2=u2, lin=lin, prod=prod, cprod=cprod)


@pytest.mark.parametrize("binning", ["quantile", "uniform"])
def test_ordering_of_a_linear_output(normals, binning):
    """y = x1 + 2 x2 + 0 x3: the shares are 1/5, 4/5 and 0."""
    g = normals
    s = inspection.sensitivity(g["lin"], g["x1"], g["x2"], g["x3"], binning=binning)
    e1, e2, e3 = s.first_order
    assert e2 > e1 > e3 >= 0.0 and s.order().tolist() == [1, 0, 2]
    assert abs(e1 - 0.2) < 0.02 and abs(e2 - 0.8) < 0.02 and e3 < 0.01  # (bins / N = 3e-4 of noise)
    _no_download(*g.values())


def test_a_product_that_corrcoef_does_not_see(normals):
    """y = u1 u2 with centred inputs correlated 0.8: E[y | u1] = 0.8 u1^2, so each input owns
    2 * 0.64 / (1 + 0.64) = 0.78 of the variance while its correlation with y is 0 by symmetry.
    (With independent centred inputs E[y | x1] = x1 E[x2] = 0: the product is then pure interaction,
    which no first-order measure sees either; that case is asserted as such.)"""
    g = normals
    corr = inspection.corrcoef(g["cprod"], g["u1"], g["u2"])
    assert abs(corr[0, 1]) < 0.05 and abs(corr[0, 2]) < 0.05 and corr[1, 2] > 0.7
    s = inspection.sensitivity(g["cprod"], g["u1"], g["u2"])
    # (0.78 is the share of the continuous E[y | u]; a bin's mean smooths u^2 within the bin, most in
    # the wide outer bins, so the binned estimate lies below it, up to bins / N = 3e-4 of noise)
    assert (s.first_order > 0.05).all() and (s.first_order < 0.78 + 0.01).all()
    corr = inspection.corrcoef(g["prod"], g["x1"], g["x2"])
    s = inspection.sensitivity(g["prod"], g["x1"], g["x2"])
    assert abs(corr[0, 1]) < 0.05 and abs(corr[0, 2]) < 0.05 and (s.first_order < 0.01).all()
    _no_download(*g.values())


def test_refused_nodes(graph):
    nodes, _, _, _ = graph
    a, total = nodes["a"], nodes["total"]
    c = Constant(2.5)
    (c + Distribution("norm")).sample_device(N, random_state=0)
    d1, d2 = MultivariateDistribution("multivariate_normal", mean=[1, 2], cov=np.eye(2))
    (d1 + d2).sample_device(N, random_state=0)
    short = Distribution("norm")
    short.sample_device(N - 1, random_state=0)
    for bad in (c, d1.distr):
        for call in (lambda: inspection.binned_statistic(a, bad), lambda: inspection.binned_statistic(bad, a),
                     lambda: inspection.binned_statistic(a, [total, bad]), lambda: inspection.sensitivity(total, bad),
                     lambda: inspection.sensitivity(bad, a)):
            with pytest.raises(ValueError, match="one sample vector"):
                call()
    with pytest.raises(ValueError, match="different numbers"):
        inspection.binned_statistic(a, short)
    with pytest.raises(ValueError, match="different numbers"):
        inspection.sensitivity(total, a, short)
    with pytest.raises(NotImplementedError, match="1024"):
        inspection.binned_statistic(a, total, bins=1025)
    with pytest.raises(ValueError, match="monotonically increasing"):
        inspection.binned_statistic(a, total, bins=[0.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="at least two edges"):
        inspection.binned_statistic(a, total, bins=[1.0])
    with pytest.raises(ValueError, match="supplied range of"):
        inspection.binned_statistic(a, total, range=(0.0, np.inf))
    with pytest.raises(ValueError, match="max must be larger than min"):
        inspection.binned_statistic(a, total, range=(1.0, 0.0))


def test_a_nan_among_the_samples(graph):
    """A NaN in x: no range can be found (ValueError, as numpy says it); with edges the row is
    dropped.  A NaN in the values reaches its bin's sum, mean and std only."""
    from probabilit_amd import device

    nodes, _, host, _ = graph
    x = host["a"].copy()
    x[17] = np.nan
    nan = Distribution("norm")
    nan._set_device(device.to_device(x))
    with pytest.raises(ValueError, match=r"autodetected range of \[nan, nan\] is not finite"):
        inspection.binned_statistic(nan, nodes["total"])
    with pytest.raises(ValueError, match="not finite"):
        inspection.sensitivity(nodes["total"], nan)
    with pytest.raises(ValueError, match="not finite"):
        inspection.sensitivity(nodes["total"], nan, binning="uniform")
    count, _ = inspection.binned_statistic(nan, nodes["total"], "count", bins=XE)
    assert np.array_equal(count, np.histogram(x[~np.isnan(x)], XE)[0])
    mean, _ = inspection.binned_statistic(nodes["a"], nan, "mean", bins=XE)
    hit = np.searchsorted(XE, host["a"][17], "right") - 1
    assert np.isnan(mean[hit]) and np.isfinite(np.delete(mean, hit)).all()


def test_draw(sens):
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    _, got, _, _, _ = sens
    s = got["quantile"]
    fig = s.draw()
    try:
        assert len(fig.axes) == 5
        order = s.order().tolist()
        assert [t.get_text() for t in fig.axes[0].get_yticklabels()] == [s.labels[i] for i in order]
        assert [p.get_width() for p in fig.axes[0].patches] == s.first_order[order].tolist()
        for ax, i in zip(fig.axes[1:], order):
            (line,) = ax.lines
            assert len(line.get_xdata()) == (s.counts[i] > 0).sum()
    finally:
        plt.close("all")
