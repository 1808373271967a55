"""inspection.histogram2d and inspection.pairgrid on sampled graphs: every answer is taken from the
device first, and only then are the samples downloaded to compare with np.histogram2d /
np.histogram, count for count and edge for edge."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from probabilit_amd import inspection, native  # noqa: E402
from probabilit_amd.modeling import Constant, Distribution, MultivariateDistribution, NoOp  # noqa: E402

N = 10_007
XE = np.array([-6.0, -1.0, 0.5, 0.5, 1.0, 2.5, 9.0])
YE = np.linspace(0.0, 12.0, 9)

# every form of (bins, range) np.histogram2d takes
FORMS = {
    "default": dict(),
    "int": dict(bins=13),
    "int_with_ranges": dict(bins=7, range=((-1.0, 3.5), (0.5, 6.0))),
    "two_ints": dict(bins=(7, 5)),
    "two_ints_one_range": dict(bins=(7, 5), range=(None, (0.0, 6.0))),
    "other_range_only": dict(bins=(3, 4), range=((-1.0, 1.0), None)),
    "one_edge_array_for_both": dict(bins=np.array([-3.0, -1.0, 0.0, 0.5, 4.0, 4.0, 11.0])),
    "two_edge_arrays": dict(bins=(XE, YE)),
    "edges_and_int": dict(bins=(XE, 6)),
    "int_and_edges": dict(bins=(6, YE), range=((-2.0, 2.0), None)),
    "empty_range_is_widened": dict(bins=4, range=((1.0, 1.0), None)),
    "the_cell_cap": dict(bins=128),
    "the_bin_cap": dict(bins=(1024, 16)),
}


def _no_download(*nodes):
    for node in nodes:
        assert node.__dict__.get("_host") is None, f"{node}: inspection downloaded the samples"


def _equal(got, want):
    (H, xe, ye), (wH, wxe, wye) = got, want
    assert H.dtype == np.int64 and H.shape == wH.shape
    assert np.array_equal(H, wH)
    assert xe.tobytes() == wxe.tobytes() and ye.tobytes() == wye.tobytes()


@pytest.fixture(scope="module")
def graph(gpu):
    """A correlated norm / gamma pair, a poisson, and a sum of them, sampled once; what inspection
    says about them, taken before any download."""
    a, b = Distribution("norm", loc=1.0, scale=2.0), Distribution("gamma", a=2.0)
    p = Distribution("poisson", mu=3.5)
    total = a + b + p
    NoOp(total).correlate(a, b, corr_mat=np.array([[1.0, 0.6], [0.6, 1.0]])).sample_device(N, random_state=7)
    nodes = dict(a=a, b=b, p=p, total=total)
    device = {"forms": {name: inspection.histogram2d(a, b, **kw) for name, kw in FORMS.items()},
              "discrete": [inspection.histogram2d(p, a, bins=(9, 6)), inspection.histogram2d(a, p),
                           inspection.histogram2d(p, total, bins=(np.arange(-0.5, 12.5), 5))],
              "grid": inspection.pairgrid(a, b, total, bins=[30, 7, 12]),
              "grid_ranges": inspection.pairgrid(a, p, bins=5, range=[(-1.0, 1.0), None])}
    _no_download(*nodes.values())
    host = {name: np.asarray(node.samples_, dtype=np.float64) for name, node in nodes.items()}
    assert abs(np.corrcoef(host["a"], host["b"])[0, 1] - 0.6) < 0.1  # (the pair is correlated)
    return nodes, device, host


@pytest.mark.parametrize("form", list(FORMS))
def test_histogram2d_forms(graph, form):
    _, device, host = graph
    _equal(device["forms"][form], np.histogram2d(host["a"], host["b"], **FORMS[form]))


def test_histogram2d_discrete_against_continuous(graph):
    _, device, host = graph
    a, p, total = host["a"], host["p"], host["total"]
    assert p.min() >= 0 and (p == np.round(p)).all()
    _equal(device["discrete"][0], np.histogram2d(p, a, bins=(9, 6)))
    _equal(device["discrete"][1], np.histogram2d(a, p))
    _equal(device["discrete"][2], np.histogram2d(p, total, bins=(np.arange(-0.5, 12.5), 5)))


def test_histogram2d_marginals_off_alignment(gpu):
    """Odd n: the second row of the parent's (2, n) block starts one double off 16-byte alignment."""
    n = 10_007
    n1, n2 = MultivariateDistribution("multivariate_normal", mean=[1, 2], cov=[[1.0, 0.9], [0.9, 1.0]])
    (n1 + n2).sample_device(n, random_state=3)
    assert n2.samples_device.data_ptr() % 16 == 8 or n1.samples_device.data_ptr() % 16 == 8
    got = inspection.histogram2d(n1, n2, bins=(11, 6))
    back = inspection.histogram2d(n2, n1, bins=(6, 11))
    grid = inspection.pairgrid(n2, n1, bins=9)
    _no_download(n1, n2, n1.distr)
    x, y = n1.samples_, n2.samples_
    _equal(got, np.histogram2d(x, y, bins=(11, 6)))
    _equal(back, np.histogram2d(y, x, bins=(6, 11)))
    assert np.array_equal(grid.joint(0, 1), np.histogram2d(y, x, bins=9)[0])


def test_pairgrid(graph):
    nodes, device, host = graph
    grid = device["grid"]
    cols, bins = [host["a"], host["b"], host["total"]], [30, 7, 12]
    assert isinstance(grid, inspection.PairGrid)
    assert grid.count == N and grid.labels == [str(nodes[k]) for k in ("a", "b", "total")]
    assert len(grid.edges) == len(grid.diagonal) == 3
    for i in range(3):
        want, want_edges = np.histogram(cols[i], bins=bins[i])
        assert grid.edges[i].tobytes() == want_edges.tobytes()
        assert grid.diagonal[i].dtype == np.int64 and np.array_equal(grid.diagonal[i], want)
        with pytest.raises(ValueError):
            grid.joint(i, i)
        for j in range(3):
            if i != j:
                H = grid.joint(i, j)
                assert H.dtype == np.int64 and H.shape == (bins[i], bins[j])
                assert np.array_equal(H, np.histogram2d(cols[i], cols[j], bins=(bins[i], bins[j]))[0])
                assert np.array_equal(grid.joint(j, i), H.T)
                assert np.array_equal(H.sum(axis=1), grid.diagonal[i])  # no range: every row is in every panel


def test_pairgrid_ranges(graph):
    _, device, host = graph
    grid = device["grid_ranges"]
    want, xe, ye = np.histogram2d(host["a"], host["p"], bins=5, range=[(-1.0, 1.0), None])
    assert np.array_equal(grid.joint(0, 1), want) and 0 < want.sum() < N
    assert grid.edges[0].tobytes() == xe.tobytes() and grid.edges[1].tobytes() == ye.tobytes()
    assert np.array_equal(grid.diagonal[0], np.histogram(host["a"], bins=5, range=(-1.0, 1.0))[0])
    assert np.array_equal(grid.diagonal[1], np.histogram(host["p"], bins=5)[0])


def test_pairgrid_of_sixteen_nodes(gpu):
    ds = [Distribution("norm", loc=0.1 * c, scale=1.0 + 0.05 * c) for c in range(16)]
    NoOp(*ds).sample_device(1001, random_state=1)
    grid = inspection.pairgrid(*ds, bins=6)
    _no_download(*ds)
    cols = [d.samples_ for d in ds]
    for i, j in ((0, 1), (0, 15), (14, 15), (7, 3)):
        assert np.array_equal(grid.joint(i, j), np.histogram2d(cols[i], cols[j], bins=6)[0])


def test_value_errors(graph):
    nodes, _, _ = graph
    a, b = nodes["a"], nodes["b"]
    c = Constant(2.5)
    (c + Distribution("norm")).sample_device(N, random_state=0)
    d1, d2 = MultivariateDistribution("multivariate_normal", mean=[1, 2], cov=np.eye(2))
    (d1 + d2).sample_device(N, random_state=0)
    short = Distribution("norm")
    short.sample_device(N - 1, random_state=0)
    nan = Distribution("norm")
    x = np.random.default_rng(0).standard_normal(N)
    x[17] = np.nan
    from probabilit_amd import device

    nan._set_device(device.to_device(x))
    for bad in (c, d1.distr):
        with pytest.raises(ValueError, match="one sample vector"):
            inspection.histogram2d(a, bad)
        with pytest.raises(ValueError, match="one sample vector"):
            inspection.pairgrid(bad, a)
    with pytest.raises(ValueError, match="different numbers"):
        inspection.histogram2d(a, short)
    with pytest.raises(ValueError, match="different numbers"):
        inspection.pairgrid(a, b, short)
    with pytest.raises(ValueError, match="2 to 16 nodes"):
        inspection.pairgrid(a)
    with pytest.raises(ValueError, match="2 to 16 nodes"):
        inspection.pairgrid(*[a, b] * 8, a)
    with pytest.raises(ValueError, match="monotonically increasing"):
        inspection.histogram2d(a, b, bins=([0.0, 2.0, 1.0], 5))
    with pytest.raises(ValueError, match="monotonically increasing"):
        np.histogram2d(x, x, bins=([0.0, 2.0, 1.0], 5))
    with pytest.raises(ValueError, match=r"autodetected range of \[nan, nan\] is not finite"):
        inspection.histogram2d(a, nan)
    with pytest.raises(ValueError, match=r"autodetected range of \[nan, nan\] is not finite"):
        np.histogram2d(x, x)
    with pytest.raises(ValueError, match="autodetected range"):
        inspection.pairgrid(nan, a)
    # with a range or edges for the axis the NaN row is dropped, as numpy drops it
    _equal(inspection.histogram2d(a, nan, bins=(4, XE)),
           np.histogram2d(a.samples_, x, bins=(4, XE)))
    _equal(inspection.histogram2d(nan, nan, bins=3, range=((-1, 1), (-2, 2))),
           np.histogram2d(x, x, bins=3, range=((-1, 1), (-2, 2))))


def test_caps_are_named(graph):
    nodes, _, _ = graph
    a, b = nodes["a"], nodes["b"]
    with pytest.raises(NotImplementedError, match=str(native.HISTOGRAM2D_MAX_BINS)):
        inspection.histogram2d(a, b, bins=(1025, 1))
    with pytest.raises(NotImplementedError, match=str(native.HISTOGRAM2D_MAX_BINS)):
        inspection.histogram2d(a, b, bins=(2, np.arange(1026.0)))
    with pytest.raises(NotImplementedError, match=str(native.HISTOGRAM2D_MAX_CELLS)):
        inspection.histogram2d(a, b, bins=(129, 128))
    with pytest.raises(NotImplementedError, match=str(native.HISTOGRAM2D_MAX_CELLS)):
        inspection.pairgrid(a, b, bins=[128, 129])
    with pytest.raises(NotImplementedError, match=str(native.HISTOGRAM2D_MAX_BINS)):
        inspection.pairgrid(a, b, bins=[1, 1025])
