"""probabilit_amd.inspection on sampled graphs: every answer is taken from the device first, and
only then are the samples downloaded to compare with numpy / scipy."""

import json
import os
import socket
import tempfile

import numpy as np
import pytest
import scipy.stats

from summary_reference import check_moments

pytestmark = pytest.mark.gpu

from probabilit_amd import correlation, inspection  # noqa: E402
from probabilit_amd.modeling import Constant, Distribution, MultivariateDistribution, NoOp  # noqa: E402

N = 100_003
METHODS = ["linear", "lower", "higher", "nearest", "midpoint"]
QS = np.array([0.0, 1.0, 0.5, 1 / 3, 1e-9])


@pytest.fixture(scope="module")
def graph(gpu):
    """One sampled graph: a norm, a poisson, a comparison of the two (bool) and a dirichlet parent,
    with what inspection says about each, taken before any download."""
    norm = Distribution("norm", loc=1.0, scale=2.0)
    pois = Distribution("poisson", mu=3.5)
    comp = norm > pois
    d1, d2, d3 = MultivariateDistribution("dirichlet", alpha=[0.5, 2.5, 7.0])
    NoOp(norm, pois, comp, d1 + d2 + d3).sample_device(N, random_state=7)
    nodes = {"norm": norm, "poisson": pois, "comparison": comp, "dirichlet": d1.distr}
    device = {}
    for name, node in nodes.items():
        device[name] = {
            "summary": inspection.summary(node),
            "quantile": {m: inspection.quantile(node, QS, method=m) for m in METHODS},
            "histogram": inspection.histogram(node, bins=37),
            "histogram_range": inspection.histogram(node, bins=1000, range=(0.1, 0.7)),
        }
        assert node.__dict__.get("_host") is None, f"{name}: inspection downloaded the samples"
    host = {name: np.asarray(node.samples_, dtype=np.float64) for name, node in nodes.items()}
    return nodes, device, host


def _columns(name, host, dev):
    """(samples, device answer) per component: the dirichlet parent has three."""
    if name != "dirichlet":
        return [(host, dev)]
    return [(np.ascontiguousarray(host[:, c]), dev[c]) for c in range(host.shape[1])]


NAMES = ["norm", "poisson", "comparison", "dirichlet"]


@pytest.mark.parametrize("name", NAMES)
def test_summary(graph, name):
    _, device, host = graph
    for x, s in _columns(name, host[name], device[name]["summary"]):
        assert isinstance(s, dict) and s["count"] == N and s["nan"] == 0
        assert s["min"] == x.min() and s["max"] == x.max()
        # the moments behind std / skew / kurtosis, within the kernel's a-priori bound
        from probabilit_amd import native

        k = dict(zip(native.MOMENT_FIELDS, native.moments(_device_column(graph, name, x))[0]))
        assert k["mean"] == s["mean"] and np.sqrt(k["m2"]) == s["std"]
        check_moments(x, k, name)
        # against numpy / scipy, whose own pairwise sums carry errors of the same order: both sides'
        # a-priori bounds are below 50 eps relative to mean(|x - mean|^p) here, i.e. 1e-14
        np.testing.assert_allclose(s["mean"], np.mean(x), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(s["std"], np.std(x), rtol=1e-12)
        np.testing.assert_allclose(s["std_ddof1"], np.std(x, ddof=1), rtol=1e-12)
        np.testing.assert_allclose(s["skew"], scipy.stats.skew(x), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(s["kurtosis"], scipy.stats.kurtosis(x), rtol=1e-10, atol=1e-12)
        assert list(s["quantiles"]) == [0.1, 0.5, 0.9]
        assert list(s["quantiles"].values()) == np.quantile(x, [0.1, 0.5, 0.9]).tolist()


def _device_column(graph, name, x):
    """The float64 device vector whose download is x (uploaded again: the comparison is of the
    kernel's sums with the exact ones, on the same values)."""
    from probabilit_amd import device

    return device.to_device(np.ascontiguousarray(x))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", NAMES)
def test_quantile_bit_equal(graph, name, method):
    _, device, host = graph
    got = device[name]["quantile"][method]
    if name == "dirichlet":
        want = np.quantile(host[name], QS, axis=0, method=method)
    else:
        want = np.quantile(host[name], QS, method=method)
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", NAMES)
def test_histogram_counts(graph, name):
    _, device, host = graph
    for key, kw in (("histogram", dict(bins=37)), ("histogram_range", dict(bins=1000, range=(0.1, 0.7)))):
        for x, (counts, edges) in _columns(name, host[name], device[name][key]):
            want, want_edges = np.histogram(x, **kw)
            np.testing.assert_array_equal(edges, want_edges)
            np.testing.assert_array_equal(counts, want)
            assert counts.dtype == np.int64


def test_scalar_quantile_and_many_quantiles(graph):
    nodes, _, host = graph
    assert inspection.quantile(nodes["norm"], 0.25) == np.quantile(host["norm"], 0.25)
    q = np.linspace(0.0, 1.0, 77).reshape(7, 11)  # more than one select
    np.testing.assert_array_equal(inspection.quantile(nodes["norm"], q), np.quantile(host["norm"], q))
    with pytest.raises(ValueError):
        inspection.quantile(nodes["norm"], 1.5)


def test_nan_samples_make_every_quantile_nan(gpu):
    node = Distribution("norm")
    x = np.random.default_rng(0).standard_normal(1000)
    x[17] = np.nan
    from probabilit_amd import device

    node._set_device(device.to_device(x))
    for m in METHODS:
        assert np.isnan(inspection.quantile(node, QS, method=m)).all() and np.isnan(np.quantile(x, QS, method=m)).all()
    assert inspection.summary(node)["nan"] == 1
    with pytest.raises(ValueError, match="finite"):
        inspection.histogram(node)
    counts, _ = inspection.histogram(node, bins=5, range=(-1, 1))
    np.testing.assert_array_equal(counts, np.histogram(x, bins=5, range=(-1, 1))[0])


def test_constant_is_answered_on_the_host(gpu):
    c = Constant(2.5)
    (c + Distribution("norm")).sample_device(100, random_state=0)
    s = inspection.summary(c)
    assert s["count"] == 100 and s["mean"] == 2.5 and s["std"] == 0.0 and s["min"] == s["max"] == 2.5
    assert inspection.quantile(c, 0.3) == 2.5
    counts, edges = inspection.histogram(c, bins=4)
    want, want_edges = np.histogram(np.full(100, 2.5), bins=4)
    np.testing.assert_array_equal(counts, want)
    np.testing.assert_array_equal(edges, want_edges)
    assert c.__dict__.get("_host") is None


@pytest.mark.parametrize("kind", ["pearson", "spearman"])
def test_corrcoef(graph, kind):
    nodes, _, host = graph
    d = nodes["dirichlet"]
    picks = [nodes["norm"], nodes["poisson"], nodes["comparison"]]
    got = inspection.corrcoef(*picks, kind=kind)
    X = np.vstack([host["norm"], host["poisson"], host["comparison"]])
    want = np.corrcoef(X) if kind == "pearson" else scipy.stats.spearmanr(X.T).statistic
    assert got.shape == (3, 3)
    assert np.abs(got - want).max() <= 1e-12
    with pytest.raises(ValueError, match="one sample vector"):
        inspection.corrcoef(nodes["norm"], d)


def test_refusals(graph):
    nodes, _, _ = graph
    norm = nodes["norm"]
    with pytest.raises(AttributeError, match="samples_"):
        inspection.summary(Distribution("norm"))
    with pytest.raises(ValueError, match=str(correlation.MAX_VARIABLES)):
        inspection.corrcoef(*[norm] * (correlation.MAX_VARIABLES + 1))
    with pytest.raises(NotImplementedError, match="edges"):
        inspection.histogram(norm, bins=[0.0, 0.5, 1.0])


_CALLS = {"summary": inspection.summary, "quantile": lambda nd: inspection.quantile(nd, 0.5),
          "histogram": inspection.histogram, "corrcoef": inspection.corrcoef}
_SHARD_N = 1 << 12


def _sharded_graph():
    a, b = Distribution("norm", loc=1.0, scale=2.0), Distribution("poisson", mu=3.5)
    return {"norm": a, "poisson": b, "sum": a + b}


def _sharded_worker(rank, world, port, outdir):
    """One of two gloo ranks on the one GPU: samples a graph with group=, asks inspection about
    every node, samples the same nodes again without a group and asks again; what happened goes
    to a JSON file per rank."""
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        nodes = _sharded_graph()
        out = nodes["sum"].sample_device(_SHARD_N, random_state=7, group=dist.group.WORLD)
        seen = {"rows": int(out.shape[0]), "sharded": {}, "again": {}}
        for name, node in nodes.items():
            for what, call in _CALLS.items():
                try:
                    call(node)
                    seen["sharded"][f"{name}.{what}"] = "returned"
                except NotImplementedError as e:
                    seen["sharded"][f"{name}.{what}"] = str(e)
        nodes["sum"].sample_device(_SHARD_N, random_state=7)  # the same nodes, whole again
        for name, node in nodes.items():
            seen["again"][name] = [inspection.summary(node)["count"], float(inspection.quantile(node, 0.5)),
                                   int(inspection.histogram(node)[0].sum()), inspection.corrcoef(node).tolist()]
        with open(os.path.join(outdir, f"seen{rank}.json"), "w") as f:
            json.dump(seen, f)
    finally:
        dist.destroy_process_group()


def test_group_sharded_samples_are_refused(gpu):
    """Node.sample_device(..., group=) over two ranks leaves this rank's rows on every node:
    summary / quantile / histogram / corrcoef refuse each of them, naming the sharding, and answer
    again once the same nodes were sampled without a group."""
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_sharded_worker, args=(2, port, d), nprocs=2, join=True, start_method="spawn")
        seen = []
        for r in range(2):
            with open(os.path.join(d, f"seen{r}.json")) as f:
                seen.append(json.load(f))
    ref = _sharded_graph()
    ref["sum"].sample_device(_SHARD_N, random_state=7)
    for r, s in enumerate(seen):
        assert s["rows"] == _SHARD_N // 2  # the ranks did hold shards
        assert len(s["sharded"]) == 12
        for key, msg in s["sharded"].items():
            assert "row-sharded" in msg and f"rank {r} of 2" in msg, (r, key, msg)
        for name, node in ref.items():
            count, median, total, corr = s["again"][name]
            assert count == _SHARD_N and total == _SHARD_N and abs(corr[0][0] - 1.0) <= 1e-12
            assert median == inspection.quantile(node, 0.5)
