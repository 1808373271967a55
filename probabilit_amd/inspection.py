"""Inspecting sampled nodes where their samples are: on the device.

The reference's workflow ends in np.mean(node.samples_), np.percentile(node.samples_, ...), a
histogram or a look at the achieved correlation.  Here every `.samples_` access is a download of
the whole vector; the functions of this module answer the same questions from the device
vector with a few kernel sweeps (pbh_moments, pbh_select_ranks, pbh_histogram and the K x K
statistics Iman-Conover already uses) and bring back a handful of numbers.  None of them
populates `node.samples_`.

    summary(*nodes, quantiles=(0.1, 0.5, 0.9))    count / nan / mean / std / min / max / skew / ...
    quantile(node, q, method="linear")            np.quantile(node.samples_, q, method=method)
    histogram(node, bins=10, range=None)          np.histogram(node.samples_, bins, range)
    corrcoef(*nodes, kind="pearson")              np.corrcoef / scipy.stats.spearmanr of the nodes
    treeprint(node)                               the graph above a node, one line per node
    plot(...)                                     probabilit_amd.plot (not provided)

Limits: histograms take an integer number of at most 4096 uniform bins; quantile methods are
linear, lower, higher, nearest and midpoint; samples row-sharded over a process group
(`sample_device(group=...)` with more than one rank) are not summarised across ranks.
"""

import numpy as np

__all__ = ["summary", "quantile", "histogram", "corrcoef", "treeprint", "plot"]

QUANTILE_METHODS = ("linear", "lower", "higher", "nearest", "midpoint")


# =============================================================================
# host pieces (no device call)
# =============================================================================
def quantile_indexes(n, q, method="linear"):
    """numpy's (previous index, next index, gamma) of np.quantile over n sorted values
    (lib/_function_base_impl.py _quantile: the method's virtual index, _get_indexes' clamping with
    -1 for the last element, _get_gamma); gamma is None for the methods that take one element as
    it is.  q: a float64 array of probabilities in [0, 1]."""
    if method not in QUANTILE_METHODS:
        raise ValueError(f"method {method!r} is not one of {QUANTILE_METHODS}")
    q = np.asarray(q, dtype=np.float64)
    if not np.all((q >= 0.0) & (q <= 1.0)):  # (a NaN fails it too)
        raise ValueError("Quantiles must be in the range [0, 1]")
    vi = (n - 1) * q
    if method in ("lower", "higher", "nearest"):
        idx = {"lower": np.floor, "higher": np.ceil, "nearest": np.around}[method](vi).astype(np.intp)
        return idx, idx, None  # numpy takes arr[idx] itself: no interpolation
    if method == "midpoint":
        vi = 0.5 * (np.floor(vi) + np.ceil(vi))
    prev = np.asarray(np.floor(vi))
    nxt = np.asarray(prev + 1)
    above = vi >= n - 1
    prev[above] = -1
    nxt[above] = -1
    gamma = np.asarray(vi - prev)
    if method == "midpoint":
        gamma = np.where(vi % 1 == 0, 0.0, 0.5)
    return prev.astype(np.intp), nxt.astype(np.intp), gamma


def lerp(a, b, t):
    """numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5 (t None: a as it is)."""
    if t is None:
        return np.asarray(a, dtype=np.float64)
    a, b, t = (np.asarray(v, dtype=np.float64) for v in (a, b, t))
    with np.errstate(invalid="ignore"):
        diff = b - a
        out = np.asarray(a + diff * t)
        hi = np.asarray(b - diff * (1 - t))
    return np.where(t >= 0.5, hi, out)


def quantile_of_sorted(values, q, method="linear"):
    """np.quantile(values, q, method=method) for an ascending float64 array (NaN last): the host
    half of `quantile`, which takes values[i] from the device instead."""
    values = np.asarray(values, dtype=np.float64)
    prev, nxt, gamma = quantile_indexes(len(values), q, method)
    if np.isnan(values[-1]):
        return np.full(np.shape(q), np.nan)[()]
    return lerp(values[prev], values[nxt], gamma)[()]


def _skew_kurtosis(mean, m2, m3, m4):
    """scipy.stats.skew / kurtosis (bias=True, fisher=True) from the central moments, NaN where
    scipy finds the data constant (m2 <= (eps mean)^2)."""
    with np.errstate(all="ignore"):
        zero = m2 <= (np.finfo(np.float64).resolution * mean) ** 2
        skew = np.nan if zero else m3 / m2 ** 1.5
        kurt = np.nan if zero else m4 / m2 ** 2.0 - 3.0
    return float(skew), float(kurt)


def treeprint(node):
    """Print the graph above `node`, one line per node: a Transform by its class name, anything
    else by str(node)."""
    from .modeling import Transform

    def label(nd):
        return type(nd).__name__ if isinstance(nd, Transform) else str(nd)

    def walk(nd, indent):
        parents = list(nd.get_parents())
        for i, p in enumerate(parents):
            last = i == len(parents) - 1
            print(indent + ("└──" if last else "├──") + label(p))
            walk(p, indent + ("   " if last else "│  "))

    print(label(node))
    walk(node, "")


def plot(*variables, **kwargs):
    """probabilit.inspection.plot: forwarded to probabilit_amd.plot, which does not provide it."""
    from . import plot as _plot

    return _plot(*variables, **kwargs)


# =============================================================================
# the device vectors behind nodes
# =============================================================================
class _Scalar:
    """A Constant's samples: n copies of one value, answered on the host."""

    def __init__(self, value, n):
        self.value, self.n = float(value), int(n)

    def host(self):
        return np.array([self.value])


def _samples(node):
    """The node's samples as a float64 device vector, a (d, n) block (multivariate parent) or a
    _Scalar; never a download."""
    from . import modeling

    d = node.__dict__
    if "_smp" not in d:
        raise AttributeError(f"'{type(node).__name__}' object has no attribute 'samples_'")
    if d.get("_shard") is not None:
        rank, world = d["_shard"]
        raise NotImplementedError(f"{node}: its samples are row-sharded over a process group (group=, rank {rank} "
                                  f"of {world}); summaries across ranks are not provided")
    dev = node._dev()  # (a DiscreteDistribution of labels raises TypeError here)
    if dev is None:
        raise ValueError(f"{node} holds no samples")
    if isinstance(dev, modeling._Broadcast):
        return _Scalar(dev.value, dev.n)
    f64 = np.dtype(np.float64)
    if modeling._dtype_of(dev) != f64:  # int64 / bool: the cast kernel
        flat = dev.reshape(-1) if dev.is_contiguous() else dev.contiguous().reshape(-1)
        dev = modeling._elementwise("cast", flat, None, flat.shape[0], f64, f64, None).reshape(dev.shape)
    if dev.dim() == 1 and not dev.is_contiguous():
        dev = dev.contiguous()
    return dev


def _per_component(x, fn):
    """fn(column) for a vector, or the list over the rows of a (d, n) block."""
    if isinstance(x, _Scalar) or x.dim() == 1:
        return fn(x)
    return [fn(x[c]) for c in range(x.shape[0])]


# =============================================================================
# quantiles
# =============================================================================
def _select(x, ranks):
    """{rank: np.sort(x)[rank]} for any number of ranks, and whether x holds a NaN (rank n - 1 is
    one; asked once per column): the distinct ranks, 64 per device call, so more than 32 quantiles
    take several selects."""
    from . import native

    n = x.shape[0]
    want = np.unique(np.append(np.asarray(ranks, dtype=np.int64) % n, n - 1))
    got = {}
    for lo in range(0, len(want), native.SELECT_MAX_RANKS):
        part = want[lo:lo + native.SELECT_MAX_RANKS]
        got.update(zip(part.tolist(), native.select_ranks(x, part).tolist()))
    return got, bool(np.isnan(got[n - 1]))


def _quantile_vector(x, q, method):
    q = np.asarray(q, dtype=np.float64)
    if isinstance(x, _Scalar):
        quantile_indexes(x.n, q, method)  # (validates q and method)
        return quantile_of_sorted(x.host(), q, method)
    n = x.shape[0]
    prev, nxt, gamma = quantile_indexes(n, q, method)
    flat_prev, flat_next = prev.reshape(-1) % n, nxt.reshape(-1) % n
    got, has_nan = _select(x, np.concatenate([flat_prev, flat_next]))
    if has_nan:
        return np.full(q.shape, np.nan)[()]
    lo_v = np.array([got[r] for r in flat_prev.tolist()], dtype=np.float64)
    hi_v = np.array([got[r] for r in flat_next.tolist()], dtype=np.float64)
    return lerp(lo_v.reshape(q.shape), hi_v.reshape(q.shape), gamma)[()]


def quantile(node, q, method="linear"):
    """np.quantile(node.samples_, q, method=method) for the methods linear, lower, higher, nearest
    and midpoint, as float64: the device picks the at most two order statistics each q needs
    (pbh_select_ranks, no sort), numpy's interpolation runs on the host over those.  Any NaN among
    the samples makes every result NaN.  For the parent of a MultivariateDistribution: over axis 0,
    one column of the result per component."""
    x = _samples(node)
    res = _per_component(x, lambda col: _quantile_vector(col, q, method))
    return np.stack(res, axis=-1) if isinstance(res, list) else res


# =============================================================================
# moments, summary
# =============================================================================
def _moment_rows(x):
    """One dict of pbh_moments' fields per column."""
    from . import native

    if isinstance(x, _Scalar):
        v, nan = x.value, np.isnan(x.value)
        zero = np.nan if nan else 0.0
        return [dict(nan=x.n if nan else 0, min=v, max=v, mean=v, m2=zero, m3=zero, m4=zero)]
    rows = native.moments(x)
    return [dict(zip(native.MOMENT_FIELDS, (int(r[0]), *map(float, r[1:])))) for r in rows]


def _summary_entry(col, n, mom, quantiles):
    with np.errstate(all="ignore"):
        std = float(np.sqrt(mom["m2"]))
        std1 = float(np.sqrt(mom["m2"] * n / (n - 1))) if n > 1 else float("nan")
    skew, kurt = _skew_kurtosis(mom["mean"], mom["m2"], mom["m3"], mom["m4"])
    qv = np.atleast_1d(_quantile_vector(col, np.asarray(quantiles, dtype=np.float64).reshape(-1), "linear"))
    return {"count": n, "nan": mom["nan"], "mean": mom["mean"], "std": std, "std_ddof1": std1, "min": mom["min"],
            "max": mom["max"], "skew": skew, "kurtosis": kurt,
            "quantiles": {float(p): float(v) for p, v in zip(np.asarray(quantiles, dtype=np.float64).reshape(-1), qv)}}


def summary(*nodes, quantiles=(0.1, 0.5, 0.9)):
    """Per sampled node a plain dict: count, nan (the number of NaNs), mean, std (ddof 0),
    std_ddof1, min, max, skew and kurtosis (scipy.stats' biased defaults) and quantiles
    ({q: np.quantile(samples, q)}).  The parent of a MultivariateDistribution gives a list with one
    dict per component.  One node: its entry; several: the list of their entries."""
    if not nodes:
        raise TypeError("summary() needs at least one node")
    out = []
    for node in nodes:
        x = _samples(node)
        moms = _moment_rows(x)
        if isinstance(x, _Scalar) or x.dim() == 1:
            n = x.n if isinstance(x, _Scalar) else x.shape[0]
            out.append(_summary_entry(x, n, moms[0], quantiles))
        else:
            out.append([_summary_entry(x[c], x.shape[1], moms[c], quantiles) for c in range(x.shape[0])])
    return out[0] if len(nodes) == 1 else out


# =============================================================================
# histogram
# =============================================================================
def _histogram_vector(x, bins, rng):
    from . import native

    if rng is None:
        mom = _moment_rows(x)[0]
        lo, hi = mom["min"], mom["max"]
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"autodetected range of [{lo}, {hi}] is not finite")
    else:
        lo, hi = (float(v) for v in rng)
        if lo > hi:
            raise ValueError("max must be larger than min in range parameter.")
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
    if lo == hi:  # numpy's widening of an empty range
        lo, hi = lo - 0.5, hi + 0.5
    if isinstance(x, _Scalar):
        counts, edges = np.histogram(x.host(), bins=bins, range=(lo, hi))
        return counts * x.n, edges
    return native.histogram(x, bins, (lo, hi))


def histogram(node, bins=10, range=None):
    """np.histogram(node.samples_, bins=bins, range=range) -> (counts, edges) for an integer number
    of at most 4096 uniform bins.  Without a range the minimum and maximum come from the device
    (widened by 0.5 to each side when equal, as numpy does); a non-finite one raises ValueError.
    The parent of a MultivariateDistribution gives one (counts, edges) per component."""
    if np.ndim(bins) != 0 or isinstance(bins, str):
        raise NotImplementedError("histogram takes an integer number of uniform bins; a sequence of bin edges or a "
                                  "binning rule by name is not provided on the device")
    nb = int(bins)
    if nb != bins or nb < 1:
        raise ValueError("`bins` must be a positive integer")
    from .native import HISTOGRAM_MAX_BINS

    if nb > HISTOGRAM_MAX_BINS:
        raise NotImplementedError(f"histogram takes at most {HISTOGRAM_MAX_BINS} bins on the device; got {nb}")
    return _per_component(_samples(node), lambda col: _histogram_vector(col, nb, range))


# =============================================================================
# achieved correlation
# =============================================================================
def corrcoef(*nodes, kind="pearson"):
    """The K x K correlation the sampled nodes achieved: np.corrcoef of their vectors
    (kind="pearson") or of their average ranks (kind="spearman": scipy.stats.spearmanr), with the
    kernels of Iman-Conover's step 2 (pbh_column_sums, pbh_centered_gram, pbh_ic_factor's
    correlation output) and pbh_rankdata_average.  At most correlation.MAX_VARIABLES nodes."""
    import ctypes

    from . import _lib, device
    from .correlation import MAX_VARIABLES

    if kind not in ("pearson", "spearman"):
        raise ValueError(f"kind {kind!r} is not 'pearson' or 'spearman'")
    K = len(nodes)
    if K < 1:
        raise TypeError("corrcoef() needs at least one node")
    if K > MAX_VARIABLES:
        raise ValueError(f"corrcoef takes at most {MAX_VARIABLES} nodes on the device; got {K}")
    cols = [_samples(node) for node in nodes]
    for node, x in zip(nodes, cols):
        if isinstance(x, _Scalar) or x.dim() != 1:
            raise ValueError(f"corrcoef takes nodes that hold one sample vector each; {node} does not")
    n = cols[0].shape[0]
    if any(x.shape[0] != n for x in cols):
        raise ValueError("corrcoef: the nodes hold different numbers of samples")
    if n < 2:
        raise ValueError("corrcoef needs at least two samples")
    lib = _lib.load()
    S = device.empty((K, n))
    if kind == "spearman":
        nb = ctypes.c_size_t()
        _lib.check(lib.pbh_rank_workspace_size(n, ctypes.byref(nb)))
        ws = device.empty(nb.value, "uint8")
        for c, x in enumerate(cols):
            _lib.check(lib.pbh_rankdata_average(x.data_ptr(), 1, n, S[c].data_ptr(), ws.data_ptr(), nb.value,
                                                device.stream()), "pbh_rankdata_average")
        del ws
    else:
        for c, x in enumerate(cols):
            S[c].copy_(x)
    nb = ctypes.c_size_t()
    _lib.check(lib.pbh_gram_workspace_size(K, ctypes.byref(nb)))
    ws = device.empty(nb.value, "uint8")
    sums = device.zeros(K)
    _lib.check(lib.pbh_column_sums(S.data_ptr(), n, K, S.stride(0), sums.data_ptr(), ws.data_ptr(), nb.value,
                                   device.stream()), "pbh_column_sums")
    means = device.to_device(device.to_host(sums) / n)
    gram = device.zeros((K, K))
    _lib.check(lib.pbh_centered_gram(S.data_ptr(), n, K, S.stride(0), means.data_ptr(), gram.data_ptr(),
                                     ws.data_ptr(), nb.value, device.stream()), "pbh_centered_gram")
    g = np.ascontiguousarray(device.to_host(gram))
    E, L = np.zeros((K, K)), np.zeros((K, K))
    st = lib.pbh_ic_factor(g.ctypes.data, n, K, E.ctypes.data, L.ctypes.data)
    if st != _lib.ERR_NOT_PD:  # perfectly correlated nodes have a correlation matrix all the same
        _lib.check(st, "pbh_ic_factor")
    return E
