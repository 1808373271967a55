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
    histogram2d(a, b, bins=10, range=None)        np.histogram2d(a.samples_, b.samples_, bins, range)
    pairgrid(*nodes, bins=30, range=None)         PairGrid: every pair's 2-d histogram, every node's own
    PairGrid.draw(fig=None)                       the K x K grid of those counts with matplotlib
    binned_statistic(x, values, statistic="mean", bins=10, range=None)
                                                  scipy.stats.binned_statistic(...)[:2]: count / sum / mean / std
    sensitivity(output, *inputs, bins=32, binning="quantile")
                                                  Sensitivity: E and std of the output per input bin, eta^2
    Sensitivity.order() / .draw(fig=None)         the inputs by descending eta^2; the bars and curves
    treeprint(node)                               the graph above a node, one line per node
    plot(...)                                     probabilit_amd.plot (not provided)

Limits: histograms take an integer number of at most 4096 uniform bins; joint histograms take
numpy's forms of `bins` (edge arrays included) with at most 1024 bins per axis and 16384 cells per
pair, a pair grid 2 to 16 nodes; binned statistics and sensitivity take at most 1024 bins per
binning node and 128 value nodes or inputs, offer count, sum, mean and std, and add with atomics,
so their floating-point results are not bit-reproducible from run to run; quantile methods are
linear, lower, higher, nearest and midpoint; samples row-sharded over a process group (`sample_device(group=...)` with more than one rank) are
not summarised across ranks.
"""

import numpy as np

# (histogram2d, pairgrid, PairGrid, binned_statistic, sensitivity and Sensitivity are public as
# well; the names a star import brings are the reference module's and the first summaries, which
# tests/test_inspection_host.py pins)
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


def axis_edges(axis, bins, rng, limits):
    """np.histogramdd's edges of one axis (lib/_histograms_impl.py histogramdd, _get_outer_edges)
    with its errors.  bins: a number of bins or a 1-d array of edges, returned as np.asarray gives
    it; rng: (lo, hi) or None, read only for a number of bins; limits(axis) -> (min, max) of the
    axis' samples, called only when both a number of bins and no range are given."""
    import operator

    if np.ndim(bins) == 0:
        if bins < 1:
            raise ValueError(f"`bins[{axis}]` must be positive, when an integer")
        if rng is not None:
            lo, hi = rng
            if lo > hi:
                raise ValueError("max must be larger than min in range parameter.")
            if not (np.isfinite(lo) and np.isfinite(hi)):
                raise ValueError(f"supplied range of [{lo}, {hi}] is not finite")
        else:
            lo, hi = limits(axis)
            if not (np.isfinite(lo) and np.isfinite(hi)):
                raise ValueError(f"autodetected range of [{lo}, {hi}] is not finite")
        if lo == hi:  # numpy's widening of an empty range
            lo, hi = lo - 0.5, hi + 0.5
        try:
            nb = operator.index(bins)
        except TypeError as e:
            raise TypeError(f"`bins[{axis}]` must be an integer, when a scalar") from e
        return np.linspace(lo, hi, nb + 1)
    if np.ndim(bins) == 1:
        edges = np.asarray(bins)
        if np.any(edges[:-1] > edges[1:]):
            raise ValueError(f"`bins[{axis}]` must be monotonically increasing, when an array")
        return edges
    raise ValueError(f"`bins[{axis}]` must be a scalar or 1d array")


def uniform_edges(bins, lo, hi):
    """The `bins` + 1 uniform edges over a column's minimum and maximum, numpy's way (axis_edges
    without a range: widened by 0.5 to each side when equal, ValueError when not finite)."""
    return axis_edges(0, bins, None, lambda axis: (lo, hi))


def quantile_ranks(n, bins):
    """The `bins` + 1 zero-based ranks of the equal-probability edges of n samples: the order
    statistics np.quantile(x, k / bins, method="nearest") takes, k = 0 .. bins, so rank 0 (the
    minimum) first and rank n - 1 (the maximum) last."""
    import operator

    nb = operator.index(bins)
    if nb < 1:
        raise ValueError("`bins` must be positive")
    return quantile_indexes(n, np.arange(nb + 1) / nb, "nearest")[0].astype(np.int64)


def quantile_edges(values_at_ranks):
    """The edge table from the order statistics at quantile_ranks: the values as they are, ties
    kept as repeated edges (which give empty bins); a constant column's range is widened by 0.5 to
    each side as axis_edges does.  A non-finite value (a NaN among the samples sorts last) raises
    ValueError."""
    e = np.array(values_at_ranks, dtype=np.float64).ravel()
    if len(e) < 2:
        raise ValueError("quantile_edges needs at least two order statistics")
    if not np.all(np.isfinite(e)):
        raise ValueError(f"autodetected range of [{e[0]}, {e[-1]}] is not finite")
    if np.any(e[:-1] > e[1:]):
        raise ValueError("the order statistics must be non-decreasing")
    if e[0] == e[-1]:
        e[0], e[-1] = e[0] - 0.5, e[-1] + 0.5
    return e


BINNED_STATISTICS = ("count", "sum", "mean", "std")


def binned_finish(count, s1, s2, centre, statistic):
    """scipy.stats.binned_statistic's `statistic` per bin, as float64, from pbh_binned_sums' raw
    sums about `centre` (count rows, s1 = sum(y - centre), s2 = sum((y - centre)^2)):
    count; sum = s1 + count centre; mean = centre + s1 / count; std (ddof 0) =
    sqrt(max(s2 / count - (s1 / count)^2, 0)).  Empty bins give NaN for mean and std and 0 for
    count and sum, as scipy does."""
    if statistic not in BINNED_STATISTICS:
        raise ValueError(f"statistic {statistic!r} is not one of {BINNED_STATISTICS}")
    cnt = np.asarray(count, dtype=np.float64)
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    if not (cnt.shape == s1.shape == s2.shape):
        raise ValueError("count, s1 and s2 must have one shape")
    centre = float(centre)
    if statistic == "count":
        return cnt.copy()
    if statistic == "sum":
        return np.where(cnt > 0, s1 + cnt * centre, 0.0)
    with np.errstate(all="ignore"):
        m1 = s1 / cnt
        if statistic == "mean":
            return np.where(cnt > 0, centre + m1, np.nan)
        var = s2 / cnt - m1 * m1
        return np.where(cnt > 0, np.sqrt(np.where(var < 0.0, 0.0, var)), np.nan)  # (a NaN variance stays NaN)


def correlation_ratio(count, s1, s2):
    """eta^2 = Var(E[Y | X]) / Var(Y) over the bins of X, from the raw sums about any centre:
    sum_b n_b (s1_b / n_b - S1 / N)^2 / (S2 - S1^2 / N) with S1, S2, N the totals over the bins, so
    the base is the rows inside the edges.  NaN when the denominator is not positive (no rows, a
    constant Y, or a non-finite sum)."""
    cnt = np.asarray(count, dtype=np.float64)
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    if not (cnt.shape == s1.shape == s2.shape) or cnt.ndim != 1:
        raise ValueError("count, s1 and s2 must be vectors of one length")
    N = cnt.sum()
    if not N > 0:
        return float("nan")
    has = cnt > 0
    S1, S2 = s1[has].sum(), s2[has].sum()
    with np.errstate(all="ignore"):
        den = S2 - S1 * S1 / N
        if not den > 0.0:
            return float("nan")
        dev = s1[has] / cnt[has] - S1 / N
        return float((cnt[has] * dev * dev).sum() / den)


class Sensitivity:
    """What K inputs explain of one output (sensitivity): `output` and `labels` (str(node)),
    `count` samples, and per input k `edges[k]`, `counts[k]` (int64 rows per bin),
    `conditional_mean[k]` and `conditional_std[k]` (E and std of the output given the input's bin;
    NaN for an empty bin), and `first_order`, the (K,) correlation ratios eta^2."""

    def __init__(self, output, labels, count, edges, counts, conditional_mean, conditional_std, first_order):
        self.output, self.labels, self.count = str(output), list(labels), int(count)
        self.edges, self.counts = list(edges), list(counts)
        self.conditional_mean, self.conditional_std = list(conditional_mean), list(conditional_std)
        self.first_order = np.asarray(first_order, dtype=np.float64)

    def order(self):
        """The inputs' indices by descending eta^2 (NaN last, ties in the given order)."""
        key = np.where(np.isnan(self.first_order), -np.inf, self.first_order)
        return np.argsort(-key, kind="stable")

    def draw(self, fig=None):
        """Draw with matplotlib and return the figure: on top the horizontal bars of eta^2 in
        descending order, below it every input's conditional-mean curve over its bin centres, in
        the same order.  Draws what the object holds: nothing is downloaded."""
        try:
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError("Sensitivity.draw needs matplotlib, which is not installed") from e
        order = self.order()
        k = len(order)
        if fig is None:
            fig = plt.figure(figsize=(6.0, 2.0 + 0.25 * k + 1.8 * k))
        axes = fig.subplots(k + 1, 1, squeeze=False)[:, 0]
        top = axes[0]
        top.barh(np.arange(k), self.first_order[order])
        top.set_yticks(np.arange(k))
        top.set_yticklabels([self.labels[i] for i in order])
        top.invert_yaxis()
        top.set_xlabel(f"first-order share of Var({self.output})")
        for ax, i in zip(axes[1:], order):
            e = np.asarray(self.edges[i], dtype=np.float64)
            has = np.asarray(self.counts[i]) > 0
            ax.plot((0.5 * (e[:-1] + e[1:]))[has], np.asarray(self.conditional_mean[i])[has], marker=".")
            ax.set_xlabel(self.labels[i])
            ax.set_ylabel(f"E[{self.output} | bin]")
        return fig


def histogram2d_edges(bins, rng, limits):
    """[xedges, yedges] of np.histogram2d(x, y, bins=bins, range=rng) for numpy's forms of `bins`:
    an int, (nx, ny), one edge array for both axes, or (xedges | nx, yedges | ny); rng is None or
    ((xlo, xhi) | None, (ylo, yhi) | None).  limits: as for axis_edges."""
    try:
        nb = len(bins)
    except TypeError:  # a number of bins for both axes
        nb, bins = 2, [bins, bins]
    if nb == 1:
        raise ValueError("The dimension of bins must be equal to the dimension of the sample x.")
    if nb != 2:  # np.histogram2d: one edge array for both axes
        both = np.asarray(bins)
        bins = [both, both]
    if rng is None:
        rng = (None, None)
    elif len(rng) != 2:
        raise ValueError("range argument must have one entry per dimension")
    return [axis_edges(i, bins[i], rng[i], limits) for i in range(2)]


def pairgrid_edges(k, bins, rng, limits):
    """The k edge arrays of pairgrid: `bins` one number of bins or one per node, `rng` None or one
    (lo, hi) | None per node; every axis by axis_edges."""
    if np.ndim(bins) == 0:
        bins = [bins] * k
    elif np.ndim(bins) != 1 or len(bins) != k:
        raise ValueError(f"pairgrid: `bins` must be one number of bins or one per node ({k})")
    if rng is None:
        rng = [None] * k
    elif len(rng) != k:
        raise ValueError(f"pairgrid: `range` must be None or one entry per node ({k}); got {len(rng)}")
    return [axis_edges(i, bins[i], rng[i], limits) for i in range(k)]


class PairGrid:
    """The binned pair grid of K nodes (pairgrid): `count` samples, `labels` (str(node) per node),
    `edges` (K edge arrays), `diagonal` (K int64 count vectors) and joint(i, j)."""

    def __init__(self, count, labels, edges, diagonal, joints):
        """joints: {(i, j): (bins_i, bins_j) int64 matrix} for every i < j."""
        self.count, self.labels = int(count), list(labels)
        self.edges, self.diagonal = list(edges), list(diagonal)
        self._joints = dict(joints)

    def joint(self, i, j):
        """The (bins_i, bins_j) int64 counts of node i (rows) against node j (columns)."""
        k = len(self.labels)
        if not (0 <= i < k and 0 <= j < k):
            raise IndexError(f"joint({i}, {j}): the grid has {k} nodes")
        if i == j:
            raise ValueError(f"joint({i}, {j}): the diagonal holds the one-node histograms (`diagonal`)")
        return self._joints[(i, j)] if i < j else self._joints[(j, i)].T

    def draw(self, fig=None, **imshow_kwargs):
        """Draw the K x K grid with matplotlib and return the figure: bars of `diagonal` on the
        diagonal, pcolormesh of joint(i, j) over the edges (node j along x, node i along y) off it.
        The keyword arguments go to pcolormesh."""
        try:
            import matplotlib.pyplot as plt
        except ImportError as e:
            raise ImportError("PairGrid.draw needs matplotlib, which is not installed") from e
        k = len(self.labels)
        if fig is None:
            fig = plt.figure(figsize=(2.4 * k, 2.4 * k))
        axes = fig.subplots(k, k, squeeze=False)
        for i in range(k):
            for j in range(k):
                ax = axes[i][j]
                if i == j:
                    e = np.asarray(self.edges[i], dtype=np.float64)
                    ax.bar(e[:-1], self.diagonal[i], width=np.diff(e), align="edge")
                else:
                    ax.pcolormesh(self.edges[j], self.edges[i], self.joint(i, j), **imshow_kwargs)
                if i == k - 1:
                    ax.set_xlabel(self.labels[j])
                if j == 0:
                    ax.set_ylabel(self.labels[i])
        return fig


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
# joint histograms
# =============================================================================
def _joint_columns(what, nodes):
    """corrcoef's rules: one float64 device vector per node, all of one length."""
    cols = [_samples(node) for node in nodes]
    for node, x in zip(nodes, cols):
        if isinstance(x, _Scalar) or x.dim() != 1:
            raise ValueError(f"{what} takes nodes that hold one sample vector each; {node} does not")
    if any(x.shape[0] != cols[0].shape[0] for x in cols):
        raise ValueError(f"{what}: the nodes hold different numbers of samples")
    return cols


def _limits_of(cols):
    def limits(axis):
        mom = _moment_rows(cols[axis])[0]
        return mom["min"], mom["max"]

    return limits


def _device_edges(what, edges, pairs):
    """The float64 edge arrays the kernel takes, within its caps."""
    from . import native

    out = [np.ascontiguousarray(e, dtype=np.float64) for e in edges]
    for i, e in enumerate(out):
        if len(e) < 2:
            raise ValueError(f"{what}: `bins[{i}]` needs at least two edges")
        if len(e) - 1 > native.HISTOGRAM2D_MAX_BINS:
            raise NotImplementedError(f"{what} takes at most {native.HISTOGRAM2D_MAX_BINS} bins per axis on the "
                                      f"device; got {len(e) - 1}")
    for i, j in pairs:
        cells = (len(out[i]) - 1) * (len(out[j]) - 1)
        if cells > native.HISTOGRAM2D_MAX_CELLS:
            raise NotImplementedError(f"{what} takes at most {native.HISTOGRAM2D_MAX_CELLS} cells per pair of nodes "
                                      f"on the device; got {len(out[i]) - 1} x {len(out[j]) - 1} = {cells}")
    return out


def histogram2d(a, b, bins=10, range=None):
    """np.histogram2d(a.samples_, b.samples_, bins=bins, range=range) -> (H, xedges, yedges) with H
    as int64 (numpy's is float64 with the same values) and numpy's edges.  `bins`: an int,
    (nx, ny), one edge array for both axes or (xedges | nx, yedges | ny), at most 1024 bins per axis
    and 16384 cells; `range`: None or ((xlo, xhi) | None, (ylo, yhi) | None).  Without a range an
    axis uses the minimum and maximum from the device (widened by 0.5 to each side when equal); a
    non-finite one raises ValueError.  Both nodes must hold one sample vector of the same length.
    One sweep over the two columns (pbh_histogram2d); only the counts come back."""
    from . import native

    cols = _joint_columns("histogram2d", (a, b))
    edges = histogram2d_edges(bins, range, _limits_of(cols))
    H = native.histogram2d(cols, _device_edges("histogram2d", edges, [(0, 1)]), [(0, 1)])[0]
    return H, edges[0], edges[1]


def pairgrid(*nodes, bins=30, range=None):
    """The binned joint view of 2 to 16 sampled nodes, a PairGrid: every pair's 2-d histogram (all
    K (K - 1) / 2 of them in one pbh_histogram2d launch) and every node's own histogram over the
    same edges.  `bins`: one number of bins or one entry per node (at most 1024 per node, 16384
    cells per pair); `range`: None or one (lo, hi) | None per node, the device minimum and maximum
    otherwise.  Only the counts come back; PairGrid.draw() plots them."""
    from . import native

    K = len(nodes)
    if K < 2 or K > native.HISTOGRAM2D_MAX_COLUMNS:
        raise ValueError(f"pairgrid takes 2 to {native.HISTOGRAM2D_MAX_COLUMNS} nodes on the device; got {K}")
    cols = _joint_columns("pairgrid", nodes)
    edges = pairgrid_edges(K, bins, range, _limits_of(cols))
    pairs = [(i, j) for i, j in np.ndindex(K, K) if i < j]
    dev_edges = _device_edges("pairgrid", edges, pairs)
    mats = native.histogram2d(cols, dev_edges, pairs)
    # (uniform edges: np.linspace over the same ends gives pbh_histogram the same table)
    diagonal = [native.histogram(x, len(e) - 1, (e[0], e[-1]))[0] for x, e in zip(cols, dev_edges)]
    return PairGrid(cols[0].shape[0], [str(node) for node in nodes], edges, diagonal, dict(zip(pairs, mats)))


# =============================================================================
# conditional statistics, first-order sensitivity
# =============================================================================
def _binning_edges(what, e):
    """One float64 edge array the kernel takes, within its cap."""
    from . import native

    e = np.ascontiguousarray(e, dtype=np.float64)
    if len(e) < 2:
        raise ValueError(f"{what}: `bins` needs at least two edges")
    if len(e) - 1 > native.BINNED_MAX_BINS:
        raise NotImplementedError(f"{what} takes at most {native.BINNED_MAX_BINS} bins on the device; got {len(e) - 1}")
    return e


def _centre(col):
    """The column's mean from the device, or 0 where it is not finite (the sums then carry the
    NaN or inf themselves)."""
    mean = _moment_rows(col)[0]["mean"]
    return mean if np.isfinite(mean) else 0.0


def binned_statistic(x, values, statistic="mean", bins=10, range=None):
    """scipy.stats.binned_statistic(x.samples_, values.samples_, statistic, bins, range) without
    its N-sized binnumber: (statistic, bin_edges), the statistic as float64.  `statistic`: count,
    sum, mean or std (median, min, max and callables have no device path); `values`: one node, or a
    list of up to 128, which gives a (len, bins) result; `bins`: a number of bins or an array of
    edges, at most 1024 bins; `range`: (lo, hi) or None, then the minimum and maximum of x from the
    device (widened by 0.5 to each side when equal; a non-finite one raises ValueError).  The bin
    rule is numpy's: the last bin is closed and rows outside the edges or with a NaN x are dropped.
    Every node must hold one sample vector of the same length.  One sweep over the columns
    (pbh_binned_sums) about each value column's mean; its sums come from atomics, so the last bits
    of sum, mean and std change from run to run.  Only the per-bin numbers come back."""
    from . import native

    if statistic not in BINNED_STATISTICS:
        raise ValueError(f"statistic {statistic!r} is not one of {BINNED_STATISTICS}; median, min, max and callables "
                         "are not provided on the device")
    many = isinstance(values, (list, tuple))
    vals = list(values) if many else [values]
    if not 1 <= len(vals) <= native.BINNED_MAX_PAIRS:
        raise ValueError(f"binned_statistic takes 1 to {native.BINNED_MAX_PAIRS} value nodes; got {len(vals)}")
    cols = _joint_columns("binned_statistic", (x, *vals))
    edges = axis_edges(0, bins, range, _limits_of(cols))
    dev_edges = _binning_edges("binned_statistic", edges)
    centres = [0.0] + [0.0 if statistic == "count" else _centre(c) for c in cols[1:]]
    raw = native.binned_sums(cols, [dev_edges] + [None] * len(vals), [(0, 1 + v) for v in np.arange(len(vals))], centres)
    out = np.stack([binned_finish(c, s1, s2, ctr, statistic) for (c, s1, s2), ctr in zip(raw, centres[1:])])
    return (out if many else out[0]), edges


def sensitivity(output, *inputs, bins=32, binning="quantile"):
    """Which of 1 to 128 inputs drive `output`: a Sensitivity with, per input, the output's mean
    and std given the input's bin and the correlation ratio eta^2 = Var(E[output | input]) /
    Var(output), the given-data estimate of the first-order share of the variance, which unlike
    corrcoef also sees non-monotone dependence (products, maxima, comparisons).  `bins`: 1 to 1024
    per input; binning="quantile": equal-probability edges per input, the order statistics at ranks
    round(k (n - 1) / bins) (pbh_select_ranks; ties give repeated edges and empty bins),
    binning="uniform": uniform edges from the input's minimum to its maximum; a constant input's
    range is widened by 0.5 to each side.  One pbh_binned_sums launch covers all inputs; its sums
    come from atomics, so the last bits change from run to run.  Nothing N-sized comes back."""
    import operator

    from . import native

    K = len(inputs)
    if not 1 <= K <= native.BINNED_MAX_PAIRS:
        raise ValueError(f"sensitivity takes 1 to {native.BINNED_MAX_PAIRS} inputs on the device; got {K}")
    if binning not in ("quantile", "uniform"):
        raise ValueError(f"binning {binning!r} is not 'quantile' or 'uniform'")
    try:
        nb = operator.index(bins)
    except TypeError as e:
        raise TypeError("`bins` must be an integer") from e
    if not 1 <= nb <= native.BINNED_MAX_BINS:
        raise ValueError(f"sensitivity takes 1 to {native.BINNED_MAX_BINS} bins per input; got {nb}")
    cols = _joint_columns("sensitivity", (output, *inputs))
    n = cols[0].shape[0]
    edges = []
    for x in cols[1:]:
        if binning == "quantile":
            ranks = quantile_ranks(n, nb)
            got, _ = _select(x, ranks)
            edges.append(quantile_edges([got[r] for r in ranks.tolist()]))
        else:
            mom = _moment_rows(x)[0]
            edges.append(uniform_edges(nb, mom["min"], mom["max"]))
    centre = _centre(cols[0])
    raw = native.binned_sums(cols, [None] + edges, [(1 + k, 0) for k in np.arange(K)], [centre] + [0.0] * K)
    return Sensitivity(output, [str(node) for node in inputs], n, edges, [c for c, _, _ in raw],
                       [binned_finish(c, s1, s2, centre, "mean") for c, s1, s2 in raw],
                       [binned_finish(c, s1, s2, centre, "std") for c, s1, s2 in raw],
                       [correlation_ratio(c, s1, s2) for c, s1, s2 in raw])


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
