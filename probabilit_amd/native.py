"""Thin numpy/torch front-ends for single native kernels (used by tests, bench and callers
that want one kernel without building a DAG).  Each wraps one C-ABI entry point."""

import numpy as np

from . import _lib, device
from .modeling import _DIST_SHAPES, _parse_scipy_args


def _dev_vec(a):
    import torch

    if isinstance(a, torch.Tensor):
        return a.to(device.device(), torch.float64).contiguous()
    return device.to_device(np.ascontiguousarray(a, dtype=np.float64))


def _params(name, n, kwargs):
    out, keep = [], []
    for v in _parse_scipy_args(name, (), kwargs):
        a = np.asarray(v) if not hasattr(v, "data_ptr") else None
        if a is not None and a.ndim == 0:
            out.append(_lib.Param(None, float(a)))
        else:
            t = _dev_vec(v)
            assert t.shape == (n,)
            keep.append(t)
            out.append(_lib.Param(t.data_ptr(), 0.0))
    return (_lib.Param * len(out))(*out), keep


def ppf(name, q, return_device=False, **params):
    """scipy.stats.<name>(**params).ppf(q) on the GPU (pbh_ppf)."""
    if name not in _DIST_SHAPES:
        raise NotImplementedError(name)
    qd = _dev_vec(q)
    n = qd.shape[0]
    arr, keep = _params(name, n, params)
    out = device.empty(n)
    flag = device.zeros(1, "int32")
    _lib.check(_lib.load().pbh_ppf(_lib.DIST_IDS[name], qd.data_ptr(), 1, n, arr, len(arr), out.data_ptr(),
                                   flag.data_ptr(), device.stream()), "pbh_ppf")
    del keep
    return out if return_device else device.to_host(out)


def lhs_ppf(name, seed, n_total, col, row0=0, nrows=None, return_device=False, **params):
    """Fused native-LHS column `col` of an n_total-row design pushed through ppf (pbh_lhs_ppf).
    (n_total, not n: binom's shape parameter is called n.)"""
    nrows = n_total - row0 if nrows is None else nrows
    arr, keep = _params(name, nrows, params)
    out = device.empty(nrows)
    _lib.check(_lib.load().pbh_lhs_ppf(seed, n_total, row0, nrows, col, _lib.DIST_IDS[name], arr, len(arr),
                                       out.data_ptr(), None, device.stream()), "pbh_lhs_ppf")
    del keep
    return out if return_device else device.to_host(out)


def fill_lhs(seed, n, d, row0=0, nrows=None, return_device=False):
    """(nrows, d) native Latin hypercube rows [row0, row0 + nrows) (column-major on device)."""
    nrows = n - row0 if nrows is None else nrows
    q = device.empty((d, nrows))
    _lib.check(_lib.load().pbh_fill_lhs(seed, n, row0, nrows, 0, d, q.data_ptr(), nrows, device.stream()),
               "pbh_fill_lhs")
    return q if return_device else device.to_host(q).T


def fill_uniform(seed, n, d, row0=0, return_device=False):
    q = device.empty((d, n))
    _lib.check(_lib.load().pbh_fill_uniform(seed, row0, n, 0, d, q.data_ptr(), n, device.stream()),
               "pbh_fill_uniform")
    return q if return_device else device.to_host(q).T


MULTIVARIATE = ("multivariate_normal", "dirichlet", "multinomial")


def mvn_factor(cov):
    """A with A A^T = cov: V diag(sqrt(max(lambda, 0))) of np.linalg.eigh(cov) (what numpy's own
    multivariate_normal factors a positive semi-definite cov by: rank-deficient ones included)."""
    cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
    lam, V = np.linalg.eigh(cov)
    return np.ascontiguousarray(V * np.sqrt(np.maximum(lam, 0.0)))


def multinomial_conditionals(p):
    """pc_j = clip(p_j / (1 - sum_{k<j} p_k), 0, 1), the prefix sum left to right in float64: the
    success probability of category j among the trials the categories before it left over (0 where
    they left none)."""
    p = np.asarray(p, dtype=np.float64).ravel()
    left = 1.0 - np.concatenate([[0.0], np.cumsum(p)[:-1]])
    with np.errstate(divide="ignore", invalid="ignore"):
        pc = np.where(left > 0.0, p / left, 0.0)
    return np.clip(pc, 0.0, 1.0)


def multivariate_tables(name, frozen):
    """The host parameter tables of the fused sampler of scipy.stats.<name>'s frozen distribution
    (whose construction validated the arguments): (d, tables).  No device call."""
    from .correlation import MAX_VARIABLES

    if name == "multivariate_normal":
        mean = np.ascontiguousarray(np.atleast_1d(frozen.mean), dtype=np.float64)
        tables = (mean, mvn_factor(frozen.cov))
    elif name == "dirichlet":
        alpha = np.asarray(frozen.alpha, dtype=np.float64)
        if alpha.ndim != 1:
            raise NotImplementedError(f"dirichlet: alpha of shape {alpha.shape}; the device path takes one vector")
        tables = (np.ascontiguousarray(alpha),)
    elif name == "multinomial":
        if np.ndim(frozen.n) != 0 or np.ndim(frozen.p) != 1:
            raise NotImplementedError("multinomial: the device path takes a scalar n and one vector p, got shapes "
                                      f"{np.shape(frozen.n)} and {np.shape(frozen.p)}")
        if np.any(frozen.npcond):
            raise ValueError("multinomial: n must be a non-negative integer and p probabilities that sum to 1")
        tables = (float(frozen.n), multinomial_conditionals(frozen.p))
    else:
        raise NotImplementedError(name)
    d = len(tables[-1])
    if d > MAX_VARIABLES:
        raise ValueError(f"probabilit_amd samples at most {MAX_VARIABLES} components of a multivariate "
                         f"distribution on the device; got {d}")
    return d, tables


def multivariate_launch(name, tables, seed, n, row0, flag_ptr=None):
    """The (d, n) device block of rows [row0, row0 + n) of the sampler's stream `seed`."""
    lib = _lib.load()
    d = len(tables[-1])
    out = device.empty((d, n), "int64" if name == "multinomial" else "float64")
    if name == "multivariate_normal":
        mean, A = tables
        st = lib.pbh_multivariate_normal(seed, row0, n, d, _lib.np_ptr(mean), _lib.np_ptr(A), out.data_ptr(), n,
                                         flag_ptr, device.stream())
    elif name == "dirichlet":
        st = lib.pbh_dirichlet(seed, row0, n, d, _lib.np_ptr(tables[0]), out.data_ptr(), n, flag_ptr, device.stream())
    else:
        trials, pc = tables
        st = lib.pbh_multinomial(seed, row0, n, d, trials, _lib.np_ptr(pc), out.data_ptr(), n, flag_ptr,
                                 device.stream())
    _lib.check(st, f"pbh_{name}")
    return out


def multivariate(name, seed, n, row0=0, return_device=False, **params):
    """Rows [row0, row0 + n) of scipy.stats.<name>(**params) drawn by the fused native sampler from
    the uniforms fill_uniform(seed, n, d, row0) (a native stream, not numpy's): (n, d) on the host or
    (d, n) on the device.  n is the number of rows, as everywhere in this module; multinomial's
    number of trials is passed as `trials`."""
    import scipy.stats

    if name not in MULTIVARIATE:
        raise NotImplementedError(name)
    if name == "multinomial" and "trials" in params:
        params = dict(params, n=params["trials"])
        del params["trials"]
    _, tables = multivariate_tables(name, getattr(scipy.stats, name)(**params))
    out = multivariate_launch(name, tables, seed, n, row0)
    return out if return_device else device.to_host(out).T


def fill_sobol(sv, shift, n, bits=30, row0=0, return_device=False):
    sv = np.ascontiguousarray(sv, dtype=np.uint32)
    shift = np.ascontiguousarray(shift, dtype=np.uint32)
    d = sv.shape[0]
    q = device.empty((d, n))
    _lib.check(_lib.load().pbh_fill_sobol(_lib.np_ptr(sv), _lib.np_ptr(shift), d, bits, row0, n, 0, d, q.data_ptr(),
                                          n, device.stream()), "pbh_fill_sobol")
    return q if return_device else device.to_host(q).T


# launch shapes of the summary kernels (include/probabilit_hip.h): a block's tile and the samples
# one sweep of the whole grid spans
SUMMARY_TILE, SUMMARY_SPAN = 2048, 2048 * 1024
SELECT_TILE, SELECT_SPAN = 16384, 16384 * 256
SELECT_MAX_RANKS = 64
HISTOGRAM_MAX_BINS = 4096
HISTOGRAM2D_MAX_BINS, HISTOGRAM2D_MAX_CELLS = 1024, 16384  # per axis; bins_x * bins_y of one pair
HISTOGRAM2D_MAX_COLUMNS, HISTOGRAM2D_MAX_PAIRS = 16, 120
BINNED_MAX_BINS, BINNED_MAX_COLUMNS, BINNED_MAX_PAIRS = 1024, 129, 128  # 128 inputs and one output
MOMENT_FIELDS = ("nan", "min", "max", "mean", "m2", "m3", "m4")


def moments_terms(n):
    """(serial length L(n), tree depth D) of every sum pbh_moments forms over n samples: the
    summation shape stated beside its declaration, from which a caller bounds the rounding error."""
    tiles = -(-n // SUMMARY_TILE)
    blocks = min(tiles, SUMMARY_SPAN // SUMMARY_TILE)
    return 8 * -(-tiles // blocks) + -(-blocks // 256), 16


def _block(x_dev):
    """(k, n, ld) of a device float64 vector or (k, n) block whose rows are contiguous."""
    import torch

    if not isinstance(x_dev, torch.Tensor) or x_dev.dtype != torch.float64 or x_dev.dim() not in (1, 2):
        raise TypeError("a float64 device vector or (k, n) block is required")
    if x_dev.stride(-1) != 1 and x_dev.shape[-1] > 1:
        raise ValueError("the samples of a column must be contiguous")
    if x_dev.dim() == 1:
        return 1, x_dev.shape[0], x_dev.shape[0]
    return x_dev.shape[0], x_dev.shape[1], (x_dev.stride(0) if x_dev.shape[0] > 1 else x_dev.shape[1])


def _workspace(query, arg):
    import ctypes

    b = ctypes.c_size_t()
    _lib.check(query(arg, ctypes.byref(b)))
    return device.empty(b.value, "uint8"), b.value


def moments(x_dev):
    """(k, 7) host array of MOMENT_FIELDS per column of a device vector / (k, n) block (pbh_moments)."""
    lib = _lib.load()
    k, n, ld = _block(x_dev)
    ws, nbytes = _workspace(lib.pbh_moments_workspace_size, k)
    out = device.empty((k, 8))
    _lib.check(lib.pbh_moments(x_dev.data_ptr(), n, k, ld, out.data_ptr(), ws.data_ptr(), nbytes, device.stream()),
               "pbh_moments")
    return device.to_host(out)[:, :7]


def select_ranks(x_dev, ranks):
    """np.sort(x)[ranks] of one device vector for at most SELECT_MAX_RANKS ranks (pbh_select_ranks)."""
    lib = _lib.load()
    k, n, _ = _block(x_dev)
    if k != 1:
        raise ValueError("select_ranks takes one column")
    ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
    out = np.empty(len(ranks), dtype=np.float64)
    if len(ranks) == 0:
        return out
    ws, nbytes = _workspace(lib.pbh_select_workspace_size, len(ranks))
    _lib.check(lib.pbh_select_ranks(x_dev.data_ptr(), n, _lib.np_ptr(ranks), len(ranks), _lib.np_ptr(out),
                                    ws.data_ptr(), nbytes, device.stream()), "pbh_select_ranks")
    return out


def histogram(x_dev, bins, range):
    """(counts, edges): np.histogram(x, bins, range) per column of a device vector / (k, n) block for
    an integer `bins` and a finite (lo, hi); counts is (bins,) for a vector, else (k, bins)."""
    lib = _lib.load()
    k, n, ld = _block(x_dev)
    lo, hi = (float(v) for v in range)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"histogram: the range [{lo}, {hi}] is not finite and increasing")
    edges = np.linspace(lo, hi, int(bins) + 1)
    ws, nbytes = _workspace(lib.pbh_histogram_workspace_size, int(bins))
    counts = device.empty((k, int(bins)), "int64")
    _lib.check(lib.pbh_histogram(x_dev.data_ptr(), n, k, ld, _lib.np_ptr(edges), int(bins), counts.data_ptr(),
                                 ws.data_ptr(), nbytes, device.stream()), "pbh_histogram")
    host = device.to_host(counts)
    return (host[0] if x_dev.dim() == 1 else host), edges


def histogram2d(cols, edges, pairs, ws_bytes=None):
    """np.histogram2d(cols[i], cols[j], bins=(edges[i], edges[j]))[0] as an int64 host matrix per
    (i, j) of `pairs`, in one launch (pbh_histogram2d).  cols: float64 device vectors of one length;
    edges: one host edge array per column; an axis is uniform when its edges equal
    np.linspace(e[0], e[-1], len(e)) bit for bit.  ws_bytes: the workspace to allocate and state
    instead of pbh_histogram2d_workspace_size's (the library refuses one that is too small)."""
    import ctypes

    import torch

    lib = _lib.load()
    cols = list(cols)
    for x in cols:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 1:
            raise TypeError("float64 device vectors are required")
        if x.shape[0] > 1 and x.stride(0) != 1:
            raise ValueError("the samples of a column must be contiguous")
    if len(edges) != len(cols):
        raise ValueError("histogram2d: one edge array per column is required")
    if cols and any(x.shape[0] != cols[0].shape[0] for x in cols):
        raise ValueError("histogram2d: the columns hold different numbers of samples")
    k, n = len(cols), (cols[0].shape[0] if cols else 0)
    edges = [np.ascontiguousarray(e, dtype=np.float64).ravel() for e in edges]
    if any(len(e) < 2 for e in edges):
        raise ValueError("histogram2d: an axis needs at least two edges")
    bins = np.array([len(e) - 1 for e in edges], dtype=np.int32)
    with np.errstate(all="ignore"):  # (non-finite ends: the library refuses them)
        uniform = np.array([np.linspace(e[0], e[-1], len(e)).tobytes() == e.tobytes() for e in edges], dtype=np.uint8)
    flat = np.concatenate(edges) if edges else np.zeros(0)
    ptrs = np.array([x.data_ptr() for x in cols], dtype=np.uint64)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    if ws_bytes is None:
        b = ctypes.c_size_t()
        _lib.check(lib.pbh_histogram2d_workspace_size(k, _lib.np_ptr(bins), ctypes.byref(b)),
                   "pbh_histogram2d_workspace_size")
        ws_bytes = b.value
    ws = device.empty(max(int(ws_bytes), 8), "uint8")
    inside = (pr >= 0).all(axis=1) & (pr < k).all(axis=1)  # (the library refuses the others)
    shapes = [(int(bins[i]), int(bins[j])) if ok else (0, 0) for (i, j), ok in zip(pr.tolist(), inside.tolist())]
    cells = sum(a * b for a, b in shapes)
    counts = device.empty(max(cells, 1), "int64")
    _lib.check(lib.pbh_histogram2d(_lib.np_ptr(ptrs), k, n, _lib.np_ptr(flat), _lib.np_ptr(bins), _lib.np_ptr(uniform),
                                   _lib.np_ptr(pr), len(pr), counts.data_ptr(), ws.data_ptr(), int(ws_bytes),
                                   device.stream()), "pbh_histogram2d")
    host = device.to_host(counts)  # (the read-back: the host tables above have been consumed)
    out, at = [], 0
    for a, b in shapes:
        out.append(host[at:at + a * b].reshape(a, b).copy())
        at += a * b
    return out


def binned_sums(cols, edges, pairs, centres, ws_bytes=None):
    """[(count int64[b], s1 float64[b], s2 float64[b])] per (i, j) of `pairs`, in one launch
    (pbh_binned_sums): over the b bins of edges[i], the rows of cols[i] in the bin (np.histogram's
    counts) and the sums of cols[j] - centres[j] and of its square over those rows.  cols: float64
    device vectors of one length; edges: one host edge array per column, None (or an empty one) for
    a column that only gives values; an axis is uniform when its edges equal
    np.linspace(e[0], e[-1], len(e)) bit for bit; centres: one float per column.  The sums come
    from atomics and change in their last bits from run to run.  ws_bytes: the workspace to
    allocate and state instead of pbh_binned_sums_workspace_size's."""
    import ctypes

    import torch

    lib = _lib.load()
    cols = list(cols)
    for x in cols:
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.dim() != 1:
            raise TypeError("float64 device vectors are required")
        if x.shape[0] > 1 and x.stride(0) != 1:
            raise ValueError("the samples of a column must be contiguous")
    if len(edges) != len(cols):
        raise ValueError("binned_sums: one edge array (or None) per column is required")
    centres = np.ascontiguousarray(centres, dtype=np.float64).ravel()
    if len(centres) != len(cols):
        raise ValueError("binned_sums: one centre per column is required")
    if cols and any(x.shape[0] != cols[0].shape[0] for x in cols):
        raise ValueError("binned_sums: the columns hold different numbers of samples")
    k, n = len(cols), (cols[0].shape[0] if cols else 0)
    edges = [np.zeros(0) if e is None else np.ascontiguousarray(e, dtype=np.float64).ravel() for e in edges]
    if any(len(e) == 1 for e in edges):
        raise ValueError("binned_sums: a binning column needs at least two edges")
    bins = np.array([max(len(e) - 1, 0) for e in edges], dtype=np.int32)
    with np.errstate(all="ignore"):  # (non-finite ends: the library refuses them)
        uniform = np.array([len(e) > 0 and np.linspace(e[0], e[-1], len(e)).tobytes() == e.tobytes() for e in edges],
                           dtype=np.uint8)
    flat = np.concatenate(edges + [np.zeros(1)])  # (never empty: its pointer is not NULL)
    ptrs = np.array([x.data_ptr() for x in cols], dtype=np.uint64)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    if ws_bytes is None:
        b = ctypes.c_size_t()
        _lib.check(lib.pbh_binned_sums_workspace_size(k, _lib.np_ptr(bins), ctypes.byref(b)),
                   "pbh_binned_sums_workspace_size")
        ws_bytes = b.value
    ws = device.empty(max(int(ws_bytes), 8), "uint8")
    inside = (pr >= 0).all(axis=1) & (pr < k).all(axis=1)  # (the library refuses the others)
    sizes = [int(bins[i]) if ok else 0 for (i, _), ok in zip(pr.tolist(), inside.tolist())]
    total = max(sum(sizes), 1)
    counts, s1, s2 = device.empty(total, "int64"), device.empty(total), device.empty(total)
    _lib.check(lib.pbh_binned_sums(_lib.np_ptr(ptrs), k, n, _lib.np_ptr(flat), _lib.np_ptr(bins), _lib.np_ptr(uniform),
                                   _lib.np_ptr(centres), _lib.np_ptr(pr), len(pr), counts.data_ptr(), s1.data_ptr(),
                                   s2.data_ptr(), ws.data_ptr(), int(ws_bytes), device.stream()), "pbh_binned_sums")
    hc, h1, h2 = (device.to_host(t) for t in (counts, s1, s2))  # (the read-back: the host tables are consumed)
    out, at = [], 0
    for b in sizes:
        out.append((hc[at:at + b].copy(), h1[at:at + b].copy(), h2[at:at + b].copy()))
        at += b
    return out


def transpose(x_dev, rows, cols):
    out = device.empty((cols, rows))
    _lib.check(_lib.load().pbh_transpose(x_dev.data_ptr(), rows, cols, cols, out.data_ptr(), rows,
                                         device.stream()), "pbh_transpose")
    return out

