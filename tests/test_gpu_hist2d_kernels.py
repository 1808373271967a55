"""pbh_histogram2d alone, through probabilit_amd.native, against np.histogram2d on the host copy of
the same data, count for count: the launch boundaries of the row tiles (one row, the wave, the
block tile T, the grid's span G, a ragged million), columns that are separate allocations one
double off 16-byte alignment with poison around them, values on and next to every edge, repeated
edges, the bin shapes up to the caps, concentrated joint densities, 120 pairs in one launch, and
every refusal."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from probabilit_amd import native  # noqa: E402

T, G = native.SUMMARY_TILE, native.SUMMARY_SPAN
NS = [1, 2, 63, 64, 65, T - 1, T, T + 1, G + 1, 1_000_003]


def _correlated(n, k=2, seed=0, rho=0.7):
    z = np.random.default_rng(seed).standard_normal((k, n))
    for c in range(1, k):
        z[c] = rho * z[0] + np.sqrt(1.0 - rho * rho) * z[c]
    return z


BASE = _correlated(G + 1)  # the two correlated normal columns every size takes its rows from


def _place(gpu, col):
    """One column as an allocation of its own: three poison doubles, the column, two more, so that
    the column starts one double off 16-byte alignment and both neighbours of either end are poison
    (NaN and 1e300)."""
    import torch

    host = np.concatenate([[1e300, np.nan, 1e300], col, [1e300, np.nan]])
    buf = torch.from_numpy(host).to(gpu)
    view = buf[3:3 + len(col)]
    assert view.data_ptr() % 16 == 8
    return view


def _check(gpu, cols, edges, pairs=((0, 1),)):
    cols = [np.asarray(c, dtype=np.float64) for c in cols]
    edges = [np.asarray(e, dtype=np.float64) for e in edges]
    got = native.histogram2d([_place(gpu, c) for c in cols], edges, list(pairs))
    assert len(got) == len(pairs)
    for (i, j), H in zip(pairs, got):
        want = np.histogram2d(cols[i], cols[j], bins=(edges[i], edges[j]))[0]
        assert H.dtype == np.int64 and H.shape == want.shape == (len(edges[i]) - 1, len(edges[j]) - 1)
        assert np.array_equal(H, want), (i, j)
    return got


XE, YE = np.linspace(-1.0, 1.5, 8), np.linspace(-1.2, 0.9, 6)  # 7 x 5, rows outside on every side


@pytest.mark.parametrize("n", NS)
def test_sizes(gpu, n):
    x, y = BASE[0, :n], BASE[1, :n]
    if n > 64:
        assert (x < XE[0]).any() and (x > XE[-1]).any() and (y < YE[0]).any() and (y > YE[-1]).any()
    _check(gpu, [x, y], [XE, YE])


@pytest.mark.parametrize("n", [1, 65, T, T + 1])
def test_poison_around_the_columns_is_not_counted(gpu, n):
    """Ranges that reach 1e300 on both axes: a row read one before or one past the columns
    (1e300, 1e300) or (NaN, NaN) would land in the last cell."""
    e = np.array([-10.0, 0.0, 10.0, 1e300])
    H = _check(gpu, [BASE[0, :n], BASE[1, :n]], [e, np.linspace(-10.0, 1e300, 4)])[0]
    assert H.sum() == n and H[2].sum() == 0 and H[:, 2].sum() == 0


# ---------------------------------------------------------------- special values
U9 = np.linspace(-1.1, 2.3, 10)  # 9 uniform bins whose edges are not exact multiples of a step
NONUNI = np.array([-1.1, -0.3, 0.0, 0.0, 0.4, 0.4, 0.4, 1.7, 2.3])  # repeated edges, a zero among them


def _special(edges):
    return np.concatenate([[np.nan, np.inf, -np.inf, -0.0, 0.0, edges[0], edges[-1]], edges,
                           np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("kind", ["uniform", "nonuniform_repeated", "mixed"])
def test_special_values_on_each_axis(gpu, kind, axis):
    n = T + 65
    edges = {"uniform": [U9, U9], "nonuniform_repeated": [NONUNI, NONUNI[2:]], "mixed": [NONUNI, U9]}[kind]
    cols = _correlated(n, seed=3 + axis)
    sp = _special(edges[axis])
    at = np.random.default_rng(5).choice(n, len(sp), replace=False)
    cols[axis, at] = sp
    cols[1 - axis, at[::2]] = 0.25  # half of the planted rows surely inside the other axis
    _check(gpu, list(cols), edges)
    if kind == "mixed":  # and the pair the other way round: x uniform, y not
        _check(gpu, [cols[1], cols[0]], [edges[1], edges[0]])


def test_rows_on_repeated_edges(gpu):
    """Every row on a repeated edge value of both axes: numpy puts it after the last repeat."""
    n = T + 1
    rng = np.random.default_rng(8)
    x = rng.choice(NONUNI, n)
    y = rng.choice(NONUNI, n)
    H = _check(gpu, [x, y], [NONUNI, NONUNI])[0]
    assert H.sum() == n and H[2].sum() == 0 and H[4].sum() == 0 and H[5].sum() == 0  # zero-width bins stay empty


def test_last_edge_repeated(gpu):
    e = np.array([-1.0, 0.0, 1.0, 1.0])
    x = np.array([1.0, 1.0, 0.5, -1.0, np.nextafter(1.0, 2.0), 0.0] * 20)
    _check(gpu, [x, x[::-1].copy()], [e, e])


# ---------------------------------------------------------------- bin shapes
@pytest.mark.parametrize("shape", [(1, 1), (1, 1024), (1024, 1), (1024, 16), (128, 128), (3, 5)])
@pytest.mark.parametrize("uniform", [True, False])
def test_bin_shapes(gpu, shape, uniform):
    n = 3 * T + 7
    x, y = BASE[0, :n], BASE[1, :n]
    edges = [np.linspace(-2.5, 2.75, b + 1) for b in shape]
    if not uniform:
        edges = [np.concatenate([e[:1], np.sort(np.random.default_rng(b).uniform(-2.5, 2.75, b - 1)), e[-1:]])
                 for e, b in zip(edges, shape)]
    H = _check(gpu, [x, y], edges)[0]
    assert 0 < H.sum() < n


# ---------------------------------------------------------------- concentration
@pytest.mark.parametrize("n", [T + 1, G + 1])
@pytest.mark.parametrize("case", ["both_constant", "x_equals_y", "x_constant_y_spread"])
def test_concentrated_densities(gpu, case, n):
    e = np.linspace(-3.0, 3.0, 17)
    spread = BASE[1, :n]
    x, y = {"both_constant": (np.full(n, 0.3), np.full(n, -1.7)), "x_equals_y": (spread, spread),
            "x_constant_y_spread": (np.full(n, 0.3), spread)}[case]
    H = _check(gpu, [x, y], [e, e])[0]
    if case == "both_constant":
        assert H[8, 3] == n and H.sum() == n
    if case == "x_equals_y":
        assert H.sum() == np.trace(H) > 0


# ---------------------------------------------------------------- pairs
@pytest.mark.parametrize("n", [65, T + 1])
def test_sixteen_columns_all_pairs(gpu, n):
    k = 16
    cols = _correlated(n, k, seed=n) + 0.1 * np.arange(k)[:, None]
    bins = [(3, 4, 5, 8)[c % 4] for c in range(k)]
    edges = [np.linspace(-1.5 + 0.05 * c, 1.75, b + 1) if c % 3 else np.array([-2.0, *np.arange(b - 1) * 0.3, 2.0])
             for c, b in enumerate(bins)]
    pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]
    assert len(pairs) == native.HISTOGRAM2D_MAX_PAIRS
    _check(gpu, list(cols), edges, pairs)


def test_both_orders_of_a_pair(gpu):
    cols = _correlated(T + 1, 3, seed=2)
    edges = [XE, YE, NONUNI]
    pairs = [(0, 1), (1, 0), (2, 0), (0, 2), (1, 2), (2, 1), (0, 1)]
    got = _check(gpu, list(cols), edges, pairs)
    for a, b in ((0, 1), (2, 3), (4, 5)):
        assert np.array_equal(got[a], got[b].T)
    assert np.array_equal(got[0], got[6])


def test_same_call_twice(gpu):
    n = G + 1
    cols = [_place(gpu, BASE[0, :n]), _place(gpu, BASE[1, :n])]
    e = [np.linspace(-2.0, 2.0, 65), NONUNI]
    a = native.histogram2d(cols, e, [(0, 1), (1, 0)])
    b = native.histogram2d(cols, e, [(0, 1), (1, 0)])
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b)) and a[0].sum() > 0


# ---------------------------------------------------------------- refusals
def _edges(bins):
    return np.linspace(-2.0, 2.0, bins + 1)


REFUSALS = {
    "cells_over_the_cap": (dict(edges=[_edges(129), _edges(128)]), ValueError, "cells"),
    "bins_1025": (dict(edges=[_edges(1025), _edges(1)]), ValueError, "1024"),
    "k_17": (dict(k=17), ValueError, "columns"),
    "npairs_121": (dict(pairs=[(0, 1)] * 121), ValueError, "npairs"),
    "npairs_0": (dict(pairs=[]), ValueError, "npairs"),
    "pair_i_i": (dict(pairs=[(0, 1), (1, 1)]), ValueError, "twice"),
    "index_out_of_range": (dict(pairs=[(0, 2)]), ValueError, "outside"),
    "negative_index": (dict(pairs=[(-1, 0)]), ValueError, "outside"),
    "decreasing_edges": (dict(edges=[np.array([0.0, 2.0, 1.0, 3.0]), _edges(4)]), ValueError, "edges"),
    "non_finite_edge": (dict(edges=[_edges(4), np.array([0.0, 1.0, np.inf])]), ValueError, "finite"),
    "nan_edge": (dict(edges=[np.array([0.0, np.nan, 1.0]), _edges(4)]), ValueError, "finite"),
    "first_edge_equals_last": (dict(edges=[np.array([1.0, 1.0, 1.0]), _edges(4)]), ValueError, "increasing"),
    "workspace_too_small": (dict(ws_bytes=64), MemoryError, "workspace"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_launch_nothing(gpu, case):
    """Host-side argument checks: the library's error through _lib.check, and a valid call right
    after gives the right counts."""
    n = 1000
    kw, error, text = REFUSALS[case]
    k = kw.get("k", 2)
    cols = [_place(gpu, BASE[c % 2, :n]) for c in range(k)]
    edges = kw.get("edges", [_edges(4)] * k)
    with pytest.raises(error, match=text):
        native.histogram2d(cols, edges, kw.get("pairs", [(0, 1)]), ws_bytes=kw.get("ws_bytes"))
    _check(gpu, [BASE[0, :n], BASE[1, :n]], [XE, YE])


def test_caps_mirror_the_header():
    import os
    import re

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "probabilit_hip.h")).read()
    for name in ("MAX_BINS", "MAX_CELLS", "MAX_COLUMNS", "MAX_PAIRS"):
        value = int(re.search(rf"#define PBH_HISTOGRAM2D_{name}\s+(\d+)", text).group(1))
        assert getattr(native, f"HISTOGRAM2D_{name}") == value
    assert native.HISTOGRAM2D_MAX_PAIRS == 16 * 15 // 2
