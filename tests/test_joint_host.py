"""The host side of probabilit_amd.inspection's joint histograms (no kernel is launched): numpy's
forms of `bins` / `range`, and PairGrid over plain numpy arrays."""

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

RNG = np.random.default_rng(11)
X, Y = RNG.standard_normal(500), 3.0 + 2.0 * RNG.standard_normal(500)
XE = np.array([-2.0, -0.5, -0.5, 0.25, 3.0])
YE = np.linspace(-1.1, 7.3, 10)

# (bins, range) in every form np.histogram2d takes
FORMS = {
    "default": (10, None),
    "int_with_ranges": (7, ((-1.0, 1.5), (0.0, 6.0))),
    "two_ints": ((7, 5), None),
    "two_ints_one_range": ((7, 5), (None, (0.0, 6.0))),
    "other_range_only": ((3, 4), ((-1.0, 1.0), None)),
    "one_edge_array_for_both": (np.array([-3.0, -1.0, 0.0, 0.5, 4.0]), None),
    "edge_list_for_both": ([-3, -1, 0, 4], None),
    "two_edge_arrays": ((XE, YE), None),
    "edges_and_int": ((XE, 6), None),
    "int_and_edges": ((6, YE), ((-2.0, 2.0), (100.0, 200.0))),  # (a range beside edges is ignored)
    "empty_range_is_widened": (4, ((1.0, 1.0), None)),
    "numpy_ints": ((np.int64(3), np.int32(4)), None),
}


def _limits(axis):
    v = (X, Y)[axis]
    return v.min(), v.max()


@pytest.mark.parametrize("form", list(FORMS))
def test_edges_are_numpys(form):
    from probabilit_amd.inspection import histogram2d_edges

    bins, rng = FORMS[form]
    _, xe, ye = np.histogram2d(X, Y, bins=bins, range=rng)
    got = histogram2d_edges(bins, rng, _limits)
    assert len(got) == 2
    assert got[0].tobytes() == xe.tobytes() and got[0].dtype == xe.dtype
    assert got[1].tobytes() == ye.tobytes() and got[1].dtype == ye.dtype


def test_limits_are_asked_only_for_an_axis_without_edges_or_range():
    from probabilit_amd.inspection import histogram2d_edges

    asked = []

    def limits(axis):
        asked.append(axis)
        return 0.0, 1.0

    histogram2d_edges((XE, 5), (None, (0.0, 1.0)), limits)
    assert asked == []
    histogram2d_edges((4, 5), ((0.0, 1.0), None), limits)
    assert asked == [1]


BAD = {
    "decreasing_edges": (([0.0, 2.0, 1.0], 5), None, "monotonically increasing"),
    "decreasing_edges_for_both": ([0.0, 2.0, 1.0, 3.0], None, "monotonically increasing"),
    "zero_bins": (0, None, "must be positive"),
    "negative_bins": ((5, -1), None, "must be positive"),
    "one_entry": ([5], None, "dimension of bins"),
    "two_dimensional_edges": ((np.zeros((2, 2)), 5), None, "scalar or 1d array"),
    "range_of_three": (5, ((0, 1), (0, 1), (0, 1)), "one entry per dimension"),
    "range_decreasing": (5, ((1.0, 0.0), None), "max must be larger than min"),
    "range_not_finite": (5, (None, (0.0, np.inf)), "supplied range of"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_parser_errors_are_numpys(case):
    from probabilit_amd.inspection import histogram2d_edges

    bins, rng, text = BAD[case]
    with pytest.raises(ValueError, match=text):
        np.histogram2d(X, Y, bins=bins, range=rng)
    with pytest.raises(ValueError, match=text):
        histogram2d_edges(bins, rng, _limits)


def test_non_finite_autodetected_range_and_non_integer_bins():
    from probabilit_amd.inspection import histogram2d_edges

    with pytest.raises(ValueError, match=r"autodetected range of \[nan, nan\] is not finite"):
        histogram2d_edges(5, None, lambda axis: (np.nan, np.nan))
    with pytest.raises(ValueError, match="autodetected range"):
        histogram2d_edges(5, ((0.0, 1.0), None), lambda axis: (0.0, np.inf))
    with pytest.raises(TypeError, match="must be an integer"):
        histogram2d_edges(5.5, None, _limits)
    with pytest.raises(TypeError, match="must be an integer"):
        np.histogram2d(X, Y, bins=5.5)


def test_pairgrid_edges():
    from probabilit_amd.inspection import pairgrid_edges

    cols = [X, Y, X + Y]

    def limits(axis):
        return cols[axis].min(), cols[axis].max()

    got = pairgrid_edges(3, 30, None, limits)
    for c, e in zip(cols, got):
        assert e.tobytes() == np.histogram(c, bins=30)[1].tobytes()
    got = pairgrid_edges(3, [3, 4, 5], [None, (0.0, 1.0), None], limits)
    want = [np.histogram(cols[0], bins=3)[1], np.linspace(0.0, 1.0, 5), np.histogram(cols[2], bins=5)[1]]
    for e, w in zip(got, want):
        assert e.tobytes() == w.tobytes()
    with pytest.raises(ValueError, match="one per node"):
        pairgrid_edges(3, [3, 4], None, limits)
    with pytest.raises(ValueError, match="one entry per node"):
        pairgrid_edges(3, 5, [None, None], limits)
    with pytest.raises(ValueError, match="must be positive"):
        pairgrid_edges(3, [3, 0, 5], None, limits)


# ---------------------------------------------------------------- PairGrid
def _grid(bins=(3, 4, 5)):
    from probabilit_amd.inspection import PairGrid

    cols = [X, Y, X * Y]
    edges = [np.histogram(c, bins=b)[1] for c, b in zip(cols, bins)]
    diagonal = [np.histogram(c, bins=e)[0] for c, e in zip(cols, edges)]
    joints = {(i, j): np.histogram2d(cols[i], cols[j], bins=(edges[i], edges[j]))[0].astype(np.int64)
              for i in range(3) for j in range(i + 1, 3)}
    return PairGrid(len(X), ["x", "y", "x*y"], edges, diagonal, joints), joints


def test_pairgrid_members_and_transposition():
    grid, joints = _grid()
    assert grid.count == 500 and grid.labels == ["x", "y", "x*y"]
    assert [len(e) for e in grid.edges] == [4, 5, 6] and [len(d) for d in grid.diagonal] == [3, 4, 5]
    for (i, j), m in joints.items():
        assert grid.joint(i, j) is m and grid.joint(i, j).shape == (len(grid.diagonal[i]), len(grid.diagonal[j]))
        assert np.array_equal(grid.joint(j, i), m.T) and grid.joint(j, i).shape == m.shape[::-1]
        assert np.array_equal(grid.joint(i, j).sum(axis=1), grid.diagonal[i])
        assert np.array_equal(grid.joint(i, j).sum(axis=0), grid.diagonal[j])
    for i in range(3):
        with pytest.raises(ValueError, match="diagonal"):
            grid.joint(i, i)
    with pytest.raises(IndexError):
        grid.joint(0, 3)
    with pytest.raises(IndexError):
        grid.joint(-1, 0)


def test_draw():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.collections import QuadMesh

    grid, _ = _grid()
    fig = grid.draw(cmap="viridis")
    try:
        assert len(fig.axes) == 9
        axes = np.array(fig.axes).reshape(3, 3)
        for i in range(3):
            for j in range(3):
                ax = axes[i, j]
                meshes = [c for c in ax.collections if isinstance(c, QuadMesh)]
                if i == j:
                    assert not meshes and len(ax.patches) == len(grid.diagonal[i])
                    assert [p.get_height() for p in ax.patches] == grid.diagonal[i].tolist()
                else:
                    assert len(meshes) == 1 and not ax.patches
                    assert np.array_equal(np.asarray(meshes[0].get_array()).reshape(grid.joint(i, j).shape),
                                          grid.joint(i, j))
                assert ax.get_xlabel() == (grid.labels[j] if i == 2 else "")
                assert ax.get_ylabel() == (grid.labels[i] if j == 0 else "")
        mine = plt.figure()
        assert grid.draw(fig=mine) is mine and len(mine.axes) == 9
    finally:
        plt.close("all")


def test_draw_without_matplotlib_says_so(monkeypatch):
    grid, _ = _grid()
    monkeypatch.setitem(sys.modules, "matplotlib", None)
    monkeypatch.setitem(sys.modules, "matplotlib.pyplot", None)
    with pytest.raises(ImportError, match="needs matplotlib"):
        grid.draw()


def test_new_names_import_with_no_gpu_visible():
    code = ("import probabilit_amd.inspection as i, sys; "
            "assert 'torch' not in sys.modules or not sys.modules['torch'].cuda.is_initialized(); "
            "print(callable(i.histogram2d), callable(i.pairgrid), isinstance(i.PairGrid, type), "
            "all(n in i.__doc__ for n in ('histogram2d', 'pairgrid', 'PairGrid')))")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="",
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["True", "True", "True", "True"]


def test_unsampled_nodes_raise_like_samples_():
    from probabilit_amd import inspection
    from probabilit_amd.modeling import Distribution

    a, b = Distribution("norm"), Distribution("norm")
    with pytest.raises(AttributeError) as want:
        a.samples_
    for call in (lambda: inspection.histogram2d(a, b), lambda: inspection.pairgrid(a, b)):
        with pytest.raises(AttributeError) as got:
            call()
        assert str(got.value) == str(want.value)
