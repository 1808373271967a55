"""probabilit_amd.inspection's host side (no kernel is launched)."""

import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

TREE = """\
Subtract
├──Add
│  ├──Distribution("norm", loc=1, scale=Distribution("expon"))
│  │  └──Distribution("expon")
│  └──Distribution("expon")
└──Power
   ├──Distribution("expon")
   └──Constant(2)
"""


def test_treeprint(capsys):
    from probabilit_amd.inspection import treeprint
    from probabilit_amd.modeling import Distribution

    scale = Distribution("expon")
    a = Distribution("norm", loc=1, scale=scale)
    treeprint(a + scale - scale ** 2)
    assert capsys.readouterr().out == TREE


@pytest.mark.parametrize("method", ["linear", "lower", "higher", "nearest", "midpoint"])
def test_host_lerp_equals_np_quantile(method):
    from probabilit_amd.inspection import quantile_of_sorted

    rng = np.random.default_rng(5)
    fixed = np.array([0.0, 1.0, 0.5, 1 / 3, 1e-9])
    for trial in range(300):
        n = int(rng.integers(1, 400))
        x = np.sort(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4))
        q = np.concatenate([fixed, rng.random(6)])
        np.testing.assert_array_equal(quantile_of_sorted(x, q, method), np.quantile(x, q, method=method))
        assert quantile_of_sorted(x, 0.25, method) == np.quantile(x, 0.25, method=method)  # a scalar q
    x = np.array([1.0, 2.0, np.nan])
    assert np.isnan(quantile_of_sorted(x, fixed, method)).all() and np.isnan(np.quantile(x, fixed, method=method)).all()
    x = np.array([-np.inf, 1.0, np.inf])
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(quantile_of_sorted(x, fixed, method), np.quantile(x, fixed, method=method))


def test_quantile_arguments_are_validated():
    from probabilit_amd.inspection import quantile_indexes

    with pytest.raises(ValueError, match="range"):
        quantile_indexes(10, [0.5, 1.5])
    with pytest.raises(ValueError, match="method"):
        quantile_indexes(10, [0.5], "hazen")


def test_plot_forwards_to_the_package(monkeypatch):
    import probabilit_amd
    from probabilit_amd import inspection

    with pytest.raises(NotImplementedError, match="plotting"):
        inspection.plot()
    monkeypatch.setattr(probabilit_amd, "plot", lambda *a, **k: ("forwarded", a, k))
    assert inspection.plot(1, x=2) == ("forwarded", (1,), {"x": 2})


def test_unsampled_node_raises_like_samples_():
    from probabilit_amd import inspection
    from probabilit_amd.modeling import Distribution

    node = Distribution("norm")
    with pytest.raises(AttributeError) as want:
        node.samples_
    for call in (inspection.summary, lambda nd: inspection.quantile(nd, 0.5), inspection.histogram,
                 inspection.corrcoef):
        with pytest.raises(AttributeError) as got:
            call(node)
        assert str(got.value) == str(want.value)


def test_module_imports_with_no_gpu_visible():
    code = ("import probabilit_amd.inspection as i, sys; "
            "assert 'torch' not in sys.modules or not sys.modules['torch'].cuda.is_initialized(); "
            "print(sorted(i.__all__))")
    import os

    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="",
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == str(sorted(["summary", "quantile", "histogram", "corrcoef", "treeprint", "plot"])).split()
