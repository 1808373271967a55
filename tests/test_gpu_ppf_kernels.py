"""The inverse-CDF sweep kernels behind pbh_ppf / pbh_lhs_ppf / pbh_sobol_ppf, called through the
C ABI at their own launch boundaries.

Which kernel a call takes (launch_ppf / launch_lhs_ppf / launch_ext), its tile T and grid cap G:

    norm, lognorm                       k_ppf_c<D, SC>                         2048   8192
    uniform, triang, expon, q and out   k_ppf_v                                2048   2048
      16-byte aligned, stride 1
    the same, any other geometry        k_ppf                                   256   4096
    gamma, scalar parameters            k_ppf_gamma_w + k_ppf_gamma_slow       2048    768
      (PBH_GAMMA_WIN=0)                 k_ppf_gamma_lds                        4096    256
    gamma, a per-row loc                k_ppf (global guide table)              256   4096
    poisson, scalar mu, short table     k_ppf_poisson_lds + k_ppf_poisson_slow 1024   2048
    poisson, mu = 1e5                   k_ppf (global CDF table)                256   4096
    weibull_min, beta, binom, ...       k_ppf_ext<D, LHS>                       256  16384

q is a view at element offset qo with stride qs inside a buffer of NaN sentinels, out lies at
offset oo between 4096 sentinels on each side, per-row parameters are device vectors followed by
sentinels (abi_views.py), and the flag word starts at 0.  References: scipy's ppf of the same
(q_i, params_i) within 1e-10 relative for continuous distributions, exactly for discrete ones; bit
for bit between the kernel variants of one distribution.  At the sizes past G x T the quantiles
tile a pattern of 4099, and so does the reference.

The poisson sweep answers q = 0 and q = 1 itself (poisson_ppf_fast); what it lists for
k_ppf_poisson_slow are the quantiles in scipy's window just above a CDF value and the deep tail
below 1e-150, so the slow-list cases fill the list with those, and keep 0 and 1 among the rest.
"""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from abi_views import Flag, View, tile_to, tiles_equal_first
from conftest import assert_close

pytestmark = pytest.mark.gpu

PERIOD = 4099
DISCRETE = {"poisson", "binom", "nbinom", "betabinom", "hypergeom"}
COMBOS = [(qo, oo, qs) for qs in (1, 3) for qo, oo in ((0, 0), (1, 0), (0, 1), (1, 1))]
ROW_LOC = "row_loc"  # marks a per-row loc vector in a case's parameters


def scipy_ppf(name, q, vals):
    import scipy.stats

    with np.errstate(all="ignore"):
        return np.asarray(getattr(scipy.stats, name).ppf(q, *vals), dtype=np.float64)


def param_values(name, kw):
    from probabilit_amd.modeling import _parse_scipy_args

    return _parse_scipy_args(name, (), kw)


def pack_params(vals, n, qs=1):
    """pbh_param[]: scalars by value, vectors (host arrays or device tensors of length n) as device
    views followed by sentinels, so that an index i * q_stride or row0 + i reads a NaN."""
    from probabilit_amd import _lib

    keep, out = [], []
    for v in vals:
        if np.ndim(v) == 0 and not hasattr(v, "data_ptr"):
            out.append(_lib.Param(None, float(v)))
        else:
            view = View(n, 0, 1, v, tail=n * max(qs - 1, 1) if n <= (1 << 20) else 0)
            keep.append(view)
            out.append(_lib.Param(view.ptr.value, 0.0))
    return (_lib.Param * max(len(out), 1))(*out), len(out), keep


class Result:
    def __init__(self, out, flag, status, inputs):
        self.view, self.flag, self.status = out, flag, status
        self.intact = out.intact() and all(v.intact() for v in inputs)

    @functools.cached_property
    def out(self):
        return self.view.host()

    @property
    def bits(self):
        return self.out.view(np.int64)


def call_ppf(name, vals, q, n=None, qo=0, qs=1, oo=0, with_flag=True, nparams=None, dist=None, null_params=False):
    """pbh_ppf on q (host array or device tensor) through the sentinel views."""
    from probabilit_amd import _lib, device

    n = len(q) if n is None else n
    qv, ov = View(n, qo, qs, q), View(n, oo, 1)
    arr, k, keep = pack_params(vals, n, qs)
    flag = Flag() if with_flag else None
    st = _lib.load().pbh_ppf(_lib.DIST_IDS[name] if dist is None else dist, qv.ptr, qs, n, None if null_params else arr,
                             k if nparams is None else nparams, ov.ptr, flag.ptr if flag else None, device.stream())
    device.synchronize()
    return Result(ov, flag.value() if flag else None, st, [qv] + keep)


def call_lhs_ppf(name, vals, seed, n_total, row0, nrows, col, oo=0, with_flag=True):
    from probabilit_amd import _lib, device

    ov = View(nrows, oo, 1)
    arr, k, keep = pack_params(vals, nrows, 2)
    flag = Flag() if with_flag else None
    st = _lib.load().pbh_lhs_ppf(seed, n_total, row0, nrows, col, _lib.DIST_IDS[name], arr, k, ov.ptr,
                                 flag.ptr if flag else None, device.stream())
    device.synchronize()
    return Result(ov, flag.value() if flag else None, st, keep)


def lhs_column(seed, n_total, row0, nrows, col):
    from probabilit_amd import native

    return np.ascontiguousarray(native.fill_lhs(seed, n_total, col + 1, row0=row0, nrows=nrows)[:, col])


def check_values(name, got, ref, what=""):
    if name in DISCRETE:
        np.testing.assert_array_equal(got, ref, err_msg=what)
    else:
        assert_close(got, ref, rtol=1e-10, what=what)


# ---------------------------------------------------------------------------- geometry
# name, parameters, tile, grid cap (read from launch_ppf / launch_ext)
GEOMETRY = {
    "norm": ("norm", {"loc": 1.11, "scale": 0.15}, 2048, 8192),
    "norm_rowloc": ("norm", {"loc": ROW_LOC, "scale": 0.15}, 2048, 8192),
    "lognorm": ("lognorm", {"s": 0.5, "scale": 2.0}, 2048, 8192),
    "lognorm_rowloc": ("lognorm", {"s": 0.5, "loc": ROW_LOC}, 2048, 8192),
    "uniform": ("uniform", {"loc": -1.0, "scale": 3.0}, 2048, 2048),
    "triang": ("triang", {"c": 0.3, "loc": 1.0, "scale": 2.0}, 2048, 2048),
    "expon": ("expon", {"scale": 2.5}, 2048, 2048),
    "gamma": ("gamma", {"a": 2.0}, 2048, 768),
    "gamma_rowloc": ("gamma", {"a": 2.0, "loc": ROW_LOC}, 256, 4096),
    "poisson": ("poisson", {"mu": 4.0}, 1024, 2048),
    "poisson_1e5": ("poisson", {"mu": 1e5}, 256, 4096),
    "weibull_min": ("weibull_min", {"c": 1.5}, 256, 16384),
    "beta": ("beta", {"a": 2.0, "b": 3.0}, 256, 16384),
    "binom": ("binom", {"n": 50, "p": 0.4}, 256, 16384),
}


@functools.lru_cache(maxsize=None)
def pattern():
    rng = np.random.default_rng(4099)
    q, loc = rng.uniform(1e-6, 1.0 - 1e-6, PERIOD), rng.uniform(-2.0, 2.0, PERIOD)
    q.setflags(write=False)
    loc.setflags(write=False)
    return q, loc


@functools.lru_cache(maxsize=None)
def pattern_reference(case):
    name, kw, _, _ = GEOMETRY[case]
    q, loc = pattern()
    ref = scipy_ppf(name, q, param_values(name, {k: (loc if v is ROW_LOC else v) for k, v in kw.items()}))
    ref.setflags(write=False)
    return ref


def geometry_values(case, n, on_device=False):
    """(q, parameter values) of n rows: the pattern and its per-row loc, tiled."""
    name, kw, _, _ = GEOMETRY[case]
    q, loc = pattern()
    tile = (lambda a: tile_to(a, n)) if on_device else (lambda a: np.resize(a, n))
    return tile(q), param_values(name, {k: (tile(loc) if v is ROW_LOC else v) for k, v in kw.items()})


@pytest.mark.parametrize("case", list(GEOMETRY))
def test_ppf_geometry(gpu, case):
    """n = 1, T - 1, T, T + 1: values, sentinels and flag == 0 at every offset / stride combination;
    every combination gives the bits of the first (for uniform, triang and expon that is k_ppf_v
    against k_ppf)."""
    T = GEOMETRY[case][2]
    for n in (1, T - 1, T, T + 1):
        geometry_case(case, n)


def geometry_case(case, n):
    name = GEOMETRY[case][0]
    q, vals = geometry_values(case, n)
    ref = np.resize(pattern_reference(case), n)
    first = None
    for qo, oo, qs in COMBOS:
        r = call_ppf(name, vals, q, qo=qo, qs=qs, oo=oo)
        what = f"{case} n={n} qo={qo} oo={oo} qs={qs}"
        assert r.status == 0, what
        check_values(name, r.out, ref, what)
        assert r.intact, what
        assert r.flag == 0, what
        if first is None:
            first = r.bits
        np.testing.assert_array_equal(r.bits, first, err_msg=what + ": not the bits of (0, 0, 1)")


@pytest.mark.parametrize("qo,oo,qs", [(0, 0, 1), (1, 1, 3)])
@pytest.mark.parametrize("case", list(GEOMETRY))
def test_ppf_second_grid_trip(gpu, case, qo, oo, qs):
    """n = G T + T + 77: every block takes a second grid-stride trip (the one-trip-ahead prefetch
    of k_ppf_gamma_w reads real rows), the last tile is ragged.  For uniform, triang and expon the
    second combination runs k_ppf past its own cap of 4096 x 256."""
    name, _, T, G = GEOMETRY[case]
    n = G * T + T + 77
    q, vals = geometry_values(case, n, on_device=True)
    r = call_ppf(name, vals, q, n=n, qo=qo, qs=qs, oo=oo)
    assert r.status == 0 and r.flag == 0
    dev = r.view.dev()
    assert tiles_equal_first(dev, PERIOD), "a row differs from the same quantile's first occurrence"
    check_values(name, dev[:PERIOD].cpu().numpy().view(np.float64), pattern_reference(case), case)
    assert r.intact


# ---------------------------------------------------------------------------- per-row parameters
def row_parameters(name, n, rng):
    u = lambda lo, hi: rng.uniform(lo, hi, n)  # noqa: E731
    return {
        "norm": {"loc": u(-3, 3), "scale": u(0.5, 2)},
        "lognorm": {"s": u(0.2, 1.5), "loc": u(-1, 1), "scale": u(0.5, 2)},
        "triang": {"c": u(0.05, 0.95), "loc": u(-1, 1), "scale": u(0.5, 2)},
        "gamma": {"a": u(0.3, 20), "loc": u(-1, 1), "scale": u(0.5, 2)},
        "poisson": {"mu": u(0.2, 300), "loc": np.floor(u(-3, 3))},
        "beta": {"a": u(0.5, 8), "b": u(0.5, 8), "loc": u(-1, 1), "scale": u(0.5, 2)},
        "nbinom": {"n": np.floor(u(1, 40)), "p": u(0.05, 0.95), "loc": np.floor(u(-3, 3))},
    }[name]


@pytest.mark.parametrize("name", ["norm", "lognorm", "triang", "gamma", "poisson", "beta", "nbinom"])
def test_every_parameter_per_row_with_stride(gpu, name):
    """Params::at(j, i) takes the row i, not i * q_stride: every parameter a vector, q_stride 3."""
    n = 2049 + 300
    rng = np.random.default_rng(len(name))
    q = rng.uniform(1e-4, 1.0 - 1e-4, n)
    vals = param_values(name, row_parameters(name, n, rng))
    r = call_ppf(name, vals, q, qo=1, qs=3, oo=1)
    assert r.status == 0 and r.flag == 0
    check_values(name, r.out, scipy_ppf(name, q, vals), name)
    assert r.intact


@pytest.mark.parametrize("name", ["norm", "lognorm", "triang", "gamma", "poisson", "beta", "nbinom"])
def test_lhs_ppf_per_row_parameters_with_row0(gpu, name):
    """pbh_lhs_ppf indexes per-row parameters by the local row, not row0 + i."""
    seed, n_total, row0, nrows, col = 5, 10_000, 777, 5001, 2
    rng = np.random.default_rng(100 + len(name))
    vals = param_values(name, row_parameters(name, nrows, rng))
    r = call_lhs_ppf(name, vals, seed, n_total, row0, nrows, col, oo=1)
    assert r.status == 0 and r.flag == 0
    check_values(name, r.out, scipy_ppf(name, lhs_column(seed, n_total, row0, nrows, col), vals), name)
    assert r.intact


# ---------------------------------------------------------------------------- the non-finite flag
UNBOUNDED = {"norm", "lognorm", "expon", "gamma", "gamma_rowloc", "poisson", "poisson_1e5", "weibull_min"}


@pytest.mark.parametrize("case", list(GEOMETRY))
def test_flag_one_nonfinite_output(gpu, case):
    """flag == 0 for finite outputs; exactly one non-finite output (q = 1 of an unbounded support,
    else a NaN q) gives flag == 1 wherever it sits: element 0, the ragged end past the last whole
    tile (k_ppf_v's scalar loop), the last element, which is a lane of a partly filled wave; for
    gamma q = 1 is a slow-list row.  A NULL flag is accepted."""
    name, _, T, _ = GEOMETRY[case]
    n = T + 100
    q, vals = geometry_values(case, n)
    base = call_ppf(name, vals, q)
    assert base.status == 0 and base.flag == 0 and base.intact and np.isfinite(base.out).all()
    bad_q = [np.nan] + ([1.0] if case in UNBOUNDED else [])
    for pos in (0, T - 1, T + 5, n - 1):
        for bq in bad_q:
            q2 = q.copy()
            q2[pos] = bq
            r = call_ppf(name, vals, q2)
            what = f"{case} q[{pos}] = {bq}"
            assert r.status == 0 and r.intact, what
            assert not np.isfinite(r.out[pos]), what
            keep = np.arange(n) != pos
            np.testing.assert_array_equal(r.bits[keep], base.bits[keep], err_msg=what)
            assert r.flag == 1, what
    r = call_ppf(name, vals, q, with_flag=False)
    assert r.status == 0 and r.intact
    np.testing.assert_array_equal(r.bits, base.bits)


# ---------------------------------------------------------------------------- slow lists
N_SLOW = 8192
SLOW_CAP = {"gamma": (N_SLOW >> 8) + 4096, "poisson": (N_SLOW >> 10) + 4096}


def slow_quantiles(name, n_slow, rng):
    """n quantiles of which exactly n_slow go to the slow list, scattered by a seeded permutation."""
    import scipy.special

    if name == "gamma":  # outside |log(q / (1 - q))| < 19.9, or 0 or 1
        slow = np.array([0.0, 1.0, 1e-12, 1.0 - 1e-13])
        fast = rng.uniform(0.01, 0.99, N_SLOW)
    else:  # scipy's window just above a CDF value, and the deep tail; 0 and 1 are answered at once
        cdf = scipy.special.pdtr(np.arange(14.0), 4.0)
        slow = np.concatenate([np.nextafter(cdf[:10], 1.0), [1e-200]])
        fast = rng.choice(np.concatenate([0.5 * (cdf[:-1] + cdf[1:]), [0.0, 1.0]]), N_SLOW)
    q = fast
    where = rng.permutation(N_SLOW)[:n_slow]
    q[where] = slow[rng.integers(0, len(slow), n_slow)]
    return q


@pytest.mark.parametrize("count", ["0", "1", "cap-1", "cap", "cap+1", "n"])
@pytest.mark.parametrize("name", ["gamma", "poisson"])
def test_slow_list_boundaries(gpu, name, count):
    """The list holds cap entries; one more makes the slow kernel redo every row.  Compared with
    scipy and, bit for bit, with the same q sent with a per-row loc (k_ppf: no slow list);
    q_stride 1 and 3."""
    for qs in (1, 3):
        slow_list_case(name, count, qs)


def slow_list_case(name, count, qs):
    cap = SLOW_CAP[name]
    n_slow = {"0": 0, "1": 1, "cap-1": cap - 1, "cap": cap, "cap+1": cap + 1, "n": N_SLOW}[count]
    q = slow_quantiles(name, n_slow, np.random.default_rng(cap + n_slow))
    kw = {"a": 2.0, "loc": 0.5} if name == "gamma" else {"mu": 4.0, "loc": 1.0}
    vals = param_values(name, kw)
    ref = scipy_ppf(name, q, vals)
    r = call_ppf(name, vals, q, qo=1, qs=qs, oo=1)
    assert r.status == 0 and r.intact
    check_values(name, r.out, ref, f"{name} {count} qs={qs}")
    assert r.flag == (0 if np.isfinite(ref).all() else 1)
    rows = param_values(name, dict(kw, loc=np.full(N_SLOW, kw["loc"])))
    g = call_ppf(name, rows, q, qo=1, qs=qs, oo=1)
    assert g.status == 0 and g.intact and g.flag == r.flag
    np.testing.assert_array_equal(r.bits, g.bits)


def test_lhs_gamma_slow_list(gpu):
    """pbh_lhs_ppf, a = 0.05 over 2^20 rows: the slow list the LHS quantiles themselves fill."""
    seed, n, col = 3, 1 << 20, 1
    vals = param_values("gamma", {"a": 0.05})
    r = call_lhs_ppf("gamma", vals, seed, n, 0, n, col)
    assert r.status == 0 and r.intact
    assert_close(r.out, scipy_ppf("gamma", lhs_column(seed, n, 0, n, col), vals), rtol=1e-10, what="lhs gamma a=0.05")
    g = call_lhs_ppf("gamma", param_values("gamma", {"a": 0.05, "loc": np.zeros(n)}), seed, n, 0, n, col)
    assert g.status == 0
    np.testing.assert_array_equal(r.bits, g.bits)


# ---------------------------------------------------------------------------- norm / lognorm tail queue
@pytest.mark.parametrize("kind", ["centre", "tail", "alternating", "cancel"])
@pytest.mark.parametrize("name", ["norm", "lognorm"])
def test_tail_queue_tiles(gpu, name, kind):
    """Tiles with no element in PPND16's tail, every element (q < 1e-300), every other one, and
    every element next to the zero crossing of loc + scale z (per-row loc: Cephes' ndtri), at
    n = 2047, 2048, 2049."""
    for n in (2047, 2048, 2049):
        tail_queue_case(name, kind, n)


def tail_queue_case(name, kind, n):
    import scipy.special

    rng = np.random.default_rng(n)
    centre, tail = rng.uniform(0.2, 0.8, n), rng.uniform(1e-305, 1e-300, n)
    kw = {"loc": 1.5, "scale": 2.0} if name == "norm" else {"s": 0.5, "loc": 1.5, "scale": 2.0}
    if kind == "centre":
        q = centre
    elif kind == "tail":
        q = tail
    elif kind == "alternating":
        q = np.where(np.arange(n) % 2 == 0, centre, tail)
    else:
        q = rng.uniform(0.01, 0.99, n)
        z = scipy.special.ndtri(q)
        v = 2.0 * z if name == "norm" else 2.0 * np.exp(0.5 * z)
        kw["loc"] = -v * (1.0 + 2.0 ** -14)
    vals = param_values(name, kw)
    r = call_ppf(name, vals, q, qo=1, qs=3, oo=1)
    assert r.status == 0 and r.intact and r.flag == 0
    assert_close(r.out, scipy_ppf(name, q, vals), rtol=1e-10, what=f"{name} {kind} {n}")


# ---------------------------------------------------------------------------- PBH_GAMMA_WIN=0
def gamma_lds_cases():
    """name -> (entry, arguments): what k_ppf_gamma_lds / k_lhs_ppf_gamma_lds run in the child."""
    rng = np.random.default_rng(40)
    cases = {}
    for n in (1, 4095, 4096, 4097, 256 * 4096 + 4096 + 77):
        for qo, oo, qs in ((0, 0, 1), (1, 1, 3)):
            cases[f"geometry_{n}_{qo}{oo}{qs}"] = ("ppf", n, None, qo, oo, qs)
    slow = np.array([0.0, 1e-12, 1.0 - 1e-13])
    for n, counts in ((2 * 4096, (2047, 2048, 2049, 4096)), (4096 + 100, (4096,))):
        for c in counts:  # the first tile holds c slow draws (2049 and 4096 overflow kQCap = 2048)
            q = rng.uniform(0.01, 0.99, n)
            q[rng.permutation(4096)[:c]] = slow[rng.integers(0, len(slow), c)]
            if n == 4096 + 100:
                q[4096:] = 1e-12  # and the ragged last tile is all slow
            cases[f"slow_{n}_{c}"] = ("ppf", n, q, 1, 1, 3)
    cases["lhs"] = ("lhs", 5001, None, 0, 1, 1)
    cases["lhs_large"] = ("lhs", 256 * 1024 + 1024 + 77, None, 0, 0, 1)
    return cases


def gamma_lds_outputs():
    vals = param_values("gamma", {"a": 2.0, "loc": 0.5, "scale": 1.5})
    out = {}
    for key, (entry, n, q, qo, oo, qs) in gamma_lds_cases().items():
        if entry == "lhs":
            r = call_lhs_ppf("gamma", vals, 9, 2 * n + 1000, 777, n, 1, oo=oo)
        else:
            r = call_ppf("gamma", vals, tile_to(pattern()[0], n) if q is None else q, n=n, qo=qo, qs=qs, oo=oo)
        assert r.status == 0 and r.intact, key
        expect_flag = 0 if q is None or np.isfinite(scipy_ppf("gamma", q, vals)).all() else 1
        assert r.flag == expect_flag, (key, r.flag)
        out[key] = r.bits
    return out


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_ppf_kernels as t
np.savez({path!r}, **t.gamma_lds_outputs())
"""


def test_gamma_lds_kernels_in_a_fresh_process(gpu, tmp_path):
    """PBH_GAMMA_WIN=0 (read once per process) sends scalar gamma to k_ppf_gamma_lds and
    k_lhs_ppf_gamma_lds: tiles of 4096, the per-tile slow queue of kQCap = 2048 and its overflow,
    the second grid-stride trip with its prefetch.  Same function, same values: the bits of the
    default process (the window sweep)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "lds.npz")
    script = _CHILD.format(root=root, tests=os.path.join(root, "tests"), path=path)
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, "PBH_GAMMA_WIN": "0"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    here = gamma_lds_outputs()
    with np.load(path) as there:
        assert sorted(there.files) == sorted(here)
        for key in here:
            np.testing.assert_array_equal(there[key], here[key], err_msg=key)


# ---------------------------------------------------------------------------- k_ppf_ext's LDS table
def nbinom_p_for_length(length, n=5.0):
    """p with nbinom.ppf(1 - 2^-40, n, p) + 1 == length (how discrete_table_len sizes the table)."""
    import scipy.stats

    lo, hi = 1e-3, 0.999
    for _ in range(200):
        p = 0.5 * (lo + hi)
        top = scipy.stats.nbinom.ppf(1.0 - 2.0 ** -40, n, p) + 1
        if top == length:
            return p
        lo, hi = (p, hi) if top > length else (lo, p)
    raise AssertionError(f"no p for a table of {length}")


@pytest.mark.parametrize("length", [511, 512, 513])
@pytest.mark.parametrize("name", ["binom", "nbinom", "betabinom", "hypergeom"])
def test_ext_lds_table_lengths(gpu, name, length):
    """The CDF table staged in LDS up to kExtLdsTab = 512 entries, read from global memory above.
    The quantiles stop at 1 - 2^-41 (one step past the end of nbinom's table): within an ulp of 1
    the answer turns on CDF values that doubles next to 1 cannot tell apart, and scipy's own
    differ from the table's there (measured at q = 1 - 2^-53: hypergeom(2000, 1000, 511) 335
    against scipy's 334; nbinom(5, p) 639 / 640 / 641 against scipy's 648 / 649 / 650, which
    come from the complement)."""
    kw = {"binom": {"n": length - 1, "p": 0.3}, "betabinom": {"n": length - 1, "a": 2.0, "b": 3.0},
          "hypergeom": {"M": 2000, "n": 1000, "N": length - 1}}.get(name)
    if kw is None:
        kw = {"n": 5.0, "p": nbinom_p_for_length(length)}
    rng = np.random.default_rng(length)
    q = np.concatenate([rng.uniform(0.0, 1.0, 3000), [0.0, 1e-300, 2.0 ** -40, 1.0 - 2.0 ** -40, 1.0 - 2.0 ** -41]])
    vals = param_values(name, kw)
    ref = scipy_ppf(name, q, vals)
    r = call_ppf(name, vals, q, qo=1, qs=3, oo=1)
    assert r.status == 0 and r.intact and r.flag == 0
    np.testing.assert_array_equal(r.out, ref)
    g = call_ppf(name, param_values(name, dict(kw, loc=np.zeros(len(q)))), q, qo=1, qs=3, oo=1)
    assert g.status == 0 and g.intact
    np.testing.assert_array_equal(r.bits, g.bits)


# ---------------------------------------------------------------------------- pbh_sobol_ppf
SOBOL_DISTS = [("norm", {"loc": 1.11, "scale": 0.15}), ("uniform", {"loc": -1.0, "scale": 3.0}), ("expon", {}),
               ("lognorm", {"s": 0.5}), ("triang", {"c": 0.3}), ("gamma", {"a": 2.0}), ("poisson", {"mu": 4.0})]


def call_sobol_ppf(dist, vals, sv, shift, d, bits, row0, n, col):
    from probabilit_amd import _lib, device

    ov, flag = View(n, 1, 1), Flag()
    arr, k, _ = pack_params(vals, n)
    st = _lib.load().pbh_sobol_ppf(_lib.np_ptr(sv), _lib.np_ptr(shift), d, bits, row0, n, col, dist, arr, k, ov.ptr,
                                   flag.ptr, device.stream())
    device.synchronize()
    return ov, flag.value(), st


@pytest.mark.parametrize("name,kw", SOBOL_DISTS, ids=[d[0] for d in SOBOL_DISTS])
def test_sobol_ppf_is_fill_then_ppf(gpu, name, kw):
    """row0 = 0 and 12345, n = 1 and 2049."""
    for row0 in (0, 12345):
        for n in (1, 2049):
            sobol_case(name, kw, row0, n)


def sobol_case(name, kw, row0, n):
    from probabilit_amd import _lib, native, qmc

    d, bits, col = 6, 30, 4
    sv, shift = qmc.sobol_setup(d, 5)
    sv, shift = np.ascontiguousarray(sv, np.uint32), np.ascontiguousarray(shift, np.uint32)
    q = np.ascontiguousarray(native.fill_sobol(sv, shift, n, bits=bits, row0=row0)[:, col])
    vals = param_values(name, kw)
    want = call_ppf(name, vals, q)
    ov, flag, st = call_sobol_ppf(_lib.DIST_IDS[name], vals, sv, shift, d, bits, row0, n, col)
    assert st == 0 and ov.intact() and flag == want.flag, (row0, n)
    np.testing.assert_array_equal(ov.host().view(np.int64), want.bits, err_msg=f"row0={row0} n={n}")


def test_sobol_ppf_rejects_extended_distributions(gpu):
    from probabilit_amd import _lib, qmc

    sv, shift = qmc.sobol_setup(6, 5)
    sv, shift = np.ascontiguousarray(sv, np.uint32), np.ascontiguousarray(shift, np.uint32)
    ov, flag, st = call_sobol_ppf(_lib.DIST_IDS["beta"], [2.0, 3.0, 0.0, 1.0], sv, shift, 6, 30, 0, 257, 4)
    assert st == _lib.ERR_UNSUPPORTED and _lib.last_error()
    assert ov.untouched() and flag == 0


# ---------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("case", ["nparams", "null_params", "unknown_id"])
def test_ppf_argument_errors(gpu, case):
    """For norm, gamma (pbh_ppf's own checks) and beta (launch_ext's)."""
    from probabilit_amd import _lib

    q = np.linspace(0.01, 0.99, 257)
    for name in ("norm", "gamma", "beta"):
        vals = param_values(name, {"a": 2.0} if name == "gamma" else {"a": 2.0, "b": 3.0} if name == "beta" else {})
        kw = {"nparams": dict(nparams=len(vals) + 1), "null_params": dict(null_params=True),
              "unknown_id": dict(dist=9999)}
        r = call_ppf(name, vals, q, **kw[case])
        assert r.status != 0 and _lib.last_error(), name
        assert r.view.untouched() and r.flag == 0, name
