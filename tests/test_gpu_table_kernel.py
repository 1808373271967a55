"""pbh_table_ppf alone (k_table_ppf<KIND, OUT>), against numpy on the host, exactly.

QUANTILE  np.quantile(sorted, q, method=) for the five methods; q at every node j / (m - 1) of the
          virtual index and one ulp either side, where floor / ceil / rint decide, at the half
          nodes (nearest's ties, the t >= 0.5 branch of _lerp) and at 0, 2^-53, 1 - 2^-53, 1.
INTERP    np.interp(q, xp, fp): q at every xp node and one ulp either side, outside the table, NaN;
          fp increasing, decreasing, constant, with +-inf at and next to the node q hits (numpy
          returns fp[j] for q == xp[j] before it forms a slope) and with slopes that overflow.
SEARCH    values[searchsorted(t0, q, 'right')], the index clamped to m - 1 and flag bit 2 set
          when some q >= t0[m - 1]; repeated cumulative values; int64 and float64 values; t1 NULL.

q is a strided view at an offset inside a buffer of NaN sentinels and out lies between 4096
sentinels on each side (abi_views.py); n runs over the block edges and one size past the grid cap
(16384 blocks of 256), whose reference is a tiled pattern.
"""

import numpy as np
import pytest

from abi_views import Flag, View, tile_to, tiles_equal_first

pytestmark = pytest.mark.gpu

INTERP, QUANTILE, SEARCH = 0, 1, 2
INT64, FLOAT64 = 1, 2
METHODS = ["linear", "lower", "higher", "nearest", "midpoint"]
N_GEOMETRY = [1, 255, 256, 257]
N_LARGE = (1 << 22) + 257  # 16384 blocks x 256 rows is the grid cap: a second grid-stride trip
PERIOD = 4099


def table_ppf(kind, q, t0, t1, method=0, out_dtype=FLOAT64, qo=0, qs=1, oo=0, m=None, with_flag=True, n=None):
    """One pbh_table_ppf call: (out view, flag value or None, status).  q: host array or device tensor."""
    from probabilit_amd import _lib, device

    n = len(q) if n is None else n
    qv = View(n, qo, qs, q)
    ov = View(n, oo, 1)
    t0d = View(len(t0), 0, 1, t0)
    t1d = View(len(t1), 0, 1, t1) if t1 is not None else None
    flag = Flag() if with_flag else None
    st = _lib.load().pbh_table_ppf(kind, qv.ptr, qs, n, t0d.ptr, t1d.ptr if t1d else None,
                                   len(t0) if m is None else m, method, out_dtype, ov.ptr,
                                   flag.ptr if flag else None, device.stream())
    device.synchronize()
    assert qv.intact() and t0d.intact() and (t1d is None or t1d.intact())
    return ov, (flag.value() if flag else None), st


def same_bits(actual, expected, what=""):
    a, e = np.asarray(actual), np.asarray(expected)
    if a.dtype == np.float64:  # NaN == NaN, and no -0.0 for 0.0
        np.testing.assert_array_equal(a, e, err_msg=what)
        z = e == 0.0
        np.testing.assert_array_equal(np.signbit(a[z]), np.signbit(e[z]), err_msg=what + " (sign of zero)")
    else:
        np.testing.assert_array_equal(a, e, err_msg=what)


def ulps(x):
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


# ---------------------------------------------------------------------------- QUANTILE
def quantile_qs(m):
    edge = np.array([0.0, 2.0 ** -53, 1.0 - 2.0 ** -53, 1.0])
    if m == 1:
        return np.concatenate([edge, [0.25, 0.5, 0.75]])
    j = np.arange(m, dtype=np.float64)
    nodes = j / (m - 1)
    half = (j[:-1] + 0.5) / (m - 1)
    return np.clip(np.concatenate([ulps(nodes), ulps(half), edge]), 0.0, 1.0)


def quantile_data(kind, m):
    rng = np.random.default_rng(1000 + m)
    if kind == "arange":
        a = np.arange(m) * 1.5
    elif kind == "gamma":
        a = rng.gamma(2.0, 3.0, size=m)
    elif kind == "repeats":
        a = np.floor(rng.gamma(2.0, 3.0, size=m))
    else:  # "nan": the sorted data end in a NaN
        a = rng.gamma(2.0, 3.0, size=m)
        a[-1] = np.nan
    return np.sort(a)


@pytest.mark.parametrize("data", ["arange", "gamma", "repeats", "nan"])
@pytest.mark.parametrize("m", [1, 2, 3, 8, 1001, 4097])
def test_quantile_nodes(gpu, m, data):
    """The five methods, q_stride 1 and 3."""
    a, q = quantile_data(data, m), quantile_qs(m)
    for method in METHODS:
        with np.errstate(invalid="ignore"):
            ref = np.quantile(a, q, method=method)
        for qs in (1, 3):
            what = f"{method} m={m} {data} qs={qs}"
            out, flag, st = table_ppf(QUANTILE, q, a, None, METHODS.index(method), qo=1, qs=qs, oo=1)
            assert st == 0, what
            same_bits(out.host(), ref, what)
            assert out.intact(), what
            assert flag == (0 if np.isfinite(ref).all() else 1), what


# ---------------------------------------------------------------------------- INTERP
def interp_xp(m):
    if m == 1:
        return np.array([0.5])
    if m == 2:
        return np.array([0.125, 0.875])
    rng = np.random.default_rng(50)
    return np.sort(np.concatenate([[0.0625, 0.9375], rng.uniform(0.0625, 0.9375, m - 2)]))


FP_KINDS = ["inc", "dec", "const", "inf_at", "ninf_at", "ninf_then_inf", "inf_run", "inf_ends", "overflow"]


def interp_fp(kind, m):
    j = np.arange(m, dtype=np.float64)
    fp = {"inc": 10.0 + 2.5 * j, "dec": 7.0 - 0.3 * j ** 2, "const": np.full(m, 4.25)}.get(kind)
    if fp is not None:
        return fp
    fp = 10.0 + 2.5 * j
    h = m // 2  # the node the quantiles hit from both sides
    if kind == "inf_at":
        fp[h] = np.inf
    elif kind == "ninf_at":
        fp[h] = -np.inf
    elif kind == "ninf_then_inf":
        fp[h] = -np.inf
        fp[min(h + 1, m - 1)] = np.inf
    elif kind == "inf_run":
        fp[h:h + 2] = np.inf
    elif kind == "inf_ends":
        fp[0], fp[-1] = -np.inf, np.inf
    else:  # differences of 2e308 overflow the slope
        fp = np.where(j % 2 == 0, 1e308, -1e308)
    return fp


def interp_qs(xp, nan):
    mid = 0.5 * (xp[:-1] + xp[1:])
    q = np.concatenate([ulps(xp), mid, [0.0, xp[0] * 0.5, 0.5 * (xp[-1] + 1.0), 1.0]])
    return np.concatenate([q, [np.nan]]) if nan else q


@pytest.mark.parametrize("kind", FP_KINDS)
@pytest.mark.parametrize("m", [1, 2, 50])
def test_interp_nodes(gpu, m, kind):
    """Without and with a NaN q, q_stride 1 and 3."""
    xp, fp = interp_xp(m), interp_fp(kind, m)
    for nan in (False, True):
        q = interp_qs(xp, nan)
        with np.errstate(invalid="ignore", over="ignore"):
            ref = np.interp(q, xp, fp)
        for qs in (1, 3):
            what = f"interp m={m} {kind} nan_q={nan} qs={qs}"
            out, flag, st = table_ppf(INTERP, q, xp, fp, qo=1, qs=qs, oo=1)
            assert st == 0, what
            same_bits(out.host(), ref, what)
            assert out.intact(), what
            assert flag == (0 if np.isfinite(ref).all() else 1), what


def test_interp_numpy_exact_node_examples(gpu):
    """The two examples of numpy's early return for q == xp[j] (arr_interp): the slope times 0 is
    NaN and the retry from the right is inf - inf, so without that return the result is NaN."""
    xp = np.array([0.0, 0.2, 0.8, 1.0])
    for fp, want in (([10.0, 15.0, np.inf, 25.0], 15.0), ([10.0, -np.inf, np.inf, 25.0], -np.inf)):
        fp = np.array(fp)
        with np.errstate(invalid="ignore"):
            assert np.interp(0.2, xp, fp) == want
        out, _, st = table_ppf(INTERP, np.array([0.2]), xp, fp)
        print(f"np.interp(0.2, {xp.tolist()}, {fp.tolist()}): numpy {want}, device {out.host()[0]}")
        assert st == 0 and out.host()[0] == want and out.intact()


# ---------------------------------------------------------------------------- SEARCH
def search_reference(t0, values, q):
    m = len(t0)
    idx = np.searchsorted(t0, q, side="right")
    oob = idx >= m
    idx = np.minimum(idx, m - 1)
    return (idx.astype(np.int64) if values is None else values[idx]), bool(oob.any())


def cumulative(m, repeats):
    rng = np.random.default_rng(m)
    p = rng.uniform(0.1, 1.0, m)
    if repeats and m > 2:
        p[rng.choice(m, size=max(1, m // 3), replace=False)] = 0.0  # zero-probability entries
        p[-1] = 0.3
    return np.cumsum(p / p.sum())


SEARCH_VALUES = ["index", "index_f64", "int64", "float64", "float64_nonfinite"]


def search_values(kind, m):
    rng = np.random.default_rng(7 + m)
    if kind in ("index", "index_f64"):
        return None
    if kind == "int64":
        v = rng.integers(-10 ** 6, 10 ** 6, size=m)
        v[0], v[-1] = -(2 ** 63 - 1), 2 ** 63 - 1
        if m > 2:
            v[1] = 2 ** 63 - 1
        return v.astype(np.int64)
    v = rng.normal(size=m) * 100.0
    if kind == "float64_nonfinite":
        v[0] = np.nan
        v[-1] = np.inf
        if m > 2:
            v[m // 2] = -np.inf
    return v


@pytest.mark.parametrize("values", SEARCH_VALUES)
@pytest.mark.parametrize("m", [1, 2, 8, 1001])
def test_search_cumulative_values(gpu, m, values):
    """Distinct and repeated cumulative values, q inside the table and past its last value,
    q_stride 1 and 3."""
    for repeats in (False, True):
        for in_range in (True, False):
            for qs in (1, 3):
                search_case(m, repeats, values, in_range, qs)


def search_case(m, repeats, values, in_range, qs):
    t0 = cumulative(m, repeats)
    q = np.concatenate([ulps(t0), 0.5 * (t0[:-1] + t0[1:]), [0.0, 0.5 * t0[0]]])
    q = np.maximum(q, 0.0)  # (the last cumulative value may round to just above 1: no upper clip)
    if in_range:
        q = q[q < t0[-1]]
    v = search_values(values, m)
    ref, oob = search_reference(t0, v, q)
    assert oob == (not in_range)
    as_int = values in ("index", "int64")
    out, flag, st = table_ppf(SEARCH, q, t0, v, out_dtype=INT64 if as_int else FLOAT64, qo=1, qs=qs, oo=1)
    assert st == 0
    got = out.host(np.int64 if as_int else np.float64)
    same_bits(got, ref if as_int else np.asarray(ref, dtype=np.float64),
              f"search m={m} {values} repeats={repeats} inside={in_range} qs={qs}")
    assert out.intact()
    nonfinite = (not as_int) and not np.isfinite(np.asarray(ref, dtype=np.float64)).all()
    assert flag == (4 if oob else 0) | (1 if nonfinite else 0)


@pytest.mark.parametrize("values", ["index", "float64", "float64_nonfinite"])
def test_search_flag_one_lane(gpu, values):
    """Bit 2 from a single q >= t0[m - 1], wherever it sits: first lane, last lane of a wave, first
    lane of the next, and the only active lane of the last, partly filled wave (n = 65, 257).  With
    non-finite values the clamped row reads values[m - 1] = inf, so bits 0 and 2 are set together."""
    for n in (65, 257):
        for pos in (0, 63, 64, n - 1):
            flag_one_lane_case(n, pos, values)


def flag_one_lane_case(n, pos, values):
    m = 8
    t0 = cumulative(m, False)
    v = search_values(values, m)
    rng = np.random.default_rng(n + pos)
    lo = t0[0] if values == "float64_nonfinite" else 0.0  # values[0] is the NaN: keep the rest finite
    q = rng.uniform(lo, np.nextafter(t0[-2], 0.0), n)
    if values == "float64_nonfinite":
        q[(q >= t0[m // 2 - 1]) & (q < t0[m // 2])] = t0[0]  # and away from the -inf entry
    as_int = values == "index"
    for hit in (False, True):
        if hit:
            q[pos] = t0[-1]
        ref, oob = search_reference(t0, v, q)
        assert oob == hit
        out, flag, st = table_ppf(SEARCH, q, t0, v, out_dtype=INT64 if as_int else FLOAT64)
        assert st == 0
        same_bits(out.host(np.int64 if as_int else np.float64), ref)
        assert out.intact()
        want = 4 if hit else 0
        if hit and values == "float64_nonfinite":
            want |= 1
        assert flag == want, (n, pos, flag, want)


# ---------------------------------------------------------------------------- geometry
def geometry_case(kind):
    if kind == QUANTILE:
        a = quantile_data("gamma", 1001)
        return a, None, 0, lambda q: np.quantile(a, q, method="linear")
    if kind == INTERP:
        xp, fp = interp_xp(50), interp_fp("dec", 50)
        return xp, fp, 0, lambda q: np.interp(q, xp, fp)
    t0, v = cumulative(8, True), search_values("float64", 8)
    return t0, v, 0, lambda q: search_reference(t0, v, q)[0]


def pattern():
    rng = np.random.default_rng(4099)
    return rng.uniform(0.0, 0.99, PERIOD)


@pytest.mark.parametrize("n", N_GEOMETRY)
@pytest.mark.parametrize("kind", [INTERP, QUANTILE, SEARCH], ids=["interp", "quantile", "search"])
def test_table_geometry(gpu, kind, n):
    """Every offset of q and out, q_stride 1 and 3, with a flag word and with a NULL flag."""
    t0, t1, method, ref = geometry_case(kind)
    q = np.resize(pattern(), n)
    want = ref(q)
    for qs in (1, 3):
        for qo, oo in ((0, 0), (1, 0), (0, 1), (1, 1)):
            what = f"n={n} qs={qs} qo={qo} oo={oo}"
            out, flag, st = table_ppf(kind, q, t0, t1, method, qo=qo, qs=qs, oo=oo)
            assert st == 0, what
            same_bits(out.host(), want, what)
            assert out.intact() and flag == 0, what
            out, flag, st = table_ppf(kind, q, t0, t1, method, qo=qo, qs=qs, oo=oo, with_flag=False)
            assert st == 0 and out.intact(), what
            same_bits(out.host(), want, what)


@pytest.mark.parametrize("qo,qs,oo", [(0, 1, 0), (1, 3, 1)])
@pytest.mark.parametrize("kind", [INTERP, QUANTILE, SEARCH], ids=["interp", "quantile", "search"])
def test_table_second_grid_trip(gpu, kind, qo, qs, oo):
    t0, t1, method, ref = geometry_case(kind)
    pat = pattern()
    out, flag, st = table_ppf(kind, tile_to(pat, N_LARGE), t0, t1, method, qo=qo, qs=qs, oo=oo, n=N_LARGE)
    assert st == 0
    assert tiles_equal_first(out.dev(), PERIOD)
    same_bits(out.dev()[:PERIOD].cpu().numpy().view(np.float64), ref(pat))
    assert out.intact() and flag == 0


# ---------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("case", ["m0", "interp_without_fp", "method5", "quantile_int64"])
def test_table_argument_errors(gpu, case):
    from probabilit_amd import _lib

    q = np.linspace(0.0, 0.9, 257)
    t0, t1 = np.linspace(0.1, 1.0, 8), np.arange(8.0)
    kw = {"m0": dict(kind=SEARCH, m=0), "interp_without_fp": dict(kind=INTERP, t1=None),
          "method5": dict(kind=QUANTILE, method=5), "quantile_int64": dict(kind=QUANTILE, out_dtype=INT64)}[case]
    args = dict(kind=SEARCH, t1=t1, method=0, out_dtype=FLOAT64, m=None)
    args.update(kw)
    out, flag, st = table_ppf(args["kind"], q, t0, args["t1"], args["method"], args["out_dtype"], m=args["m"])
    assert st != 0 and _lib.last_error()
    assert out.untouched() and flag == 0
