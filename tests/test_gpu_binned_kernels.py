"""pbh_binned_sums alone, through probabilit_amd.native, on crafted columns: the counts against
np.histogram count for count, the sums against math.fsum per bin within the bound stated beside the
declaration (tests/binned_reference.py evaluates it).  The launch boundaries of the row tiles (one
row, the wave, the block tile T, the grid's span G, a ragged million), columns that are separate
allocations one double off 16-byte alignment with poison around them, values on and next to every
edge, repeated edges, the bin counts up to the cap, concentrated bins, special values, the centre,
128 pairs over 129 columns in one launch, and every refusal."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from binned_reference import finish_bounds, raw_sums, reference_allowance, sum_bounds  # noqa: E402

from probabilit_amd import _lib, device, inspection, native  # noqa: E402

T, G = native.SUMMARY_TILE, native.SUMMARY_SPAN
NS = [1, 2, 63, 64, 65, T - 1, T, T + 1, G + 1, 1_000_003]


def _columns(n, k=2, seed=0, rho=0.7):
    z = np.random.default_rng(seed).standard_normal((k, n))
    for c in range(1, k):
        z[c] = rho * z[0] + np.sqrt(1.0 - rho * rho) * z[c]
    return z


BASE = _columns(G + 1)  # the two correlated normal columns every size takes its rows from


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


def _counts(x, edges):
    x = np.asarray(x, dtype=np.float64)
    return np.histogram(x[~np.isnan(x)], edges)[0]


def _within(got, want, bound, what):
    """|got - want| <= bound where want is finite; the same NaN or infinity elsewhere."""
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), what
    err = np.abs(got[fin] - want[fin])
    assert (err <= bound[fin]).all(), (what, err.max(), bound[fin][err.argmax()])


def _compare(got, x, y, edges, centre, what=""):
    count, s1, s2 = got
    m = len(edges) - 1
    assert count.dtype == np.int64 and s1.dtype == s2.dtype == np.float64
    assert count.shape == s1.shape == s2.shape == (m,)
    assert np.array_equal(count, _counts(x, edges)), what
    want_count, want1, want2, a1 = raw_sums(x, y, edges, centre)
    assert np.array_equal(count, want_count), what
    b1, b2 = sum_bounds(count, want2, a1)
    _within(s1, want1, b1, (what, "s1"))
    _within(s2, want2, b2, (what, "s2"))
    empty = count == 0
    assert (s1[empty] == 0.0).all() and (s2[empty] == 0.0).all()
    return b1, b2


def _check(gpu, cols, edges, pairs=((0, 1),), centres=None):
    """native.binned_sums of host columns placed off alignment, every pair compared."""
    cols = [np.asarray(c, dtype=np.float64) for c in cols]
    edges = [None if e is None else np.asarray(e, dtype=np.float64) for e in edges]
    centres = [0.0] * len(cols) if centres is None else centres
    got = native.binned_sums([_place(gpu, c) for c in cols], edges, list(pairs), centres)
    assert len(got) == len(pairs)
    for p, ((i, j), res) in enumerate(zip(pairs, got)):
        _compare(res, cols[i], cols[j], edges[i], centres[j], (p, i, j))
    return got


XE = np.linspace(-1.0, 1.5, 8)  # 7 bins, rows outside on both sides


@pytest.mark.parametrize("n", NS)
def test_sizes(gpu, n):
    x, y = BASE[0, :n], BASE[1, :n]
    if n > 64:
        assert (x < XE[0]).any() and (x > XE[-1]).any()
    _check(gpu, [x, y], [XE, None], centres=[0.0, 0.25])


@pytest.mark.parametrize("n", [1, 65, T, T + 1])
def test_poison_around_the_columns_is_not_read(gpu, n):
    """A range that reaches 1e300: a row read one before or one past the columns (1e300 or NaN on
    both) would be counted in the last bin, or poison a sum."""
    e = np.array([-10.0, 0.0, 10.0, 1e300])
    count, s1, s2 = _check(gpu, [BASE[0, :n], BASE[1, :n]], [e, np.linspace(-10.0, 1e300, 4)], [(0, 1), (1, 0)])[0]
    assert count.sum() == n and count[2] == 0 and s1[2] == 0.0 and s2[2] == 0.0


# ---------------------------------------------------------------- special values
U9 = np.linspace(-1.1, 2.3, 10)  # 9 uniform bins whose edges are not exact multiples of a step
NONUNI = np.array([-1.1, -0.3, 0.0, 0.0, 0.4, 0.4, 0.4, 1.7, 2.3])  # repeated edges, a zero among them


def _special(edges):
    return np.concatenate([[np.nan, np.inf, -np.inf, -0.0, 0.0, edges[0], edges[-1]], edges,
                           np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])


@pytest.mark.parametrize("kind", ["uniform", "nonuniform_repeated"])
def test_x_on_every_edge_and_one_ulp_to_each_side(gpu, kind):
    n = T + 65
    edges = {"uniform": U9, "nonuniform_repeated": NONUNI}[kind]
    cols = _columns(n, seed=3)
    sp = _special(edges)
    at = np.random.default_rng(5).choice(n, len(sp), replace=False)
    cols[0, at] = sp
    _check(gpu, list(cols), [edges, None], centres=[0.0, -0.5])


def test_rows_on_repeated_edges(gpu):
    """Every row on a repeated edge value: numpy puts it after the last repeat."""
    n = T + 1
    x = np.random.default_rng(8).choice(NONUNI, n)
    count = _check(gpu, [x, BASE[1, :n]], [NONUNI, None])[0][0]
    assert count.sum() == n and count[2] == 0 and count[4] == 0 and count[5] == 0  # zero-width bins stay empty


def test_last_edge_repeated(gpu):
    e = np.array([-1.0, 0.0, 1.0, 1.0])
    x = np.array([1.0, 1.0, 0.5, -1.0, np.nextafter(1.0, 2.0), 0.0] * 20)
    _check(gpu, [x, x[::-1].copy()], [e, None])


def test_uniform_and_searched_edges_count_alike(gpu):
    """A bit-exact linspace takes the guess-and-correct path; one edge moved by one ulp (past no
    sample) takes the search, and so does the exact table with the uniform promise withdrawn."""
    n = 3 * T + 7
    x, y = BASE[0, :n], BASE[1, :n]
    lin = np.linspace(-2.5, 2.75, 38)
    nudged = lin.copy()
    nudged[11] = np.nextafter(lin[11], np.inf)
    assert not ((x >= lin[11]) & (x < nudged[11])).any()
    a = _check(gpu, [x, y], [lin, None])[0]
    b = _check(gpu, [x, y], [nudged, None])[0]
    assert np.array_equal(a[0], b[0]) and 0 < a[0].sum() < n
    cols = [_place(gpu, x), _place(gpu, y)]
    for promise in (1, 0):  # (and a promise broken on a table that is not uniform costs time only)
        st, out = _raw(cols, [lin, None], [(0, 1)], uniform=[promise, 0])
        assert st == _lib.OK and np.array_equal(device.to_host(out[0])[:37], a[0])
    st, out = _raw(cols, [NONUNI, None], [(0, 1)], uniform=[1, 0])
    assert st == _lib.OK and np.array_equal(device.to_host(out[0])[:8], _counts(x, NONUNI))


# ---------------------------------------------------------------- bin shapes
@pytest.mark.parametrize("bins", [1, 2, 1024])
@pytest.mark.parametrize("uniform", [True, False])
def test_bin_counts(gpu, bins, uniform):
    n = 3 * T + 7
    e = np.linspace(-2.5, 2.75, bins + 1)
    if not uniform:
        e = np.concatenate([e[:1], np.sort(np.random.default_rng(bins).uniform(-2.5, 2.75, bins - 1)), e[-1:]])
    count = _check(gpu, [BASE[0, :n], BASE[1, :n]], [e, None], centres=[0.0, 0.1])[0][0]
    assert 0 < count.sum() < n


@pytest.mark.parametrize("n", [T + 1, G + 1])
@pytest.mark.parametrize("case", ["one_bin", "i_equals_j", "x_equals_y", "x_equals_minus_y", "alternating"])
def test_concentrated_bins(gpu, case, n):
    e = np.linspace(-3.0, 3.0, 17)
    spread = BASE[1, :n]
    if case == "one_bin":  # every wave's rows share the bin: one LDS add per wave
        count = _check(gpu, [np.full(n, 0.3), spread], [e, None], centres=[0.0, 0.5])[0][0]
        assert count[8] == n and count.sum() == n
    elif case == "i_equals_j":  # E[X | X in bin]
        count, s1, _ = _check(gpu, [spread], [e], [(0, 0)])[0]
        has = count > 0
        assert (s1[has] / count[has] >= e[:-1][has]).all() and (s1[has] / count[has] <= e[1:][has]).all()
    elif case == "x_equals_y":
        a, b = _check(gpu, [spread, spread.copy()], [e, e], [(0, 1), (1, 0)])
        assert np.array_equal(a[0], b[0])
    elif case == "x_equals_minus_y":
        (count, s1, s2), (_, t1, t2) = _check(gpu, [spread, -spread], [e, None], [(0, 1), (0, 0)])
        assert count.sum() > 0 and (np.sign(s1) == -np.sign(t1)).all()
    else:  # neighbouring rows in two bins: no wave shares one
        x = np.where(np.arange(n) % 2 == 0, -2.9, 2.9)
        count = _check(gpu, [x, spread], [e, None])[0][0]
        assert count[0] == (n + 1) // 2 and count[15] == n // 2 and count.sum() == n


# ---------------------------------------------------------------- values
def test_nan_x_rows_are_dropped(gpu):
    n = T + 65
    cols = _columns(n, seed=11)
    cols[0, ::7] = np.nan
    cols[1, ::7] = 1e6  # (would show in every sum)
    count = _check(gpu, list(cols), [U9, None])[0][0]
    assert count.sum() <= n - len(cols[0, ::7])


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_non_finite_y_poisons_its_bin_only(gpu, poison):
    n = 2 * T + 3
    cols = _columns(n, seed=12)
    row = int(np.flatnonzero((cols[0] >= U9[3]) & (cols[0] < U9[4]))[5])
    cols[1, row] = poison
    outside = int(np.flatnonzero(cols[0] > U9[-1])[0])
    cols[1, outside] = np.nan  # a NaN y on a row whose x is outside reaches nothing
    count, s1, s2 = _check(gpu, list(cols), [U9, None], centres=[0.0, 0.5])[0]
    clean = np.arange(9) != 3
    assert np.isfinite(s1[clean]).all() and np.isfinite(s2[clean]).all()
    if np.isnan(poison):
        assert np.isnan(s1[3]) and np.isnan(s2[3])
    else:
        assert s1[3] == poison and s2[3] == np.inf
    assert np.array_equal(count, _counts(cols[0], U9)) and count[3] > 1


def test_a_finite_outlier(gpu):
    """y = 1e300 in one row: its square overflows, so its bin's s2 is +inf; s1 holds it within the
    bound, and the other bins are untouched."""
    n = T + 1
    cols = _columns(n, seed=13)
    row = int(np.flatnonzero((cols[0] >= U9[5]) & (cols[0] < U9[6]))[0])
    cols[1, row] = 1e300
    count, s1, s2 = _check(gpu, list(cols), [U9, None])[0]
    assert s2[5] == np.inf and np.isfinite(s1[5]) and s1[5] > 9e299
    assert np.isfinite(np.delete(s2, 5)).all()


# ---------------------------------------------------------------- the centre
def test_centre(gpu):
    """y = 1e9 + N(0, 1).  About centre 0 the sums meet the header's bound (asserted), but that bound
    carried to std (binned_reference.finish_bounds) is wider than the std itself: s2 / m and
    (s1 / m)^2 are both 1e18 and their difference is lost.  About the column's mean the same bound
    is some 1e-12, and std agrees with scipy.stats.binned_statistic's two-pass std within it: the
    reason the kernel takes a centre."""
    import scipy.stats

    n = 3 * T + 7
    x = BASE[0, :n]
    y = 1e9 + BASE[1, :n]
    e = np.linspace(-2.5, 2.75, 12)
    mean = float(np.mean(y))
    cols = [_place(gpu, x), _place(gpu, y)]
    zero, centred = (native.binned_sums(cols, [e, None], [(0, 1)], [0.0, c])[0] for c in (0.0, mean))
    _compare(zero, x, y, e, 0.0, "centre 0")
    _compare(centred, x, y, e, mean, "centre = mean")
    want = scipy.stats.binned_statistic(x, y, "std", bins=e)[0]
    allowance = reference_allowance(x, y, e, "std")
    for (count, s1, s2), c, tight in ((zero, 0.0, False), (centred, mean, True)):
        _, _, ref2, a1 = raw_sums(x, y, e, c)
        bound = finish_bounds(count, s1, ref2, a1, c)["std"]
        got = inspection.binned_finish(count, s1, s2, c, "std")
        print("centre", c, "std error", np.abs(got - want).max(), "bound", bound.max())
        if tight:
            assert (bound < 1e-10).all() and (np.abs(got - want) <= bound + allowance).all()
        else:
            assert (bound > want).all()


# ---------------------------------------------------------------- launch shapes
def test_128_pairs_over_129_columns(gpu):
    """Every input binned against the one value column, which has no bins and no edges; the bin
    counts differ from column to column, so every pair's output offset is its own."""
    n, k = T + 1, 129
    cols = _columns(n, k, seed=21) + 0.01 * np.arange(k)[:, None]
    bins = [None] + [(3, 4, 5, 8, 1, 33)[c % 6] for c in range(1, k)]
    edges = [None] + [np.linspace(-1.5 + 0.01 * c, 1.75, b + 1) if c % 3 else
                      np.concatenate([[-2.0], np.arange(b - 1) * 0.3, [2.0]]) for c, b in list(enumerate(bins))[1:]]
    pairs = [(c, 0) for c in range(1, k)]
    assert len(pairs) == native.BINNED_MAX_PAIRS and k == native.BINNED_MAX_COLUMNS
    _check(gpu, list(cols), edges, pairs, centres=[0.3] + [0.0] * (k - 1))


def test_pairs_in_any_order_and_value_columns_of_their_own_centre(gpu):
    n = T + 1
    cols = _columns(n, 4, seed=22)
    edges = [XE, None, NONUNI, U9]
    pairs = [(0, 1), (2, 1), (3, 0), (0, 1), (2, 2), (3, 1), (0, 3)]
    got = _check(gpu, list(cols), edges, pairs, centres=[0.5, -0.25, 0.0, 1.0])
    assert all(np.array_equal(a, b) for a, b in zip(got[0][:1], got[3][:1]))


def test_same_call_twice(gpu):
    """The counts are equal; the sums come from atomics, so each run is within the bound of the
    exact sum and two runs within twice the bound of each other.  Bit equality is not promised."""
    n = G + 1
    x, y = BASE[0, :n], BASE[1, :n]
    cols = [_place(gpu, x), _place(gpu, y)]
    e = [np.linspace(-2.0, 2.0, 65), NONUNI]
    a = native.binned_sums(cols, e, [(0, 1), (1, 0)], [0.1, -0.1])
    b = native.binned_sums(cols, e, [(0, 1), (1, 0)], [0.1, -0.1])
    for p, (i, j, c) in enumerate(((0, 1, -0.1), (1, 0, 0.1))):
        b1, b2 = _compare(a[p], (x, y)[i], (x, y)[j], e[i], c)
        assert np.array_equal(a[p][0], b[p][0]) and a[p][0].sum() > 0
        assert (np.abs(a[p][1] - b[p][1]) <= 2 * b1).all() and (np.abs(a[p][2] - b[p][2]) <= 2 * b2).all()


# ---------------------------------------------------------------- refusals
def _raw(cols, edges, pairs, centres=None, uniform=None, ws_bytes=None, n=None, k=None, ptrs=None, out=None,
         bins=None):
    """pbh_binned_sums through ctypes with every table as given: (status, (counts, s1, s2) device)."""
    lib = _lib.load()
    edges = [np.zeros(0) if e is None else np.ascontiguousarray(e, dtype=np.float64) for e in edges]
    k = len(cols) if k is None else k
    n = cols[0].shape[0] if n is None else n
    bins = np.array([max(len(e) - 1, 0) for e in edges] if bins is None else bins, dtype=np.int32)
    flat = np.concatenate(edges + [np.zeros(1)])
    uni = np.array([0] * len(edges) if uniform is None else uniform, dtype=np.uint8)
    ctr = np.array([0.0] * max(k, 1) if centres is None else centres, dtype=np.float64)
    ptrs = np.array([x.data_ptr() for x in cols] if ptrs is None else ptrs, dtype=np.uint64)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    if ws_bytes is None:
        b = ctypes.c_size_t()
        ok_bins = np.clip(bins[:native.BINNED_MAX_COLUMNS], 0, native.BINNED_MAX_BINS)
        _lib.check(lib.pbh_binned_sums_workspace_size(max(len(ok_bins), 1), _lib.np_ptr(ok_bins), ctypes.byref(b)))
        ws_bytes = b.value
    ws = device.empty(max(int(ws_bytes), 8), "uint8")
    if out is None:
        total = 4096
        out = (device.zeros(total, "int64"), device.zeros(total), device.zeros(total))
    st = lib.pbh_binned_sums(_lib.np_ptr(ptrs), k, n, _lib.np_ptr(flat), _lib.np_ptr(bins), _lib.np_ptr(uni),
                             _lib.np_ptr(ctr), _lib.np_ptr(pr), len(pr), out[0].data_ptr(), out[1].data_ptr(),
                             out[2].data_ptr(), ws.data_ptr(), int(ws_bytes), device.stream())
    device.synchronize()
    return st, out


def _e(bins):
    return np.linspace(-2.0, 2.0, bins + 1)


INVALID, WORKSPACE = _lib.ERR_INVALID, _lib.ERR_WORKSPACE
REFUSALS = {
    "k_130": (dict(k=130), INVALID, "columns"),
    "k_0": (dict(k=0), INVALID, "columns"),
    "npairs_129": (dict(pairs=[(0, 1)] * 129), INVALID, "npairs"),
    "npairs_0": (dict(pairs=[]), INVALID, "npairs"),
    "bins_1025": (dict(edges=[_e(1025), None]), INVALID, "1024"),
    "negative_bins": (dict(bins=[-1, 0]), INVALID, "bins"),
    "index_out_of_range": (dict(pairs=[(0, 2)]), INVALID, "outside"),
    "negative_index": (dict(pairs=[(0, 1), (-1, 0)]), INVALID, "outside"),
    "binning_column_without_bins": (dict(pairs=[(1, 0)]), INVALID, "no bins"),
    "decreasing_edges": (dict(edges=[np.array([0.0, 2.0, 1.0, 3.0]), None]), INVALID, "edges"),
    "non_finite_edge": (dict(edges=[np.array([0.0, 1.0, np.inf]), None]), INVALID, "finite"),
    "nan_edge": (dict(edges=[np.array([0.0, np.nan, 1.0]), None]), INVALID, "finite"),
    "first_edge_equals_last": (dict(edges=[np.array([1.0, 1.0, 1.0]), None]), INVALID, "increasing"),
    "nan_centre": (dict(centres=[0.0, np.nan]), INVALID, "centre"),
    "inf_centre": (dict(centres=[np.inf, 0.0]), INVALID, "centre"),
    "n_0": (dict(n=0), INVALID, "at least one sample"),
    "n_2_to_the_32": (dict(n=1 << 32), INVALID, "32-bit"),
    "null_column": (dict(null=1), INVALID, "NULL or not 8-byte aligned"),
    "misaligned_column": (dict(shift=4), INVALID, "NULL or not 8-byte aligned"),
    "workspace_too_small": (dict(ws_bytes=64), WORKSPACE, "workspace"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_launch_nothing(gpu, case):
    """Host-side argument checks, by status and message: the sentinel-filled outputs stay as they
    were, and a valid call right after gives the right sums."""
    n = 1000
    kw, status, text = REFUSALS[case]
    kw = dict(kw)
    k = kw.pop("k", 2)
    cols = [_place(gpu, BASE[c % 2, :n]) for c in range(max(k, 2))][:max(k, 1)]
    ptrs = [x.data_ptr() for x in cols]
    if "null" in kw:
        ptrs[kw.pop("null")] = 0
    if "shift" in kw:
        ptrs[0] += kw.pop("shift")
    edges = kw.pop("edges", [_e(4)] + [None] * (len(cols) - 1))
    pairs = kw.pop("pairs", [(0, 1)])
    out = (device.to_device(np.full(4096, -7, dtype=np.int64)), device.to_device(np.full(4096, 123.0)),
           device.to_device(np.full(4096, -321.0)))
    st, _ = _raw(cols, edges, pairs, k=k, ptrs=ptrs, out=out, **kw)
    assert st == status and text in _lib.last_error(), _lib.last_error()
    assert _lib.last_error().startswith("pbh_binned_sums:")
    assert (device.to_host(out[0]) == -7).all() and (device.to_host(out[1]) == 123.0).all()
    assert (device.to_host(out[2]) == -321.0).all()
    _check(gpu, [BASE[0, :n], BASE[1, :n]], [XE, None])


def test_refusals_raise_through_native(gpu):
    n = 1000
    cols = [_place(gpu, BASE[c, :n]) for c in range(2)]
    with pytest.raises(MemoryError, match="workspace"):
        native.binned_sums(cols, [_e(4), None], [(0, 1)], [0.0, 0.0], ws_bytes=64)
    with pytest.raises(ValueError, match="no bins"):
        native.binned_sums(cols, [_e(4), None], [(1, 0)], [0.0, 0.0])
    with pytest.raises(ValueError, match="centre 1 is not finite"):
        native.binned_sums(cols, [_e(4), None], [(0, 1)], [0.0, np.nan])
    with pytest.raises(ValueError, match="one centre per column"):
        native.binned_sums(cols, [_e(4), None], [(0, 1)], [0.0])
    with pytest.raises(ValueError, match="at least two edges"):
        native.binned_sums(cols, [np.array([1.0]), None], [(0, 1)], [0.0, 0.0])
    with pytest.raises(TypeError, match="float64 device vectors"):
        native.binned_sums([cols[0], cols[1].float()], [_e(4), None], [(0, 1)], [0.0, 0.0])
    with pytest.raises(ValueError, match="contiguous"):
        native.binned_sums([cols[0][::2], cols[1][::2]], [_e(4), None], [(0, 1)], [0.0, 0.0])
    _check(gpu, [BASE[0, :n], BASE[1, :n]], [XE, None])
