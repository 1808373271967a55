"""pbh_moments, pbh_select_ranks and pbh_histogram alone, through probabilit_amd.native, at their
launch boundaries: one sample, the wave, the block tile T, the grid's span G, a ragged million;
padded columns whose padding is poison, a column start one double off 16-byte alignment, 1 / 3 /
128 columns."""

import numpy as np
import pytest

from summary_reference import check_moments, header_terms

pytestmark = pytest.mark.gpu

from probabilit_amd import native  # noqa: E402

T, G = native.SUMMARY_TILE, native.SUMMARY_SPAN
ST, SG = native.SELECT_TILE, native.SELECT_SPAN
NS = [1, 2, 63, 64, 65, T - 1, T, T + 1, G + 1, 1_000_003]
SELECT_NS = [1, 2, 63, 64, 65, ST - 1, ST, ST + 1, SG + 1, 1_000_003]


def _normals(n, k=1, seed=0):
    return np.random.default_rng(seed).standard_normal((k, n))


def _place(gpu, cols, pad=0, poison=np.nan, offset=0):
    """The (k, n) host block `cols` on the device as a view with column stride n + pad, the padding
    (and everything around the block) filled with `poison`, starting `offset` doubles into a
    16-byte aligned buffer."""
    import torch

    k, n = cols.shape
    ld = n + pad
    host = np.full(offset + k * ld + 2, poison)
    host[offset:offset + k * ld].reshape(k, ld)[:, :n] = cols
    buf = torch.from_numpy(host).to(gpu)
    view = buf[offset:offset + k * ld].view(k, ld)[:, :n]
    assert view.data_ptr() % 16 == 8 * (offset % 2)
    return view


LAYOUTS = {"plain": dict(), "nan_padding_off_by_one": dict(pad=3, poison=np.nan, offset=1),
           "huge_padding": dict(pad=5, poison=1e300)}


def _rows(mom):
    return [dict(zip(native.MOMENT_FIELDS, r)) for r in mom]


# ---------------------------------------------------------------- moments
def test_documented_summation_shape():
    for n in NS + [10 ** 8]:
        assert native.moments_terms(n) == header_terms(n)


@pytest.mark.parametrize("n", NS)
def test_moments_sizes(gpu, n):
    x = _normals(n, 1, seed=n)
    got = _rows(native.moments(_place(gpu, x, **LAYOUTS["nan_padding_off_by_one"])))[0]
    assert got["nan"] == 0 and got["min"] == x.min() and got["max"] == x.max()
    check_moments(x[0], got, "normals")


@pytest.mark.parametrize("layout", ["plain", "huge_padding"])
@pytest.mark.parametrize("n", [65, T + 1])
@pytest.mark.parametrize("k", [3, 128])
def test_moments_blocks_of_columns(gpu, k, n, layout):
    x = _normals(n, k, seed=k + n) * np.arange(1, k + 1)[:, None] + np.arange(k)[:, None]
    rows = _rows(native.moments(_place(gpu, x, **LAYOUTS[layout])))
    assert len(rows) == k
    for c in (range(k) if k == 3 else (0, 1, 63, 64, 127)):
        assert rows[c]["nan"] == 0 and rows[c]["min"] == x[c].min() and rows[c]["max"] == x[c].max()
        check_moments(x[c], rows[c], f"column {c}")
    assert all(np.isfinite(list(r.values())).all() for r in rows)  # no poison leaked anywhere


@pytest.mark.parametrize("n", [65, T + 1, 3 * T + 7])
def test_moments_cancellation(gpu, n):
    """1e8 + N(0, 1): a one-pass sum of squares loses every digit of the variance here."""
    x = 1e8 + _normals(n, 1, seed=3)
    got = _rows(native.moments(_place(gpu, x)))[0]
    check_moments(x[0], got, "1e8 + normals")
    assert abs(got["m2"] - np.var(x[0])) <= 1e-6 * np.var(x[0])


@pytest.mark.parametrize("value", [0.1, -3.3e-7, 1e300, 0.0])
@pytest.mark.parametrize("n", [3, 65, T + 1, 3 * T + 7])
def test_moments_all_equal(gpu, n, value):
    got = _rows(native.moments(_place(gpu, np.full((1, n), value))))[0]
    assert got["mean"] == value and got["min"] == value and got["max"] == value
    assert got["m2"] == 0.0 and got["m3"] == 0.0 and got["m4"] == 0.0 and got["nan"] == 0


@pytest.mark.parametrize("n", [65, T + 1])
def test_moments_nan_and_inf(gpu, n):
    x = _normals(n, 4, seed=9)
    x[0, n // 2] = np.nan
    x[1, 0] = np.inf
    x[2, n - 1] = -np.inf
    x[3, 1], x[3, n - 2] = np.inf, -np.inf
    rows = _rows(native.moments(_place(gpu, x, **LAYOUTS["huge_padding"])))
    assert rows[0]["nan"] == 1 and all(np.isnan(rows[0][f]) for f in ("min", "max", "mean", "m2", "m3", "m4"))
    with np.errstate(invalid="ignore"):
        for c in (1, 2, 3):
            assert rows[c]["nan"] == 0
            assert rows[c]["min"] == x[c].min() and rows[c]["max"] == x[c].max()
            np.testing.assert_array_equal(rows[c]["mean"], np.mean(x[c]))  # +inf, -inf, nan: as numpy
            assert np.isnan(rows[c]["m2"]) and np.isnan(np.var(x[c]))


def test_moments_denormals(gpu):
    """Sums of denormals are exact (every partial sum is a multiple of 2^-1074 below 2^-1021); their
    squares underflow to zero, as they do in np.var."""
    n = T + 1
    ints = np.random.default_rng(4).integers(-2 ** 20, 2 ** 20, n)
    x = (ints * 2.0 ** -1074)[None, :]
    got = _rows(native.moments(_place(gpu, x)))[0]
    total = int(ints.sum()) * 2.0 ** -1074  # exact
    assert got["mean"] == total / n
    assert got["min"] == x.min() and got["max"] == x.max()
    assert got["m2"] == 0.0 and got["m3"] == 0.0 and got["m4"] == 0.0 and np.var(x) == 0.0


@pytest.mark.parametrize("n", [T + 1, G + 1])
def test_moments_reproducible(gpu, n):
    xd = _place(gpu, _normals(n, 1, seed=6))
    a, b = native.moments(xd), native.moments(xd)
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- select
def _check_select(gpu, x, ranks, **layout):
    got = native.select_ranks(_place(gpu, x[None, :], **layout)[0], ranks)
    want = np.sort(x)[np.asarray(ranks)]
    np.testing.assert_array_equal(got, want)  # NaN == NaN, -0.0 == 0.0


@pytest.mark.parametrize("n", SELECT_NS)
def test_select_sizes(gpu, n):
    x = _normals(n, 1, seed=n)[0]
    _check_select(gpu, x, sorted({0, n - 1, n // 2}), **LAYOUTS["nan_padding_off_by_one"])


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def _select_inputs(n):
    rng = np.random.default_rng(12)
    out = {"normals": rng.standard_normal(n), "all_equal": np.full(n, 2.5)}
    out["top_48_bits_equal"] = _from_bits((np.uint64(0x3FF0123456780000) | rng.integers(0, 2 ** 16, n).astype(np.uint64)))
    top = rng.integers(0x0010, 0x7FF0, n).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(15))
    out["only_top_16_bits_differ"] = _from_bits(top << np.uint64(48))
    mixed = rng.standard_normal(n) * 10.0 ** rng.integers(-300, 300, n)
    mixed[:12] = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308, -1e-310, 0.0, -0.0, np.inf, -np.inf]
    out["mixed_signs_zeros_inf_denormals"] = rng.permutation(mixed)
    nans = rng.standard_normal(n)
    nans[rng.choice(n, 5, replace=False)] = [np.nan, -np.nan, np.nan, _from_bits([0x7FF0000000000001])[0], np.nan]
    out["five_nans"] = nans
    rep = rng.standard_normal(n)
    rep[rng.choice(n, n // 3, replace=False)] = np.median(rep)
    out["value_repeated_across_the_rank"] = rep
    out["few_distinct_values"] = rng.poisson(3.0, n).astype(np.float64)
    return out


N_SELECT = 65_537
SELECT_INPUTS = _select_inputs(N_SELECT)


@pytest.mark.parametrize("name", list(SELECT_INPUTS))
def test_select_inputs(gpu, name):
    x, n = SELECT_INPUTS[name], N_SELECT
    rng = np.random.default_rng(1)
    ranks = [0, n - 1, n // 2, n // 2 - 1, n // 2 + 1] + rng.integers(0, n, 40).tolist()
    if name == "five_nans":
        ranks += [n - 7, n - 6, n - 5, n - 4, n - 1]  # both sides of the first NaN (rank n - 5)
    _check_select(gpu, x, ranks, **LAYOUTS["huge_padding"])


@pytest.mark.parametrize("name", ["normals", "value_repeated_across_the_rank", "top_48_bits_equal"])
def test_select_rank_lists(gpu, name):
    x, n = SELECT_INPUTS[name], N_SELECT
    _check_select(gpu, x, [0, n - 1, n // 2])
    _check_select(gpu, x, [n // 2] * 64)  # 64 ranks all equal
    _check_select(gpu, x, (n - 1 - 1000 * np.arange(64)).tolist())  # 64 distinct, descending
    _check_select(gpu, x, [7])


def test_select_rejects_bad_ranks(gpu):
    xd = _place(gpu, _normals(100))[0]
    with pytest.raises(ValueError):
        native.select_ranks(xd, [100])
    with pytest.raises(ValueError):
        native.select_ranks(xd, [-1])
    with pytest.raises(ValueError):
        native.select_ranks(xd, list(range(65)))


# ---------------------------------------------------------------- histogram
def _check_histogram(gpu, x, bins, rng, **layout):
    x = np.atleast_2d(x)
    counts, edges = native.histogram(_place(gpu, x, **layout), bins, rng)
    assert counts.dtype == np.int64 and counts.shape == (x.shape[0], bins)
    for c in range(x.shape[0]):
        want, want_edges = np.histogram(x[c], bins=bins, range=rng)
        np.testing.assert_array_equal(edges, want_edges)
        np.testing.assert_array_equal(counts[c], want)


@pytest.mark.parametrize("n", NS)
def test_histogram_sizes(gpu, n):
    _check_histogram(gpu, _normals(n, 1, seed=n), 7, (-1.0, 1.5), **LAYOUTS["nan_padding_off_by_one"])


@pytest.mark.parametrize("layout", ["plain", "huge_padding"])
@pytest.mark.parametrize("k", [3, 128])
def test_histogram_blocks_of_columns(gpu, k, layout):
    x = _normals(T + 1, k, seed=k) + 0.01 * np.arange(k)[:, None]
    _check_histogram(gpu, x, 1000, (-2.0, 1e300 if layout == "huge_padding" else 2.0), **LAYOUTS[layout])


RANGES = [(0.1, 0.7), (-1.0, 1.0), (1e8, 1e8 + 1.0), (-3e-7, 5e15)]


@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("bins", [1, 2, 7, 1000, 4096])
def test_histogram_on_every_edge(gpu, bins, rng):
    edges = np.linspace(rng[0], rng[1], bins + 1)
    x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])
    _check_histogram(gpu, np.random.default_rng(0).permutation(x), bins, rng)


@pytest.mark.parametrize("bins", [1, 2, 7, 1000, 4096])
def test_histogram_inputs(gpu, bins):
    rng_ = np.random.default_rng(bins)
    n = T + 65
    lo, hi = 0.1, 0.7
    edges = np.linspace(lo, hi, bins + 1)
    b = bins // 2
    one_bin = rng_.uniform(edges[b], np.nextafter(edges[b + 1], -np.inf), n)
    _check_histogram(gpu, one_bin, bins, (lo, hi))  # the whole wave on one counter
    outside = rng_.uniform(-1.0, 2.0, n)
    outside[:4] = [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)]
    _check_histogram(gpu, outside, bins, (lo, hi))
    nans = rng_.uniform(lo, hi, n)
    nans[::7] = np.nan
    nans[3], nans[5] = np.inf, -np.inf
    _check_histogram(gpu, nans, bins, (lo, hi))


def test_histogram_rejects_bad_arguments(gpu):
    xd = _place(gpu, _normals(100))
    with pytest.raises(ValueError):
        native.histogram(xd, 4097, (0.0, 1.0))
    with pytest.raises(ValueError):
        native.histogram(xd, 10, (1.0, 1.0))
    with pytest.raises(ValueError):
        native.histogram(xd, 10, (0.0, np.inf))
