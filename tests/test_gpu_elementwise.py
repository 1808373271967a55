"""pbh_elementwise, its 16-byte + - * / fast path, pbh_average and pbh_transpose, each called
alone and compared with numpy.

    A  k_elementwise through modeling._binary / modeling._unary: 19 binary and 22 unary operators
       (and the cast) over float64, int64 and bool, vectors and _Broadcast scalars, on the cross
       product of edge lists plus random values.  The reference is modeling._NP_BINARY /
       _NP_UNARY on the same host arrays.
    B  k_arith_f64: operands and output carved out of padded buffers at byte offset 0 (fast
       path) and 8 (generic kernel), n around the quad loop's tail.
    C  pbh_average through ctypes against np.average(np.vstack(parents), axis=0).
    D  pbh_transpose through ctypes with padded leading dimensions.

Every output lives inside a wider buffer filled with a sentinel (modeling._alloc is replaced
for the call) and the whole buffer is compared, so a write outside [0, n) fails.

Exact operators are compared bit for bit (NaN positions and the signs of zero included; a NaN's
payload is not a value numpy defines).  max / min on float64: equal values and NaN positions; on
a tie of +0 and -0 the device returns its first operand where numpy 2.2 returns the second, so
the sign is not asserted there and the number of such elements goes to records/
(elementwise_minmax_zero_ties).

Rounded operators (pow, arctan2 and the transcendental unary ones): identical to numpy where
numpy's float64 result is non-finite or zero; elsewhere the error against the same numpy function
on np.longdouble (64-bit mantissa) in ulps of the float64 result must stay within
8 x max(numpy float64's own worst error on the same inputs, 0.5 ulp), and every finite result
within 1e-10 relative of that reference.  For these operators "numpy's float64 result" is the
function on the operands converted to float64, as numpy does for int64; for bool operands numpy
itself computes in float16 and the device, whose output dtype is _canonical(float16) = float64,
is held to the float64 function.  Yardstick and device maxima per operator go to records/
(elementwise_ulp).
"""

import ctypes
import functools
import itertools

import numpy as np
import pytest

from conftest import assert_close, record

pytestmark = pytest.mark.gpu

LD = np.longdouble
F64, I64, B8 = np.dtype(np.float64), np.dtype(np.int64), np.dtype(bool)
DTYPES = [F64, I64, B8]
PAD = 64  # sentinel elements on either side of an output
SENT = {F64: -777.25, I64: -777, B8: 0xA5}
FMAX = np.finfo(np.float64).max
IMAX, IMIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min

F_EDGE = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.0, -7.0, np.pi,
                   5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, 1e300, -1e300,
                   FMAX, -FMAX, np.inf, -np.inf, np.nan, 2.0**53, 2.0**53 + 2, 2.0**63, -2.0**63,
                   1e-8, 1 + 1e-8, 1 + 1e-5, 1 + 1.1e-5])
I_EDGE = np.array([0, 1, -1, 2, -2, 3, 7, -7, 63, 64, 2**31, 2**53 + 1, IMAX, IMIN, IMIN + 1], dtype=np.int64)
B_EDGE = np.array([False, True])
EDGE = {F64: F_EDGE, I64: I_EDGE, B8: B_EDGE}
SCALARS = {F64: [0.0, -2.5, 3.0, 1 + 1e-5, np.inf, np.nan], I64: [0, -1, 3, 2**53 + 1, IMIN], B8: [False, True]}
NRANDOM = 3000

EXACT_BINARY = {"add", "sub", "mul", "truediv", "floordiv", "mod", "and", "or", "eq", "ne", "lt", "le", "gt", "ge",
                "isclose"}
EXACT_UNARY = {"neg", "abs", "floor", "ceil", "sign", "sqrt", "square"}

_ULP = {}  # operator -> [numpy float64's worst error, the device's], in ulps
_TIES = {"max": 0, "min": 0}


def _modeling():
    from probabilit_amd import modeling

    return modeling


def _name(dt):
    return np.dtype(dt).name


# ------------------------------------------------------------------------------------ inputs
def _random(dt, rng, n):
    if dt == F64:
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
        k = n // 4  # a quarter integer-valued, so that // and % meet exact multiples and ties
        x[:k] = rng.integers(-12, 13, k) * rng.choice([0.25, 0.5, 1.0, 3.0], k)
        return x
    if dt == I64:
        x = rng.integers(-40, 41, n)
        k = n // 4
        x[:k] = rng.integers(IMIN, IMAX, k, endpoint=True)
        return x.astype(np.int64)
    return rng.integers(0, 2, n).astype(bool)


@functools.lru_cache(maxsize=None)
def _pair(dta, dtb):
    """The cross product of the two edge lists, then NRANDOM random pairs (read-only)."""
    rng = np.random.default_rng([11, DTYPES.index(dta), DTYPES.index(dtb)])
    ea, eb = EDGE[dta], EDGE[dtb]
    a = np.concatenate([np.repeat(ea, eb.size), _random(dta, rng, NRANDOM)])
    b = np.concatenate([np.tile(eb, ea.size), _random(dtb, rng, NRANDOM)])
    if dta == dtb == F64:
        # isclose's band: |a - b| next to rtol |b| at magnitudes that drown atol, where a tolerance
        # taken from |a| instead of |b| decides otherwise; both orders
        x = rng.choice([-1.0, 1.0], 200) * 10.0 ** rng.uniform(3, 12, 200)
        y = x * (1.0 + rng.choice([-1.0, 1.0], 200) * 1e-5 * (1.0 + rng.uniform(-2e-5, 2e-5, 200)))
        a, b = np.concatenate([a, x, y]), np.concatenate([b, y, x])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _unary_input(op, dt):
    rng = np.random.default_rng([12, DTYPES.index(dt), sorted(_modeling()._NP_UNARY).index(op)])
    if dt != F64:
        return np.concatenate([EDGE[dt], _random(dt, rng, NRANDOM)])
    u = rng.uniform
    sign = lambda n: rng.choice([-1.0, 1.0], n)  # noqa: E731
    near1 = lambda n: 1.0 - 10.0 ** u(-16, -1, n)  # noqa: E731
    parts = [F_EDGE, _random(F64, rng, 1000)]
    if op in ("arcsin", "arccos", "arctanh"):
        parts += [u(-1, 1, 1000), sign(500) * near1(500), sign(100) * (1.0 + 10.0 ** u(-16, -1, 100)),
                  np.nextafter(1.0, [0.0, 2.0]), -np.nextafter(1.0, [0.0, 2.0])]
    elif op == "arccosh":
        parts += [1.0 + 10.0 ** u(-16, 3, 1500), np.nextafter(1.0, [0.0, 2.0]), 10.0 ** u(0, 300, 300)]
    elif op in ("sin", "cos", "tan"):
        parts += [u(-1e6, 1e6, 1000), u(-7, 7, 500), np.arange(-40, 41) * (np.pi / 4), 10.0 ** u(-300, -1, 200),
                  np.array([1e6, -1e6])]
    elif op in ("exp", "sinh", "cosh"):
        parts += [u(-710, 710, 1200), np.array([710.0, -710.0, 709.78, -709.78]), sign(300) * 10.0 ** u(-300, 0, 300)]
    elif op in ("log", "log10", "sqrt"):
        parts += [10.0 ** u(-320, 308, 1200), 1.0 + sign(300) * 10.0 ** u(-16, -1, 300)]
    elif op in ("tanh", "arctan", "arcsinh"):
        parts += [sign(600) * 10.0 ** u(-300, 0, 600), u(-25, 25, 600), sign(300) * 10.0 ** u(0, 300, 300)]
    else:  # neg abs floor ceil sign square
        parts += [rng.integers(-50, 50, 500) + rng.choice([0.0, 0.5, 0.25, -2.0**-30], 500),
                  sign(300) * 10.0 ** u(-300, 300, 300)]
    return np.concatenate(parts)


# ------------------------------------------------------------------------ device call helpers
class _Out:
    """Replaces modeling._alloc: the output is a view `lead` bytes past PAD sentinel elements of
    a sentinel-filled buffer (lead = 8 puts a float64 output off the 16-byte boundary)."""

    def __init__(self, lead=0):
        self.lead = lead
        self.base = self.dt = self.n = None

    def __call__(self, n, dt):
        import torch

        from probabilit_amd import device

        dt = _modeling()._canonical(dt)
        tdt = {F64: torch.float64, I64: torch.int64, B8: torch.uint8}[dt]
        self.k = self.lead // 8 if dt != B8 else self.lead
        self.base = torch.full((n + 2 * PAD + self.k,), SENT[dt], dtype=tdt, device=device.device())
        self.dt, self.n = dt, n
        view = self.base[PAD + self.k:PAD + self.k + n]
        return view.view(torch.bool) if dt == B8 else view

    def host(self):
        """(values, the whole buffer with the values cut out)."""
        h = self.base.cpu().numpy()
        lo = PAD + self.k
        return h[lo:lo + self.n], np.concatenate([h[:lo], h[lo + self.n:]])


def _flag():
    from probabilit_amd import device

    return device.zeros(1, "int32")


def _call(fn, *args, lead=0, flag="word"):
    """fn(*args, flag pointer) with a padded output.  Returns (values on the host as the
    canonical dtype, flag word, dtype)."""
    m = _modeling()
    out, word = _Out(lead), _flag()
    saved = m._alloc
    m._alloc = out
    try:
        res = fn(*args, word.data_ptr() if flag == "word" else None)
    finally:
        m._alloc = saved
    assert res.data_ptr() == out.base.data_ptr() + (PAD + out.k) * out.base.element_size()
    vals, rest = out.host()
    np.testing.assert_array_equal(rest, np.full(rest.shape, SENT[out.dt], dtype=rest.dtype),
                                  err_msg="sentinels around the output were overwritten")
    if out.dt == B8:
        assert set(np.unique(vals)) <= {0, 1}, "a bool output holds bytes other than 0 and 1"
        vals = vals.astype(bool)
    return vals, int(word.cpu()[0]), out.dt


def _dev(x, n):
    """Device operand: a vector, or a _Broadcast for a 0-d value."""
    from probabilit_amd import device

    if isinstance(x, np.ndarray) and x.ndim == 1:
        return device.to_device(np.array(x))  # a copy: the shared inputs are read-only
    return _modeling()._Broadcast(x, n, np.asarray(x).dtype)


def _host(x, n):
    if isinstance(x, np.ndarray) and x.ndim == 1:
        return x
    return np.full(n, x, dtype=_modeling()._canonical(np.asarray(x).dtype))


# --------------------------------------------------------------------------------- comparing
def _bits(x):
    return x.view(np.uint64) if x.dtype == F64 else x


def assert_same_bits(got, ref, what, skip=None):
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype}{got.shape} vs {ref.dtype}{ref.shape}"
    if got.dtype == F64:
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what}: NaN positions")
        keep = ~np.isnan(ref) if skip is None else ~np.isnan(ref) & ~skip
        got, ref = got[keep].view(np.uint64), ref[keep].view(np.uint64)
    np.testing.assert_array_equal(got, ref, err_msg=what)


def _ulps(x, ref_ld, mask):
    """Largest |x - ref| over the spacing of float64 at ref, on `mask`."""
    if not mask.any():
        return 0.0
    r = ref_ld[mask]
    sp = np.spacing(np.minimum(np.abs(r.astype(np.float64)), 2.0**1023)).astype(LD)  # one spacing per binade
    return float(np.max(np.abs(x[mask].astype(LD) - r) / sp))


def check_rounded(op, got, ref, ref_ld, what):
    special = ~np.isfinite(ref) | (ref == 0.0)
    assert_same_bits(np.where(special, got, 0.0), np.where(special, ref, 0.0), f"{what}: non-finite and zero results")
    mask = ~special & np.isfinite(ref_ld)
    yard, dev = _ulps(ref, ref_ld, mask), _ulps(got, ref_ld, mask)
    print(f"{what}: numpy {yard:.3f} ulp, device {dev:.3f} ulp, gate {8 * max(yard, 0.5):.3f}")
    cur = _ULP.setdefault(op, [0.0, 0.0])
    cur[0], cur[1] = max(cur[0], yard), max(cur[1], dev)
    assert dev <= 8 * max(yard, 0.5), f"{what}: device {dev:.3f} ulp > 8 x max({yard:.3f}, 0.5)"
    assert_close(got[mask], ref_ld[mask].astype(np.float64), rtol=1e-10, what=what)


def _record_ulps():
    record("elementwise_ulp", {k: {"numpy_ulp": v[0], "device_ulp": v[1], "gate_ulp": 8 * max(v[0], 0.5)}
                               for k, v in sorted(_ULP.items())})
    record("elementwise_minmax_zero_ties", dict(_TIES))


def check_minmax(op, got, ref, what):
    tie = (got == 0.0) & (ref == 0.0) & (np.signbit(got) != np.signbit(ref))
    _TIES[op] += int(tie.sum())
    assert_same_bits(got, ref, what, skip=tie)


def _as_ld(x):
    return np.asarray(x).astype(np.float64).astype(LD)


def _expect_flag(ref, neg_pow=False):
    return (1 if ref.dtype.kind == "f" and not np.isfinite(ref).all() else 0) | (2 if neg_pow else 0)


# ============================================================================ A. the grid
def _shapes(dta, dtb):
    yield "vv", None
    for s in SCALARS[dtb]:
        yield "vs", s
    for s in SCALARS[dta]:
        yield "sv", s


@pytest.mark.parametrize("dtb", DTYPES, ids=_name)
@pytest.mark.parametrize("dta", DTYPES, ids=_name)
@pytest.mark.parametrize("op", sorted(["add", "sub", "mul", "truediv", "floordiv", "mod", "pow", "max", "min", "and",
                                       "or", "eq", "ne", "lt", "le", "gt", "ge", "isclose", "arctan2"]))
def test_binary_against_numpy(gpu, op, dta, dtb):
    """Every binary operator on every dtype pair: vector o vector on the cross product of the
    edge lists plus random values, and vector o scalar / scalar o vector for the scalars of
    SCALARS.  An integer power is given the non-negative exponents (numpy raises on the others:
    test_flag_negative_integer_power)."""
    m = _modeling()
    npf = m._NP_BINARY[op]
    va, vb = _pair(dta, dtb)
    try:
        with np.errstate(all="ignore"):
            res_dt = npf(np.ones(1, dta), np.ones(1, dtb)).dtype
    except TypeError:
        for a, b in ((va, vb), (va, SCALARS[dtb][0]), (SCALARS[dta][0], vb)):
            n = va.size
            with pytest.raises(TypeError):
                m._binary(op, _dev(np.asarray(a, dta), n), _dev(np.asarray(b, dtb), n), n, None)
        return
    int_pow = op == "pow" and res_dt.kind in "iu"
    for shape, s in _shapes(dta, dtb):
        a, b = va, vb
        if shape == "vs":
            b = np.asarray(s, dtb)
        elif shape == "sv":
            a = np.asarray(s, dta)
        if int_pow:
            if b.ndim == 0 and b < 0:
                continue
            if b.ndim == 1:
                keep = vb >= 0
                a, b = (a[keep] if a.ndim else a), b[keep]
        n = max(a.size, b.size)
        ha, hb = _host(a, n), _host(b, n)
        with np.errstate(all="ignore"):
            ref = npf(ha, hb)
        ref = ref.astype(m._canonical(ref.dtype))
        got, flag, dt = _call(m._binary, op, _dev(a, n), _dev(b, n), n)
        what = f"{op}({_name(dta)}, {_name(dtb)}) {shape} {s}"
        assert dt == ref.dtype, f"{what}: output dtype {dt}, numpy gives {ref.dtype}"
        if op in EXACT_BINARY or ref.dtype != F64:
            assert_same_bits(got, ref, what)
        elif op in ("max", "min"):
            check_minmax(op, got, ref, what)
        else:
            with np.errstate(all="ignore"):
                ref = npf(ha.astype(np.float64), hb.astype(np.float64))
                ref_ld = npf(_as_ld(ha), _as_ld(hb))
            check_rounded(op, got, ref, ref_ld, what)
        assert flag == _expect_flag(ref), f"{what}: flag word {flag}"
    _record_ulps()


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("op", sorted(["neg", "abs", "log", "exp", "floor", "ceil", "sign", "sqrt", "square", "log10",
                                       "sin", "cos", "tan", "arcsin", "arccos", "arctan", "sinh", "cosh", "tanh",
                                       "arcsinh", "arccosh", "arctanh"]))
def test_unary_against_numpy(gpu, op, dt):
    m = _modeling()
    npf = m._NP_UNARY[op]
    x = _unary_input(op, dt)
    n = x.size
    try:
        with np.errstate(all="ignore"):
            ref = npf(x)
    except TypeError:
        with pytest.raises(TypeError):
            m._unary(op, _dev(x, n), n, None)
        return
    ref = ref.astype(m._canonical(ref.dtype))
    got, flag, odt = _call(m._unary, op, _dev(x, n), n)
    what = f"{op}({_name(dt)})"
    assert odt == ref.dtype, f"{what}: output dtype {odt}, numpy gives {ref.dtype}"
    if op in EXACT_UNARY or ref.dtype != F64:
        assert_same_bits(got, ref, what)
    else:
        with np.errstate(all="ignore"):
            ref = npf(x.astype(np.float64))
            ref_ld = npf(_as_ld(x))
        check_rounded(op, got, ref, ref_ld, what)
        _record_ulps()
    assert flag == _expect_flag(ref), f"{what}: flag word {flag}"


@pytest.mark.parametrize("dt", [I64, B8], ids=_name)
def test_cast_to_float64(gpu, dt):
    """The cast behind distribution parameters and Avg (modeling._as_float_vector)."""
    m = _modeling()
    x = np.concatenate([EDGE[dt], _random(dt, np.random.default_rng(13), NRANDOM)])
    got, flag, odt = _call(lambda a, n, f: m._elementwise("cast", a, None, n, F64, F64, f), _dev(x, x.size), x.size)
    assert odt == F64 and flag == 0
    assert_same_bits(got, x.astype(np.float64), f"cast({_name(dt)})")


def test_required_cases_are_present():
    """The inputs of the grid hold the cases the kernels restate numpy for (host only)."""
    a, b = _pair(F64, F64)
    pairs = set(zip(a.tolist(), b.tolist()))
    for p in [(1.5, 0.0), (-1.5, 0.0), (0.0, 0.0), (np.inf, 3.0), (3.0, np.inf), (-7.0, np.inf), (3.0, -np.inf),
              (-7.0, 3.0), (3.0, -7.0), (-7.0, -1.0), (3.0, -1.5), (-1.5, 0.5), (1e300, 5e-324), (-1e300, 5e-324)]:
        assert p in pairs, p
    assert np.isnan(a).any() and np.isnan(b).any()
    a, b = _pair(I64, I64)
    pairs = set(zip(a.tolist(), b.tolist()))
    for p in [(IMIN, -1), (IMIN, 0), (7, 0), (-7, -1), (-7, 2), (7, -2), (IMAX, 2**53 + 1), (2**53 + 1, IMAX),
              (3, 63), (3, 64), (-7, 2**31), (IMIN + 1, IMAX)]:
        assert p in pairs, p
    a, b = _pair(I64, F64)
    assert (2**53 + 1, 2.0**53) in set(zip(a.tolist(), b.tolist()))
    a, b = _pair(F64, F64)
    fin = np.isfinite(a) & np.isfinite(b)
    with np.errstate(over="ignore"):
        d = np.abs(a[fin] - b[fin])
    assert ((d <= 1e-8 + 1e-5 * np.abs(b[fin])) != (d <= 1e-8 + 1e-5 * np.abs(a[fin]))).sum() >= 20
    a, b = _pair(B8, B8)
    assert set(zip(a.tolist(), b.tolist())) >= {(False, False), (False, True), (True, False), (True, True)}


# ============================================================================ A. flags
@pytest.mark.parametrize("where", ["first", "last"])
def test_flag_single_nonfinite(gpu, where):
    """Clean vectors raise nothing; one non-finite result at index 0 or n - 1 sets bit 1 (value
    1) and nothing else.  A null flag pointer is accepted."""
    m = _modeling()
    n = 4000
    rng = np.random.default_rng(14)
    x, y = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    i = 0 if where == "first" else n - 1
    for op, bad in (("log", 0.0), ("sqrt", -1.0), ("exp", 800.0)):
        got, flag, _ = _call(m._unary, op, _dev(x, n), n)
        assert flag == 0 and np.isfinite(got).all(), op
        z = x.copy()
        z[i] = bad
        got, flag, _ = _call(m._unary, op, _dev(z, n), n)
        assert flag == 1 and not np.isfinite(got[i]) and np.isfinite(np.delete(got, i)).all(), op
        got2, flag2, _ = _call(m._unary, op, _dev(z, n), n, flag=None)
        assert_same_bits(got2, got, op)
    for op, bad in (("floordiv", 0.0), ("mod", 0.0), ("pow", 1e308)):
        got, flag, _ = _call(m._binary, op, _dev(x, n), _dev(y, n), n)
        assert flag == 0 and np.isfinite(got).all(), op
        z = y.copy()
        z[i] = bad
        got, flag, _ = _call(m._binary, op, _dev(x * 2, n), _dev(z, n), n)
        assert flag == 1 and not np.isfinite(got[i]) and np.isfinite(np.delete(got, i)).all(), op
        got2, _, _ = _call(m._binary, op, _dev(x * 2, n), _dev(z, n), n, flag=None)
        assert_same_bits(got2, got, op)
    # outputs that are not float64 never flag, whatever they compare
    got, flag, _ = _call(m._binary, "lt", _dev(np.full(n, np.nan), n), _dev(np.full(n, np.inf), n), n)
    assert flag == 0 and not got.any()


def test_flag_negative_integer_power(gpu):
    """One negative exponent among 4000, at the last index, sets bit 2 (value 2) alone; the
    other elements are numpy's."""
    m = _modeling()
    n = 4000
    rng = np.random.default_rng(15)
    a, b = rng.integers(-9, 10, n), rng.integers(0, 25, n)
    got, flag, dt = _call(m._binary, "pow", _dev(a, n), _dev(b, n), n)
    assert flag == 0 and dt == I64
    np.testing.assert_array_equal(got, np.power(a, b))
    b[-1] = -1
    got, flag, _ = _call(m._binary, "pow", _dev(a, n), _dev(b, n), n)
    assert flag == 2
    np.testing.assert_array_equal(got[:-1], np.power(a[:-1], b[:-1]))
    _call(m._binary, "pow", _dev(a, n), _dev(b, n), n, flag=None)


# ============================================================================ A. sizes
def _cycled(x, n, seed):
    rng = np.random.default_rng(seed)
    return x[rng.permutation(x.size)][np.arange(n) % x.size]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_sizes(gpu, n):
    """One wave short, full, one over; one block short, full, one over; several blocks.  The
    float64 add is taken off the 16-byte boundary so that k_elementwise runs it."""
    m = _modeling()
    fa, fb = (_cycled(v, n, 16) for v in _pair(F64, F64))
    ia, ib = (_cycled(v, n, 17) for v in _pair(I64, I64))
    with np.errstate(all="ignore"):
        for op, a, b, lead in (("add", fa, fb, 8), ("floordiv", fa, fb, 0), ("lt", fa, fb, 0), ("add", ia, ib, 0),
                               ("floordiv", ia, ib, 0), ("lt", ia, ib, 0), ("lt", ia, fb, 0)):
            ref = m._NP_BINARY[op](a, b)
            got, flag, _ = _call(m._binary, op, _dev(a, n), _dev(b, n), n, lead=lead)
            assert_same_bits(got, ref, f"{op} {a.dtype} n={n}")
            assert flag == _expect_flag(ref)


def test_grid_stride(gpu):
    """n = 8192 * 256 + 257: every thread of the capped grid takes a second element, 257 a third."""
    m = _modeling()
    n = 8192 * 256 + 257
    a, b = (_cycled(v, n, 18) for v in _pair(F64, F64))
    with np.errstate(all="ignore"):
        ref = np.floor_divide(a, b)
    got, flag, _ = _call(m._binary, "floordiv", _dev(a, n), _dev(b, n), n)
    assert_same_bits(got, ref, "floordiv grid stride")
    assert flag == 1


# ============================================================================ B. fast path
ARITH = {"add": (1.7e308, 1.7e308), "sub": (1.7e308, -1.7e308), "mul": (1e200, 1e200), "truediv": (1e200, 1e-200)}


def _carve(x, lead):
    """x on the device `lead` bytes past a 16-byte boundary (a view of a padded tensor)."""
    import torch

    from probabilit_amd import device

    buf = torch.full((x.size + 4,), SENT[F64], dtype=torch.float64, device=device.device())
    assert buf.data_ptr() % 16 == 0
    k = lead // 8
    buf[k:k + x.size] = torch.from_numpy(x).to(device.device())
    return buf[k:k + x.size]


def _arith_operand(x, n, lead):
    if isinstance(x, np.ndarray) and x.ndim == 1:
        return _carve(x, lead)
    return _modeling()._Broadcast(x, n, np.asarray(x).dtype)


def _arith_run(op, a, b, n, leads):
    m = _modeling()
    return _call(m._binary, op, _arith_operand(a, n, leads[0]), _arith_operand(b, n, leads[1]), n, lead=leads[2])


ALIGNED = (0, 0, 0)
OFF = [(8, 8, 8), (8, 0, 0), (0, 8, 0), (0, 0, 8)]  # any one of them off the boundary: the generic kernel


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027])
@pytest.mark.parametrize("op", sorted(ARITH))
def test_arith_fast_path_values(gpu, op, n):
    """k_arith_f64 (all three 16-byte aligned) and k_elementwise (one or all of them 8 bytes
    off) against numpy, bit for bit: vector o vector, vector o scalar, scalar o vector with
    float64 and int64 scalars.  No flag: the data is finite."""
    m = _modeling()
    rng = np.random.default_rng([19, n])
    va = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    vb = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
    for a, b in ((va, vb), (va, np.float64(-2.5)), (np.float64(-2.5), vb), (va, np.int64(3)), (np.int64(-7), vb),
                 (va, np.float64(1e-3)), (np.float64(1e3), vb)):
        ref = m._NP_BINARY[op](_host(a, n).astype(np.float64), _host(b, n).astype(np.float64))
        got, flag, dt = _arith_run(op, a, b, n, ALIGNED)
        assert dt == F64 and flag == 0
        assert_same_bits(got, ref, f"{op} n={n} fast")
        for leads in OFF:
            g2, f2, _ = _arith_run(op, a, b, n, leads)
            assert_same_bits(g2, got, f"{op} n={n} generic {leads}")
            assert f2 == 0


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027])
@pytest.mark.parametrize("op", sorted(ARITH))
def test_arith_fast_path_flag(gpu, op, n):
    """One overflow, placed in turn at index 0, in the last full quad and in each tail element:
    the flag word is 1 and the values are numpy's, on both paths."""
    m = _modeling()
    rng = np.random.default_rng([20, n])
    va, vb = rng.uniform(1.0, 2.0, n), rng.uniform(1.0, 2.0, n)
    big_a, big_b = ARITH[op]
    nq = n // 4
    places = sorted({0} | ({4 * nq - 1, 4 * nq - 4} if nq else set()) | set(range(4 * nq, n)))
    for i in places:
        for shape in ("vv", "vs", "sv"):
            a, b = va.copy(), vb.copy()
            if shape != "sv":
                a[i] = big_a
            if shape != "vs":
                b[i] = big_b
            if shape == "vs":
                b = np.float64(big_b)
            elif shape == "sv":
                a = np.float64(big_a)
            with np.errstate(all="ignore"):
                ref = m._NP_BINARY[op](_host(a, n), _host(b, n))
            assert np.isinf(ref[i]) and np.isfinite(np.delete(ref, i)).all()
            for leads in (ALIGNED, OFF[0]):
                got, flag, _ = _arith_run(op, a, b, n, leads)
                assert_same_bits(got, ref, f"{op} n={n} {shape} overflow at {i} {leads}")
                assert flag == 1, f"{op} n={n} {shape} overflow at {i} {leads}: flag {flag}"


def test_arith_fast_path_grid_stride(gpu):
    """n = 4 * 8192 * 256 + 4 * 256 + 3: the quad loop's second pass for one block, a tail of
    three, the only overflow in the last element."""
    m = _modeling()
    n = 4 * 8192 * 256 + 4 * 256 + 3
    rng = np.random.default_rng(21)
    a, b = rng.uniform(1.0, 2.0, n), rng.uniform(1.0, 2.0, n)
    got, flag, _ = _arith_run("add", a, b, n, ALIGNED)
    assert_same_bits(got, a + b, "add grid stride")
    assert flag == 0
    a[-1] = b[-1] = 1.7e308
    got, flag, _ = _arith_run("add", a, b, n, ALIGNED)
    with np.errstate(all="ignore"):
        assert_same_bits(got, a + b, "add grid stride, overflow last")
    assert flag == 1


# ============================================================================ C. pbh_average
def _average(rows, n, m=None, flag=True):
    """pbh_average on device vectors `rows`.  Returns (status, values, flag word)."""
    import torch

    from probabilit_amd import _lib, device

    m = len(rows) if m is None else m
    base = torch.full((n + 2 * PAD,), SENT[F64], dtype=torch.float64, device=device.device())
    word = _flag()
    ptrs = (ctypes.c_void_p * max(len(rows), 1))(*[r.data_ptr() for r in rows])
    rc = _lib.load().pbh_average(ptrs, m, n, base[PAD:].data_ptr(), word.data_ptr() if flag else None, device.stream())
    h = base.cpu().numpy()
    np.testing.assert_array_equal(np.concatenate([h[:PAD], h[PAD + n:]]), np.full(2 * PAD, SENT[F64]))
    return rc, h[PAD:PAD + n], int(word.cpu()[0])


@pytest.mark.parametrize("n", [1, 255, 257, 4097, 8192 * 256 + 257])
@pytest.mark.parametrize("m", [1, 2, 3, 31, 32])
def test_average(gpu, m, n):
    """Rows scaled by 10^+-8, so that any other summation order rounds differently.  The rows are
    windows of one vector of n + m - 1 elements (row j starts at element j), which keeps the
    largest case at 17 MB of input."""
    from probabilit_amd import _lib, device

    rng = np.random.default_rng([22, m, n])
    x = rng.standard_normal(n + m - 1) * 10.0 ** rng.choice([-8.0, 0.0, 8.0], n + m - 1)
    d = device.to_device(x)
    rows = [d[j:j + n] for j in range(m)]
    ref = np.average(np.vstack([x[j:j + n] for j in range(m)]), axis=0)
    rc, got, flag = _average(rows, n)
    assert rc == _lib.OK and flag == 0
    assert_same_bits(got, ref, f"average m={m} n={n}")
    if n <= 257:
        rc, got2, _ = _average(rows, n, flag=False)
        assert rc == _lib.OK
        assert_same_bits(got2, ref, "null flag")


def test_average_order_shows():
    """The data of test_average tells the summation orders apart (host only)."""
    rng = np.random.default_rng([22, 3, 4097])
    x = rng.standard_normal(4097 + 2) * 10.0 ** rng.choice([-8.0, 0.0, 8.0], 4099)
    r = [x[j:j + 4097] for j in range(3)]
    assert ((r[0] + r[1] + r[2]) / 3 != (r[2] + r[1] + r[0]) / 3).any()


def test_average_flag_and_limits(gpu):
    from probabilit_amd import _lib, device

    n = 1000
    rng = np.random.default_rng(23)
    rows = [rng.uniform(1.0, 2.0, n) for _ in range(3)]
    rows[0][n - 1], rows[1][n - 1], rows[2][n - 1] = 1.7e308, 1.7e308, -1.7e308  # the partial sum overflows
    rows[0][5], rows[1][5], rows[2][5] = 1.7e308, -1.7e308, 1.7e308  # this one does not
    with np.errstate(all="ignore"):
        ref = np.average(np.vstack(rows), axis=0)
    assert np.isinf(ref[n - 1]) and np.isfinite(ref[:n - 1]).all()
    dev = [device.to_device(r) for r in rows]
    rc, got, flag = _average(dev, n)
    assert rc == _lib.OK and flag == 1
    assert_same_bits(got, ref, "average with an overflowing partial sum")
    clean = [device.to_device(r[:n - 1].copy()) for r in rows]
    rc, got, flag = _average(clean, n - 1)
    assert rc == _lib.OK and flag == 0
    assert_same_bits(got, ref[:n - 1], "average, no overflow")
    many = [dev[0]] * 33
    for m in (0, 33):  # rejected on the host: the output keeps its sentinels
        rc, got, flag = _average(many, n, m=m)
        assert rc == _lib.ERR_INVALID and "pbh_average" in _lib.last_error()
        np.testing.assert_array_equal(got, np.full(n, SENT[F64]))


# ============================================================================ D. pbh_transpose
def _transpose(a, rows, cols, ld_in, ld_out, out_elems):
    """pbh_transpose of the host buffer `a` into a sentinel-filled buffer of out_elems."""
    import torch

    from probabilit_amd import _lib, device

    din = device.to_device(a)
    dout = torch.full((out_elems,), SENT[F64], dtype=torch.float64, device=device.device())
    rc = _lib.load().pbh_transpose(din.data_ptr(), rows, cols, ld_in, dout.data_ptr(), ld_out, device.stream())
    return rc, dout.cpu().numpy(), din.cpu().numpy()


@pytest.mark.parametrize("rows,cols", list(itertools.product([1, 31, 32, 33, 65], repeat=2)))
def test_transpose(gpu, rows, cols):
    from probabilit_amd import _lib

    ld_in, ld_out = cols + 3, rows + 5
    x = np.random.default_rng([24, rows, cols]).standard_normal((rows, cols))
    a = np.full((rows, ld_in), SENT[F64])
    a[:, :cols] = x
    rc, out, din = _transpose(a.ravel(), rows, cols, ld_in, ld_out, cols * ld_out + PAD)
    assert rc == _lib.OK
    exp = np.full(cols * ld_out + PAD, SENT[F64])
    exp[:cols * ld_out].reshape(cols, ld_out)[:, :rows] = x.T
    np.testing.assert_array_equal(out.view(np.uint64), exp.view(np.uint64))
    np.testing.assert_array_equal(din, a.ravel())


def test_transpose_rejects(gpu):
    """Bad leading dimensions and a column count beyond one launch's grid return the library's
    error before any launch: the output keeps its sentinels."""
    from probabilit_amd import _lib

    wide = 65535 * 32 + 1
    for rows, cols, ld_in, ld_out in ((4, 8, 7, 9), (4, 8, 11, 3), (1, wide, wide, 1)):
        rc, out, _ = _transpose(np.full(64, SENT[F64]), rows, cols, ld_in, ld_out, 64)
        assert rc == _lib.ERR_INVALID and "pbh_transpose" in _lib.last_error()
        np.testing.assert_array_equal(out, np.full(64, SENT[F64]))
