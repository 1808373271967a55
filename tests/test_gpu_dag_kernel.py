"""pbh_dag_eval (k_dag) run on hand-written programs, against numpy and the per-node kernels.

The fused-graph tests (test_gpu_dag.py) compare the fused kernel with the per-node path, which
shares pbh_ops.h with it; here the programs read LOAD vectors and PBH_QSRC_VECTOR quantiles, so
the reference is numpy (and native.ppf / the scipy oracle for the GEN ops).  A tile is 1024
rows in a block of 256; the grid is capped at 4096 blocks.  Every output vector lies between
sentinel elements and the whole buffer is compared.

The operator checks reuse the inputs, the exactness classes and the ulp gates of
test_gpu_elementwise.py (its docstring states them).
"""

import ctypes

import numpy as np
import pytest

import test_gpu_elementwise as E
from test_gpu_elementwise import F64, PAD, SENT, assert_same_bits

pytestmark = pytest.mark.gpu

TILE = 1024
NFLAGS = 8
GEN_PARAMS = {"norm": dict(loc=2.0, scale=3.0), "lognorm": dict(s=0.5, loc=-1.0, scale=1.0),
              "uniform": dict(loc=-1.5, scale=4.0), "expon": dict(loc=0.25, scale=0.7),
              "triang": dict(c=0.3, loc=-1.0, scale=4.0)}
SHAPES = {"lognorm": ("s",), "triang": ("c",)}


def _L():
    from probabilit_amd import _lib

    return _lib


def op(kind, op=0, dst=-1, a=-1, b=-1, src=-1, flag=-1, store=-1, value=0.0, params=(0.0, 0.0, 0.0)):
    o = _L().DagOp()
    o.kind, o.op, o.dst, o.a, o.b, o.src, o.flag, o.store, o.value = kind, op, dst, a, b, src, flag, store, value
    for j in range(3):
        o.params[j] = params[j]
    return o


def load(dst, vec, **kw):
    return op(_L().DAG_LOAD, dst=dst, src=vec, **kw)


def binary(name, a, b, **kw):
    return op(_L().DAG_BINARY, op=_L().OPS[name], a=a, b=b, **kw)


def unary(name, a, **kw):
    return op(_L().DAG_UNARY, op=_L().OPS[name], a=a, **kw)


def gen(name, dst, src, **kw):
    p = GEN_PARAMS[name]
    params = [p[k] for k in SHAPES.get(name, ())] + [p["loc"], p["scale"]]
    return op(_L().DAG_GEN, op=_L().DIST_IDS[name], dst=dst, src=src, params=params + [0.0] * (3 - len(params)), **kw)


def qvector(t, stride=1):
    s = _L().DagSource()
    s.kind, s.q, s.stride = _L().QSRC_VECTOR, t.data_ptr(), stride
    s.tensor = t  # the source holds a bare pointer: keep the quantiles allocated while it is in use
    return s


class Out:
    """An n-row output vector between PAD sentinel elements on either side."""

    def __init__(self, n):
        import torch

        from probabilit_amd import device

        self.n = n
        self.base = torch.full((n + 2 * PAD,), SENT[F64], dtype=torch.float64, device=device.device())

    def data_ptr(self):
        return self.base.data_ptr() + 8 * PAD

    def host(self):
        h = self.base.cpu().numpy()
        np.testing.assert_array_equal(np.concatenate([h[:PAD], h[PAD + self.n:]]), np.full(2 * PAD, SENT[F64]),
                                      err_msg="sentinels around an output vector were overwritten")
        return h[PAD:PAD + self.n]

    def untouched(self):
        np.testing.assert_array_equal(self.base.cpu().numpy(), np.full(self.n + 2 * PAD, SENT[F64]))


def run(ops, n, vectors, sources=(), row0=0, flags=True, nvectors=None):
    """pbh_dag_eval with a zeroed flags tensor.  Returns (status, the NFLAGS flag words)."""
    from probabilit_amd import device

    L = _L()
    word = device.zeros(NFLAGS, "int32")
    arr = (L.DagOp * max(len(ops), 1))(*ops)
    src = (L.DagSource * max(len(sources), 1))(*sources)
    vec = (ctypes.c_void_p * max(len(vectors), 1))(*[v.data_ptr() for v in vectors])
    rc = L.load().pbh_dag_eval(arr, len(ops), src, len(sources), vec, len(vectors) if nvectors is None else nvectors,
                               row0, n, word.data_ptr() if flags else None, device.stream())
    return rc, word.cpu().numpy()


def dev(x):
    from probabilit_amd import device

    return device.to_device(np.array(x, dtype=np.float64))  # a copy: the shared inputs are read-only


def ok(rc):
    assert rc == _L().OK, _L().last_error()


def rejected(rc, text):
    assert rc == _L().ERR_INVALID and text in _L().last_error(), (rc, _L().last_error())


# ============================================================================ 1. operators
IMMEDIATES = [-2.5, 0.0, 3.0, 1.0 + 1e-5, np.inf, np.nan]


def _check_values(name, got, ref, ref_ld, what, exact):
    if exact:
        assert_same_bits(got, ref, what)
    elif name in ("max", "min"):
        E.check_minmax(name, got, ref, what)
    else:
        E.check_rounded(name, got, ref, ref_ld, what)


@pytest.mark.parametrize("name", sorted(["add", "sub", "mul", "truediv", "floordiv", "mod", "pow", "max", "min",
                                         "arctan2"]))
def test_binary_operators(gpu, name):
    """register o register on the cross product of the float64 edge list plus random values,
    register o immediate and immediate o register for six immediates: bit-identical to
    pbh_elementwise, within the elementwise gates of numpy, the same flag."""
    from probabilit_amd import dag

    assert name in dag._BINARY
    m = E._modeling()
    npf = m._NP_BINARY[name]
    a, b = E._pair(F64, F64)
    n = a.size
    da, db = dev(a), dev(b)
    exact = name in E.EXACT_BINARY

    def compare(out, flag, x, y, what):
        got = out.host()
        hx, hy = E._host(x, n), E._host(y, n)
        with np.errstate(all="ignore"):
            ref, ref_ld = npf(hx, hy), npf(E._as_ld(hx), E._as_ld(hy))
        alone, aflag, _ = E._call(m._binary, name, E._dev(x, n), E._dev(y, n), n)
        assert_same_bits(got, alone, f"{what}: k_dag vs pbh_elementwise")
        assert flag == aflag == E._expect_flag(ref), f"{what}: flag {flag}, pbh_elementwise {aflag}"
        _check_values(name, got, ref, ref_ld, what, exact)

    out = Out(n)
    rc, flags = run([load(0, 0), load(1, 1), binary(name, 0, 1, flag=0, store=2)], n, [da, db, out])
    ok(rc)
    assert not flags[1:].any()
    compare(out, flags[0], a, b, f"{name} reg o reg")
    for s in IMMEDIATES:
        o1, o2 = Out(n), Out(n)
        rc, flags = run([load(0, 0), binary(name, 0, -1, value=s, flag=0, store=1),
                         binary(name, -1, 0, value=s, flag=1, store=2)], n, [da, o1, o2])
        ok(rc)
        assert not flags[2:].any()
        compare(o1, flags[0], a, np.float64(s), f"{name} reg o {s}")
        compare(o2, flags[1], np.float64(s), a, f"{name} {s} o reg")
    E._record_ulps()


@pytest.mark.parametrize("name", sorted(["neg", "abs", "log", "exp", "floor", "ceil", "sign", "sqrt", "square",
                                         "log10", "sin", "cos", "tan", "arcsin", "arccos", "arctan", "sinh", "cosh",
                                         "tanh", "arcsinh", "arccosh", "arctanh"]))
def test_unary_operators(gpu, name):
    m = E._modeling()
    npf = m._NP_UNARY[name]
    x = E._unary_input(name, F64)
    n = x.size
    out, out2 = Out(n), Out(n)
    rc, flags = run([load(0, 0), unary(name, 0, flag=0, store=1), unary(name, -1, value=1.5, flag=1, store=2)], n,
                    [dev(x), out, out2])
    ok(rc)
    got = out.host()
    with np.errstate(all="ignore"):
        ref, ref_ld = npf(x), npf(E._as_ld(x))
        ref2 = npf(np.full(n, 1.5))
    alone, aflag, _ = E._call(m._unary, name, E._dev(x, n), n)
    assert_same_bits(got, alone, f"{name}: k_dag vs pbh_elementwise")
    assert flags[0] == aflag == E._expect_flag(ref) and not flags[2:].any()
    _check_values(name, got, ref, ref_ld, name, name in E.EXACT_UNARY)
    alone2, aflag2, _ = E._call(lambda a, k, f: m._elementwise(name, a, None, k, F64, F64, f), E._dev(np.float64(1.5), n), n)
    assert_same_bits(out2.host(), alone2, f"{name}(immediate): k_dag vs pbh_elementwise")
    assert flags[1] == aflag2 == E._expect_flag(ref2)
    E._record_ulps()


def test_cast_and_store(gpu):
    """CAST is the identity on float64; STORE writes a register or its immediate."""
    L = _L()
    x = E.F_EDGE
    n = x.size
    o1, o2, o3 = Out(n), Out(n), Out(n)
    rc, flags = run([load(0, 0), unary("cast", 0, store=1), op(L.DAG_STORE, a=0, store=2),
                     op(L.DAG_STORE, a=-1, value=-0.0, store=3)], n, [dev(x), o1, o2, o3])
    ok(rc)
    assert_same_bits(o1.host(), x, "cast")
    assert_same_bits(o2.host(), x, "store of a register")
    assert_same_bits(o3.host(), np.full(n, -0.0), "store of an immediate")
    assert not flags.any()


# ============================================================================ 2. tiles
def _axpy(n):
    rng = np.random.default_rng([31, n])
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    out = Out(n)
    rc, flags = run([load(0, 0), binary("mul", 0, -1, value=1.0 / 3.0, dst=0), load(1, 1),
                     binary("add", 0, 1, flag=0, store=2)], n, [dev(a), dev(b), out])
    ok(rc)
    assert not flags.any()
    assert_same_bits(out.host(), a * (1.0 / 3.0) + b, f"n={n}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_tiles(gpu, n):
    _axpy(n)


def test_grid_stride(gpu):
    """4096 * 1024 + 1025 rows: block 0 takes a second full tile, block 1 a tile of one row."""
    _axpy(4096 * TILE + 1025)


# ============================================================================ 3. padding rows
def _padding_program(v0, v1, q, outs):
    """flag 0: Log(LOAD v0); flag 1: 1.0 / LOAD v1; flag 2: GEN uniform(-0.5, 1); flag 3: Log(GEN).
    A padding row holds LOAD = 0.0 and q = 0.5, so each of the three nodes is non-finite there."""
    L = _L()
    g = op(L.DAG_GEN, op=L.DIST_IDS["uniform"], dst=2, src=0, flag=2, params=(-0.5, 1.0, 0.0))
    prog = [load(0, 0, flag=4), unary("log", 0, flag=0, store=2), load(1, 1, flag=5),
            binary("truediv", -1, 1, value=1.0, flag=1, store=3), g, unary("log", 2, flag=3, store=4)]
    return run(prog, v0.shape[0], [v0, v1] + outs, [qvector(q)])


@pytest.mark.parametrize("bad", [None, "log", "div", "gen"])
def test_padding_rows_raise_no_flag(gpu, bad):
    """n = 1025: the second tile has one valid row and 1023 padding rows.  Over strictly positive
    data every flag word stays 0; one bad valid row sets its node's word and no other."""
    n = 1025
    rng = np.random.default_rng(32)
    v0, v1, q = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n), rng.uniform(0.6, 0.9, n)
    expect = np.zeros(NFLAGS, dtype=np.int32)
    if bad == "log":
        v0[700] = 0.0
        expect[0] = 1
    elif bad == "div":
        v1[1024] = 0.0
        expect[1] = 1
    elif bad == "gen":
        q[1024] = 0.5
        expect[3] = 1
    outs = [Out(n), Out(n), Out(n)]
    rc, flags = _padding_program(dev(v0), dev(v1), dev(q), outs)
    ok(rc)
    np.testing.assert_array_equal(flags, expect)
    with np.errstate(all="ignore"):
        assert_same_bits(outs[1].host(), 1.0 / v1, "1 / LOAD")
        for o, x in ((outs[0], v0), (outs[2], q - 0.5)):
            got, ref = o.host(), np.log(x)
            np.testing.assert_array_equal(np.isfinite(got), np.isfinite(ref))
            E.assert_close(got, ref, rtol=1e-10)


# ============================================================================ 4. GEN
def _tail_q(rng, k):
    """Quantiles that take PPND16's tail: |q - 0.5| > 0.425."""
    lo = np.concatenate([rng.uniform(1e-3, 0.0749, k - k // 4), 10.0 ** rng.uniform(-300, -3, k // 4)])
    return np.where(rng.integers(0, 2, k) == 1, lo, 1.0 - np.clip(lo, 2.0**-53, 0.0749))[rng.permutation(k)]


def _guard_q(name):
    """The quantile vector of test_norm_lognorm_cancellation_guard (test_gpu_ppf.py)."""
    import scipy.stats

    q0 = 0.5 if name == "lognorm" else float(scipy.stats.norm(**GEN_PARAMS["norm"]).cdf(0.0))
    offs = np.concatenate([-np.logspace(-15, -3, 400), [0.0], np.logspace(-15, -3, 400)])
    q = np.clip(q0 + offs, 1e-300, 1 - 2.0**-53)
    return np.concatenate([q, np.nextafter(q0, 0.0) - np.arange(50) * 2.0**-54,
                           np.nextafter(q0, 1.0) + np.arange(50) * 2.0**-53])


def _gen_q(kind, name, n):
    rng = np.random.default_rng([33, n])
    if kind == "all_tail":
        return _tail_q(rng, n)
    if kind == "no_tail":
        return rng.uniform(0.075, 0.925, n)
    if kind == "one_tail_last":
        q = rng.uniform(0.075, 0.925, n)
        q[-1] = 1e-9
        return q
    g, t = _guard_q(name), _tail_q(rng, n)  # guard and tail quantiles alternate within every wave
    q = t.copy()
    q[0::2] = g[np.arange((n + 1) // 2) % g.size]
    return q


GEN_CASES = [(name, kind) for name in ["norm", "lognorm", "uniform", "expon", "triang"]
             for kind in ["all_tail", "no_tail", "one_tail_last"]] + [("norm", "guard_and_tail"),
                                                                     ("lognorm", "guard_and_tail")]


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("n", [1024, 1027])
@pytest.mark.parametrize("name,kind", GEN_CASES)
def test_gen(gpu, name, kind, n, stride):
    """A GEN from a quantile vector: bit-identical to native.ppf on the same q, within 1e-10 of
    the scipy oracle.  all_tail fills the tail queue of the first tile (1024 entries).
    guard_and_tail puts the quantiles next to the zero crossing of loc + scale z (norm) and
    loc + scale exp(s z) (lognorm), which take ndtri whole, between tail quantiles.  For lognorm
    next to its crossing the bound is the one test_norm_lognorm_cancellation_guard derives: exp(s z)
    ~ 1 is within an ulp of libm's and loc + scale exp(s z) keeps that ulp absolutely, so
    4 spacing(|loc|) is added to the 1e-10 relative bound there."""
    from oracle.ppf import ppf as ref_ppf
    from probabilit_amd import native

    q = _gen_q(kind, name, n)
    assert kind != "all_tail" or (np.abs(q - 0.5) > 0.425).all()
    assert kind != "no_tail" or (np.abs(q - 0.5) <= 0.425).all()
    wide = np.full(n * stride, np.nan)
    wide[::stride] = q
    dq = dev(wide)
    out = Out(n)
    rc, flags = run([gen(name, 0, 0, flag=0, store=0)], n, [out], [qvector(dq, stride)])
    ok(rc)
    got = out.host()
    assert not flags.any()
    assert_same_bits(got, native.ppf(name, q, **GEN_PARAMS[name]), f"{name} {kind} vs native.ppf")
    atol = 4 * np.spacing(abs(GEN_PARAMS[name]["loc"])) if (name, kind) == ("lognorm", "guard_and_tail") else 0.0
    E.assert_close(got, ref_ppf(name, q, **GEN_PARAMS[name]), rtol=1e-10, atol=atol, what=f"{name} {kind} vs scipy")


@pytest.mark.parametrize("name", ["norm", "lognorm", "uniform", "expon", "triang"])
def test_gen_flag(gpu, name):
    """q = 0, 1 and nan, one at a time at the last of 1027 rows: the GEN's word is set exactly
    when scipy's value there is not finite, and no other word."""
    from oracle.ppf import ppf as ref_ppf

    n = 1027
    q = np.random.default_rng(34).uniform(0.01, 0.99, n)
    for bad in (0.0, 1.0, np.nan):
        q[-1] = bad
        ref = ref_ppf(name, q, **GEN_PARAMS[name])
        assert np.isfinite(ref[:-1]).all()
        out, out2, dq = Out(n), Out(n), dev(q)
        rc, flags = run([gen(name, 1, 0, flag=3, store=0), unary("square", 1, flag=-1, store=1)], n, [out, out2],
                        [qvector(dq)])
        ok(rc)
        expect = np.zeros(NFLAGS, dtype=np.int32)
        expect[3] = 0 if np.isfinite(ref[-1]) else 1
        np.testing.assert_array_equal(flags, expect, err_msg=f"{name} q={bad}")
        E.assert_close(out.host(), ref, rtol=1e-10, what=f"{name} q={bad}")


# ============================================================================ 5. row0
@pytest.mark.parametrize("name,col", [("norm", 0), ("expon", 2)])
def test_lhs_source_row0(gpu, name, col):
    from probabilit_amd import native

    L = _L()
    seed, n_total, row0, n = 12345, 5000, 777, 1500
    s = L.DagSource()
    s.kind, s.seed, s.n_total, s.col = L.QSRC_LHS, seed, n_total, col
    out = Out(n)
    rc, flags = run([gen(name, 0, 0, flag=0, store=0)], n, [out], [s], row0=row0)
    ok(rc)
    q = native.fill_lhs(seed, n_total, col + 1)[row0:row0 + n, col]
    assert_same_bits(out.host(), native.ppf(name, np.ascontiguousarray(q), **GEN_PARAMS[name]), "LHS rows 777..2276")
    assert not flags.any()
    rc, _ = run([gen(name, 0, 0, store=0)], n, [Out(n)], [s], row0=n_total - n + 1)
    rejected(rc, "bad LHS rows")


@pytest.mark.parametrize("size", [1025, 4096 * TILE + 1])
def test_sobol_source_through_sample(gpu, monkeypatch, size):
    """A Sobol' source is driven through Node.sample and compared with the per-node path."""
    from probabilit_amd import dag
    from probabilit_amd import modeling as m

    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("PBH_DAG", flag)
        a, b = m.Distribution("norm", loc=1.0, scale=2.0), m.Distribution("uniform", loc=0.5, scale=3.0)
        sink = a * 2.0 + b
        before = dag.counts["fused"]
        sink.sample(size=size, random_state=5, method="sobol", gc_strategy=[])
        assert (dag.counts["fused"] > before) == (flag == "1")
        res.append(np.array(sink.samples_, copy=True))
    assert res[0].shape == (size,)
    np.testing.assert_array_equal(res[0], res[1])


# ============================================================================ 6. registers
def test_sixteen_registers(gpu):
    """Sixteen LOADs live at once (16 x 8 KiB of LDS registers), then a left-to-right sum."""
    L = _L()
    n = 1027
    rng = np.random.default_rng(35)
    vs = [rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9) for _ in range(L.DAG_MAX_REGS)]
    prog = [load(r, r) for r in range(16)]
    prog += [binary("add", 0, r, dst=0) for r in range(1, 15)] + [binary("add", 0, 15, flag=0, store=16)]
    out = Out(n)
    rc, flags = run(prog, n, [dev(v) for v in vs] + [out])
    ok(rc)
    ref = vs[0]
    for v in vs[1:]:
        ref = ref + v
    assert_same_bits(out.host(), ref, "sum of sixteen registers")
    assert not flags.any()
    out = Out(n)
    rc, _ = run(prog[:16] + [load(16, 0)] + prog[16:], n, [dev(v) for v in vs] + [out])
    rejected(rc, "bad register")
    out.untouched()


# ============================================================================ 7. argument checks
def test_argument_checks(gpu):
    """Rejected on the host, before any launch: the output keeps its sentinels."""
    L = _L()
    n = 100
    x, out = dev(np.ones(n)), Out(n)
    good = [load(0, 0), unary("neg", 0, flag=0, store=1)]
    for prog, text, kw in (
            ([load(0, 0), op(9, dst=0, a=0, store=1)], "unknown kind", {}),
            ([load(0, 0), binary("lt", 0, 0, store=1)], "unknown operator", {}),
            ([load(0, 0), unary("add", 0, store=1)], "unknown operator", {}),
            ([load(0, 0), unary("neg", 0, store=2)], "bad store vector", {}),
            ([load(0, 2)], "bad vector", {}),
            (good, "without a flags array", dict(flags=False))):
        rc, _ = run(prog, n, [x, out], **kw)
        rejected(rc, text)
        out.untouched()
    s = L.DagSource()
    s.kind, s.bits = L.QSRC_SOBOL, 10
    rc, _ = run([gen("norm", 0, 0, store=1)], 1025, [x, Out(1025)], [s])
    rejected(rc, "rows exceed 2^bits")
    for nn, prog in ((0, good), (n, [])):
        rc, flags = run(prog, nn, [x, out])
        ok(rc)
        out.untouched()
        assert not flags.any()
    rc, flags = run(good, n, [x, out])
    ok(rc)
    assert_same_bits(out.host(), -np.ones(n), "neg")


# ============================================================================ Avg of one row
@pytest.mark.parametrize("m", [7, 8, 9, 20, 32])
def test_avg_node_single_row(gpu, m):
    """Avg at size 1: numpy sums a single column of 8 or more parents with eight accumulators,
    not left to right; k_average follows it and the fused program leaves that shape to it."""
    from probabilit_amd import modeling as md

    ds = [md.Distribution("norm", loc=float(j), scale=10.0 ** (8 * (j % 3 - 1))) for j in range(m)]
    sink = md.Avg(*ds)
    sink.sample(size=1, random_state=m)
    ref = np.average(np.vstack([d.samples_ for d in ds]), axis=0)
    assert_same_bits(np.asarray(sink.samples_), ref, f"Avg of {m} parents, one row")
