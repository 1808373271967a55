"""The generated-column step-4 kernels (pbh_step4.hip) on crafted scores, one column at a time.

pbh_ic_owned_column(h, i, cs, NULL, 1, p_out, ...) runs k_make_codes, k_hist16 / k_hist16c and
k_hist16_scan, the adaptive code map (k_adapt_reset, k_seg_hist, k_seg_map, k_make_codes_adapt
and the re-count), k_msd1x, k_msd2x, k_finish_q, k_place_msdo and k_place_positions on any cs
vector and returns p[r] = rank(cs[r]) - 1.  pbh_ic_owned_finish reports the columns the general
path redid, pbh_ic_owned_verdict the words the passes left: state (bit 0 a saturated 16-bit
counter, bit 1 a bucket above 2048), flags (bit 0 a bin above 32, bit 2 not flat after the
re-code) and retry.  k_adapt_reset clears the first count's state word, so after a re-code
state is the second count's: why the fixed map was rejected shows on the device as retry = 1
and is asserted here as a precondition, on the host.

Reference of every result: scipy.stats.rankdata(cs, "average").astype(int64) - 1, exactly.  cs
and p_out (or y) are views inside sentinel buffers that are compared whole.  In y-mode
y == sorted[p] with sorted from pbh_lhs_sorted_ppf.

The host mirrors (code_of of test_gpu_sortrank.py for the fixed map, adapt_codes below for
k_seg_hist / k_seg_map / code_of with the 4096-segment map, predict for the verdict words) build
inputs and assert their preconditions ("this bucket holds exactly 2048 items", "every bin holds
<= 32 after the re-code"); the verdict a case expects is written in the case, and the mirrors
must agree with it before the device is asked.

A  sizes on shuffled N(0, 1) scores, with the launch counts (k_place_msd: 0 up to 2^20, 1 above).
B  kBucketCap2 = 2048: a bucket of 2048 is finished, 2049 re-code the column (then flat).
C  kBinCap = 32: bins (32 adjacent codes) of 32 pass, 33 flag the column; codes 0 / 0xFFFFFFFF.
D  exact ties: every member of a group at sorted positions [a, a + e) receives a + (e - 1) // 2.
E  the adaptive code map, with the verdict after the re-code; three columns of one handle.
F  re-use of a column index and of a workspace.

k_hist16_q is open: step4_gen_adapt launches it only for kk > 1 columns in one call, and both
callers (the lanes of pbh_iman_conover and pbh_ic_owned_column) re-code one column at a time
(kk = 1: k_hist16 / k_hist16c with the gate), so no entry point reaches it, whatever the column
list; its success path has no test.

Mutation check (each change built into a scratch library, the 62 cases of this file run against
it on an MI355X; failing cases):
    mx > kBucketCap2 -> >=                             5    bucket_capacity[*-2048] (retry 1 for 0)
    be - bs > kBinCap -> >=                            7    bin_capacity[*-32], ties[32-*], ties[31-beside]
    eq / 2 -> (eq + 1) / 2                            10    ties[2-*, 4-*, 32-*], ties_zeros_and_ends: the
                                                            groups of even length
    pass 2 without the xm < xv term                   18    bin_capacity[*-32], ties[*-beside], sizes from
                                                            65536 (chance pairs of one code), peaks,
                                                            segment_edge, bucket_capacity[last-2049], the
                                                            three-column handle
    k_adapt_reset without the cur2 (or curF) clear     0    equivalent: step4_gen_hist zeroes the cursors and
                                                            nothing advances them before the re-code, in
                                                            either caller; the clear only repeats it
    k_seg_map bases without + j                        0    equivalent below 2^32 rows: a segment that holds
                                                            an item keeps >= 1 code from its share of the
                                                            span alone, and no item lies in an empty one
    k_hist16 saturation test == 0xFFFF -> == 0xFFFE    1    adaptive_map[outside_65535] (state 3 for 2).  The
                                                            other direction, a test that never fires, was
                                                            not run: the wrapped histogram would make the
                                                            later passes write out of bounds;
                                                            adaptive_map[outside_65536] expects state 1
    place_levels without the bits - 8 top shift        0    equivalent in its result: it is the PBH_PLACE_TOP=0
                                                            configuration (test_step4_variants_match_the_
                                                            oracle), and no timed count tells the two apart
    gstart taken at (t & 3) == 1                       -    not run: k_msd1x would write past its groups and
                                                            the finish scatter by rows it never wrote.  By
                                                            reading, cstart is wrong for every top byte
                                                            whose first 64 buckets hold an item: every case
    k_place_positions last partial block one row short 47   every case with n no multiple of 4096
"""

import ctypes
import functools
import zlib

import numpy as np
import pytest

from test_gpu_sortrank import Launches, View, _ro, _ws, chain, code_of, index_ref, x_of_code

pytestmark = pytest.mark.gpu

SEED = 20240611
BUCKET_CAP, BIN_CAP, BIN_SHIFT = 2048, 32, 5
ADAPT_M, ADAPT_X0 = 4096, -8.5
ADAPT_W = 17.0 / ADAPT_M


# ---------------------------------------------------------------------------- host mirrors
def adapt_codes(cs):
    """k_seg_hist, k_seg_map and code_of with the adaptive map of the column cs, as int64."""
    x = np.asarray(cs, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - ADAPT_X0) * (1.0 / ADAPT_W)
        inside = (u >= 0.0) & (u < float(ADAPT_M))
        j = np.where(inside, u, 0.0).astype(np.int64)
        seg = np.bincount(j[inside], minlength=ADAPT_M)
        cum = np.concatenate(([0], np.cumsum(seg)[:-1])).astype(np.float64)
        total = float(seg.sum()) if seg.sum() else 1.0
        span = 4294967295.0 - ADAPT_M
        base = np.floor(cum * span / total).astype(np.int64) + np.arange(ADAPT_M)
        base = np.concatenate((base, [4294967295]))
        assert (np.diff(base) > 0).all() and base[0] == 0
        cnt = base[1:] - base[:-1]
        slope = cnt.astype(np.float64) * (1.0 / ADAPT_W)
        lo = ADAPT_X0 + j.astype(np.float64) * ADAPT_W
        off = np.nan_to_num(np.floor((x - lo) * slope[j]), nan=0.0, posinf=0.0, neginf=0.0)
    code = base[j] + np.clip(off, 0, cnt[j] - 1).astype(np.int64)
    return np.where(~(u >= 0.0), 0, np.where(u >= ADAPT_M, 0xFFFFFFFF, code))


def bucket_counts(codes):
    return np.bincount(codes >> 16, minlength=65536)


def largest_bin(codes):
    return int(np.unique(codes >> BIN_SHIFT, return_counts=True)[1].max())


def count_state(codes):
    """state after one count of a column's codes.  Bit 0 (a block's packed counter asked to hold
    65536) is mirrored for one histogram block only (n <= 65536), where it means a bucket of 65536
    items; the counter wraps, the bucket then counts as empty (with a carry of one into its odd
    neighbour) and bit 1 stays clear."""
    h = bucket_counts(codes)
    if h.max() >= 65536:
        assert len(codes) <= 65536, "saturation is mirrored for one histogram block only"
        return 1
    return 2 if h.max() > BUCKET_CAP else 0


def monotone(cs, codes):
    return bool((np.diff(codes[np.argsort(cs, kind="stable")]) >= 0).all())


def predict(cs):
    """((state, flags, retry, redone) as the passes leave them, the first count's state, the codes
    the finish saw)."""
    codes = code_of(cs)
    assert monotone(cs, codes), "the fixed code is not monotone"
    first = count_state(codes)
    if first:
        codes = adapt_codes(cs)
        assert monotone(cs, codes), "the adaptive code is not monotone"
    state = count_state(codes)
    flags = 4 if state else int(largest_bin(codes) > BIN_CAP)
    return (state, flags, int(first != 0), int(state != 0 or flags != 0)), first, codes


# ---------------------------------------------------------------------------- the harness
class Column:
    def __init__(self, cs, redone, state, flags, retry, out):
        self.cs, self.out = cs, out
        self.verdict = (state, flags, retry, redone)


def owned_run(css, order=None, y_mode=False, ws=None, twice=False):
    """One owned handle of len(css) norm columns; column i ranks css[i] into p_out (or into y).
    Returns the columns (verdicts read, cs compared), the launches and the workspace.  twice:
    every column is launched a second time, which must be refused."""
    from probabilit_amd import _lib, device

    lib = _lib.load()
    m, n = len(css), len(css[0])
    nf = device.zeros(m, "int32")
    cols = (_lib.ICColumn * m)(*[_lib.ICColumn(SEED, i, _lib.DIST_IDS["norm"], (ctypes.c_double * 4)(0.0, 1.0), 2,
                                               nf.data_ptr() + 4 * i) for i in range(m)])
    nb = ctypes.c_size_t()
    _lib.check(lib.pbh_ic_owned_workspace_size(n, m, ctypes.byref(nb)))
    if ws is None:
        ws = _ws(nb.value)
    assert ws.numel() >= nb.value
    h = ctypes.c_void_p()
    _lib.check(lib.pbh_ic_owned_create(cols, m, n, ws.data_ptr(), nb.value, ctypes.byref(h), device.stream()),
               "pbh_ic_owned_create")
    cin = [View(n, host=cs) for cs in css]
    out = [View(n) if y_mode else View(n, dtype=np.int32) for _ in css]
    redone = np.full(m + 2, -5, dtype=np.int32)
    verdicts = []
    try:
        with Launches() as L:
            for i in (order or range(m)):
                args = (h, i, cin[i].ptr(), out[i].ptr() if y_mode else None, 1, None if y_mode else out[i].ptr(),
                        None, None, device.stream())
                _lib.check(lib.pbh_ic_owned_column(*args), "pbh_ic_owned_column")
                if twice:
                    assert lib.pbh_ic_owned_column(*args) == _lib.ERR_INVALID
                    assert "already launched" in _lib.last_error()
            _lib.check(lib.pbh_ic_owned_finish(h, redone[1:].ctypes.data, device.stream()), "pbh_ic_owned_finish")
        for i in range(m):
            s, f, r = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
            _lib.check(lib.pbh_ic_owned_verdict(h, i, ctypes.byref(s), ctypes.byref(f), ctypes.byref(r)),
                       "pbh_ic_owned_verdict")
            verdicts.append((s.value, f.value, r.value))
        w = ctypes.c_int32()
        assert lib.pbh_ic_owned_verdict(h, m, ctypes.byref(w), ctypes.byref(w), ctypes.byref(w)) == _lib.ERR_INVALID
    finally:
        _lib.check(lib.pbh_ic_owned_destroy(h, device.stream()), "pbh_ic_owned_destroy")
    assert redone[0] == -5 and redone[m + 1] == -5, "redone_host written outside its m words"
    assert (device.to_host(nf) == 0).all()
    for c in cin:
        c.check(what="cs changed")
    return [Column(css[i], int(redone[1 + i]), *verdicts[i], out[i]) for i in range(m)], L, ws


@functools.lru_cache(maxsize=None)
def sorted_column(n, col):
    """sort(X[:, col]) of the handle's norm column, from pbh_lhs_sorted_ppf."""
    from probabilit_amd import _lib, device

    out = device.empty(n)
    _lib.check(_lib.load().pbh_lhs_sorted_ppf(SEED, n, 0, n, col, _lib.DIST_IDS["norm"], (ctypes.c_double * 2)(0.0, 1.0),
                                              2, out.data_ptr(), None, device.stream()), "pbh_lhs_sorted_ppf")
    return _ro(device.to_host(out))


def check_positions(col, r, distinct):
    col.out.check(r, "p_out")
    if distinct:
        assert np.array_equal(np.sort(col.out.get()), np.arange(len(r))), "p_out is no permutation"


def run_case(cs, expect, distinct=True, y_mode=False, first=None):
    """One column through a handle of its own: the mirrors agree with the verdict the case expects
    (and with the first count's state, when given), then the device gives that verdict and the
    reference positions; (launches, reference, column)."""
    n = len(cs)
    if distinct:
        assert len(np.unique(cs)) == n, "the values are not distinct"
    pred, first_state, codes = predict(cs)
    assert pred == expect, f"precondition: the mirrors predict {pred}, the case expects {expect}"
    assert first is None or first_state == first, "precondition: the first count's state"
    if expect[1] == 0:
        assert bucket_counts(codes).max() <= BUCKET_CAP and largest_bin(codes) <= BIN_CAP
    r = index_ref(cs)
    cols, L, _ = owned_run([cs])
    print(f"n={n} verdict (state, flags, retry, redone) = {cols[0].verdict}")
    assert cols[0].verdict == expect, "(state, flags, retry, redone)"
    check_positions(cols[0], r, distinct)
    if y_mode:
        ycols, _, _ = owned_run([cs], y_mode=True)
        assert ycols[0].verdict == expect
        ycols[0].out.check(sorted_column(n, 0)[r], "y")
    return L, r, cols[0]


CLEAN, RECODED = (0, 0, 0, 0), (0, 0, 1, 0)
BIN_OVER, BIN_OVER_RECODED = (0, 1, 0, 1), (0, 1, 1, 1)


def background(n, rng, keep_out=()):
    """n N(0, 1) scores of which none lies in the top-16 buckets `keep_out`."""
    cs = rng.normal(size=n)
    for _ in range(100):
        hit = np.isin(code_of(cs) >> 16, keep_out)
        if not hit.any():
            break
        cs[hit] = rng.normal(size=int(hit.sum()))
    assert not np.isin(code_of(cs) >> 16, keep_out).any()
    return cs


def plant(cs, rng, vals):
    """vals on random rows of cs, in shuffled order."""
    vals = np.asarray(vals, dtype=np.float64)
    cs = cs.copy()
    cs[rng.choice(len(cs), size=len(vals), replace=False)] = rng.permutation(vals)
    return cs


def xs_of(codes):
    x = np.array([x_of_code(int(c)) for c in codes])
    assert np.array_equal(code_of(x), np.asarray(codes, dtype=np.int64)), "x_of_code misses its code"
    return x


def bucket_at(x):
    return int(code_of(x)) >> 16


def seeded(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else k for k in key])


# ---------------------------------------------------------------------------- A
SIZES = [2, 3, 4095, 4096, 4097, 8191, 8192, 8193, 65536, 65537, 458752, 458753, 1 << 20, (1 << 20) + 1, (1 << 21) + 1]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    """Shuffled N(0, 1) scores: clean verdicts, exact positions, a permutation; every step-4 pass
    is launched once, and k_place_msdo once above 2^20 rows (two placement levels), never below."""
    cs = seeded(21, n).normal(size=n)
    L = run_case(cs, CLEAN, y_mode=n in (3, 4097, (1 << 20) + 1))[0]
    for name in ("k_make_codes", "k_hist16", "k_msd1", "k_msd2", "k_finish", "k_place_gen"):
        assert L[name] == 1, name
    assert L["k_place_msd"] == (1 if n > 1 << 20 else 0), "k_place_msdo launches"


# ---------------------------------------------------------------------------- B
def full_bucket_codes(b, count):
    """`count` codes of bucket b, one per bin (32 codes apart); the 2049th shares the sixth bin."""
    c = (b << 16) + 32 * np.arange(min(count, 2048)) + 7
    return np.concatenate((c, [(b << 16) + 32 * 5 + 20])) if count > 2048 else c


def bucket_cases():
    odd = (bucket_at(0.3) // 64) * 64 + 63  # odd, and the last of a k_hist16_scan thread's 64
    even = bucket_at(-1.1) & ~1
    out = {}
    for name, b in (("first", 0), ("last", 65535), ("odd", odd), ("scan_first", (bucket_at(0.9) // 64) * 64)):
        out[f"{name}-2048"] = ([(b, 2048)], CLEAN)
        out[f"{name}-2049"] = ([(b, 2049)], RECODED)
    out["pair-2048-2048"] = ([(even, 2048), (even + 1, 2048)], CLEAN)  # one k_finish_q block
    out["pair-2048-2049"] = ([(even, 2048), (even + 1, 2049)], RECODED)
    out["pair-2049-2048"] = ([(even, 2049), (even + 1, 2048)], RECODED)
    return out


BUCKET_CASES = bucket_cases()


@pytest.mark.parametrize("name", sorted(BUCKET_CASES))
def test_bucket_capacity(gpu, name):
    """n = 20 000: a top-16 bucket of exactly 2048 distinct codes is finished under the fixed map;
    2049 re-code the column (first count: state bit 1), which is flat afterwards.  The first, the
    last, an odd bucket that ends a scan thread's 64, one that starts them, and both buckets of
    one finish block."""
    fill, expect = BUCKET_CASES[name]
    rng = seeded(22, name)
    cs = background(20_000, rng, [b for b, _ in fill])
    cs = plant(cs, rng, np.concatenate([xs_of(full_bucket_codes(b, count)) for b, count in fill]))
    codes = code_of(cs)
    h = bucket_counts(codes)
    for b, count in fill:
        assert h[b] == count, "precondition: the bucket's size under the fixed map"
    assert np.sort(h)[-len(fill) - 1] < 100 and largest_bin(codes) <= 2
    run_case(cs, expect, y_mode=name in ("odd-2048", "odd-2049"), first=2 if expect[2] else 0)


# ---------------------------------------------------------------------------- C
def spread_bin(c0, per_code, codes):
    """per_code distinct values in each of `codes` codes 4 apart from c0: one bin, c0 % 32 == 0."""
    assert c0 % 32 == 0 and 4 * (codes - 1) < 32
    return np.concatenate([chain(x_of_code(c0 + 4 * k), per_code) for k in range(codes)])


def below(count):
    """count distinct values of code 0: -8.5 itself, below it, -1e300 and -inf."""
    v = np.concatenate(([-8.5, -1e300, -np.inf], -8.5 - 0.125 * np.arange(1, count - 2)))
    assert len(v) == count and (code_of(v) == 0).all()
    return v


def above(count):
    v = -below(count)
    v[0] = 8.5 + 1e-9  # 8.5 itself may take the code before the last
    assert (code_of(v) == 0xFFFFFFFF).all()
    return v


C0 = int(code_of(0.7)) & ~31
BIN_CASES = {
    "spread-32": (lambda: spread_bin(C0, 4, 8), CLEAN),
    "spread-33": (lambda: np.concatenate((spread_bin(C0, 4, 8), chain(x_of_code(C0 + 30), 1))), BIN_OVER),
    "onecode-32": (lambda: chain(x_of_code(C0 + 9), 32), CLEAN),
    "onecode-33": (lambda: chain(x_of_code(C0 + 9), 33), BIN_OVER),
    "ends-32": (lambda: np.concatenate((below(32), above(32))), CLEAN),
    "below-33": (lambda: np.concatenate((below(33), above(32))), BIN_OVER),
    "above-33": (lambda: np.concatenate((below(32), above(33))), BIN_OVER),
}


@pytest.mark.parametrize("name", sorted(BIN_CASES))
def test_bin_capacity(gpu, name):
    """n = 10 000: a bin (32 adjacent codes) of 32 distinct values, over eight codes or in one, is
    ranked by the finish; 33 flag the column (flags bit 0) and the general path gives the same
    positions.  Values beyond +-8.5 and +-inf take code 0 / 0xFFFFFFFF and are ordered by value."""
    make, expect = BIN_CASES[name]
    rng = seeded(23, name)
    vals = make()
    cs = plant(background(10_000, rng, [C0 >> 16]), rng, vals)
    codes = code_of(cs)
    assert largest_bin(codes) == (33 if expect == BIN_OVER else 32), "precondition: the fullest bin"
    assert largest_bin(codes[~np.isin(cs, vals)]) <= 2
    run_case(cs, expect, y_mode=name in ("onecode-32", "onecode-33"), first=0)


# ---------------------------------------------------------------------------- D
GROUPS = [2, 3, 4, 31, 32]
CD = int(code_of(-0.4)) & ~31


def tie_values(e, variant):
    """(the values to plant, the values that tie)."""
    if variant == "alone":
        x = x_of_code(CD + 11)
        return np.full(e, x), [x]
    if variant == "beside":  # distinct values of the same code below and above, while the bin holds <= 32
        lo = min(2, BIN_CAP - e)
        hi = min(2, BIN_CAP - e - lo)
        c = chain(x_of_code(CD + 11), lo + hi + 1)
        return np.concatenate((c[:lo], np.full(e, c[lo]), c[lo + 1:])), [c[lo]]
    b = CD >> 16  # the first and the last bin of one bucket
    lo, hi = x_of_code((b << 16) + 3), x_of_code((b << 16) + 65535 - 3)
    return np.concatenate((np.full(e, lo), np.full(e, hi))), [lo, hi]


def check_groups(col, tied):
    """Every member of the tie group of value v receives a + (e - 1) // 2, a = #{values < v}."""
    p = col.out.get()
    for v in tied:
        members = col.cs == v
        a, e = int((col.cs < v).sum()), int(members.sum())
        assert e >= 2 and (p[members] == a + (e - 1) // 2).all(), (v, a, e, p[members])


@pytest.mark.parametrize("variant", ["alone", "beside", "edges"])
@pytest.mark.parametrize("e", GROUPS)
def test_ties(gpu, e, variant):
    """n = 10 000: a group of e equal values inside one bin -- alone, beside distinct values of
    its code, in the first and in the last bin of one bucket."""
    rng = seeded(24, e, variant)
    vals, tied = tie_values(e, variant)
    cs = plant(background(10_000, rng, [CD >> 16]), rng, vals)
    assert largest_bin(code_of(cs)) == len(vals) // len(tied) <= BIN_CAP
    assert len(np.unique(cs)) == len(cs) - len(tied) * (e - 1)
    col = run_case(cs, CLEAN, distinct=False, first=0)[2]
    check_groups(col, tied)


def test_ties_zeros_and_ends(gpu):
    """-0.0 ties with +0.0; tie groups at sorted positions 0 (code 0) and n - 1 (the last code)
    and inside the column, all in one column; y-mode too."""
    rng = seeded(25)
    vals = np.concatenate(([0.0, -0.0, 0.0, -0.0, -0.0], np.full(3, -9.25), np.full(2, 9.5), np.full(4, 1.25)))
    cs = plant(background(10_000, rng, [bucket_at(0.0), bucket_at(1.25)]), rng, vals)
    n = len(cs)
    assert cs.min() == -9.25 and cs.max() == 9.5 and np.signbit(cs[cs == 0.0]).sum() == 3
    _, r, col = run_case(cs, CLEAN, distinct=False, y_mode=True, first=0)
    check_groups(col, [0.0, -9.25, 9.5, 1.25])
    assert (r[cs == -9.25] == 1).all() and (r[cs == 9.5] == n - 2).all()


# ---------------------------------------------------------------------------- E
def shuffled(x, key):
    return seeded(26, key).permutation(x)


def adapt_interval():
    """100 000 values evenly spaced in [0.3, 0.301]: ~4000 a bucket under the fixed map."""
    return shuffled(np.linspace(0.3, 0.301, 100_000), 1)


def adapt_one_bucket(b):
    """65 536 values inside the top-16 bucket b (about 4e-5 wide): one histogram block, whose packed
    16-bit counter of b is asked to hold 65536."""
    cs = shuffled(np.linspace(x_of_code((b << 16) + 100), x_of_code((b << 16) + 65400), 65536), 2)
    assert (code_of(cs) >> 16 == b).all() and cs.max() - cs.min() < 1e-4
    return cs


def adapt_peaks():
    """Fifty peaks of 3000 values, each 2e-5 wide, from -3 to 3, and three values beyond each end."""
    peaks = [c + np.linspace(0.0, 2e-5, 3000) for c in np.linspace(-3.0, 3.0, 50)]
    return shuffled(np.concatenate(peaks + [[-8.75, -9.5, -np.inf, 8.75, 9.5, np.inf]]), 3)


def adapt_segment_edge():
    """~70 000 values around an edge of the 4096-segment map, the edge and its two neighbours among them."""
    edge = ADAPT_X0 + 2200 * ADAPT_W
    assert (edge - ADAPT_X0) * (1.0 / ADAPT_W) == 2200.0
    x = np.linspace(edge - 5e-4, edge + 5e-4, 69_996)
    assert edge not in x
    return shuffled(np.concatenate((x, [np.nextafter(edge, -np.inf), edge, np.nextafter(edge, np.inf)])), 4)


def adapt_narrow():
    """The interval of adapt_interval with 40 consecutive doubles in its middle: one code, even
    under the adaptive map."""
    x = np.linspace(0.3, 0.301, 99_960)
    return shuffled(np.concatenate((x, chain(np.nextafter(x[50_000], np.inf), 40))), 5)


def adapt_outside(n_below, n_above):
    lo = -8.5 - 1e-3 * np.arange(1, n_below + 1)
    hi = 8.5 + 1e-3 * np.arange(1, n_above + 1)
    return shuffled(np.concatenate((lo, hi)), 6)


# name -> (column, verdict, the first count's state)
ADAPT_CASES = {
    "interval": (adapt_interval, RECODED, 2),
    "one_bucket_even": (lambda: adapt_one_bucket(bucket_at(0.3) & ~1), RECODED, 1),
    "one_bucket_odd": (lambda: adapt_one_bucket(bucket_at(0.3) | 1), RECODED, 1),
    "peaks": (adapt_peaks, RECODED, 2),
    "segment_edge": (adapt_segment_edge, RECODED, 2),
    "narrow": (adapt_narrow, BIN_OVER_RECODED, 2),
    # no value inside [-8.5, 8.5]: the segment total is 0, the codes stay 0 and 0xFFFFFFFF
    "outside": (lambda: adapt_outside(2500, 2500), (2, 4, 1, 1), 2),
    # one histogram block: 65535 items leave the counter of bucket 0 at its last value, 65536 wrap it
    "outside_65535": (lambda: adapt_outside(65535, 1), (2, 4, 1, 1), 2),
    "outside_65536": (lambda: adapt_outside(65536, 0), (1, 4, 1, 1), 1),
}


@pytest.mark.parametrize("name", sorted(ADAPT_CASES))
def test_adaptive_map(gpu, name):
    """Columns the fixed map rejects (asserted on the host: a bucket above 2048, or a counter asked
    to hold 65536), with the verdict after the re-code: flat (state 0, flags 0, redone 0), a bin
    above 32 (flags bit 0), or not flat again (the second count's state, flags bit 2)."""
    make, expect, first = ADAPT_CASES[name]
    run_case(make(), expect, y_mode=name in ("interval", "outside"), first=first)


@functools.lru_cache(maxsize=1)
def three_columns():
    n = 100_000
    rng = seeded(27)
    css = [rng.normal(size=n), adapt_interval(), rng.normal(size=n)]
    assert [predict(cs)[0] for cs in css] == [CLEAN, RECODED, CLEAN]
    return _ro(*css), [_ro(index_ref(cs)) for cs in css]


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)], ids=["forward", "reverse"])
def test_adaptive_map_leaves_the_neighbours_alone(gpu, order):
    """Three columns of one handle, on three lanes at once; only the middle one is re-coded.  Its
    reset clears its own slices of hist, cur1, cur2, curF and cls: the neighbours' positions are
    exact and their verdicts 0, in either launch order."""
    css, refs = three_columns()
    cols, L, _ = owned_run(list(css), order=order)
    assert [c.verdict for c in cols] == [CLEAN, RECODED, CLEAN]
    for c, r in zip(cols, refs):
        check_positions(c, r, True)
    assert L["k_hist16"] == 3 and L["k_finish"] == 3


# ---------------------------------------------------------------------------- F
def test_column_launched_twice_is_refused(gpu):
    """The second pbh_ic_owned_column for one i returns PBH_ERR_INVALID; the first launch's result
    stands and the device stays usable."""
    cs = seeded(28).normal(size=5000)
    cols, L, _ = owned_run([cs], twice=True)
    assert cols[0].verdict == CLEAN and L["k_finish"] == 1
    check_positions(cols[0], index_ref(cs), True)
    run_case(cs[:3000].copy(), CLEAN)


def test_workspace_reused_after_a_redone_column(gpu):
    """A handle whose column was rejected and redone, then a second handle in the same workspace:
    clean verdicts and exact positions (nothing of the first handle's state, flags or cursors
    survives the second's setup)."""
    bad = adapt_outside(2500, 2500)
    cols, _, ws = owned_run([bad])
    assert cols[0].verdict == (2, 4, 1, 1)
    check_positions(cols[0], index_ref(bad), True)
    cs = seeded(29).normal(size=5000)
    cols, _, _ = owned_run([cs], ws=ws)
    assert cols[0].verdict == CLEAN
    check_positions(cols[0], index_ref(cs), True)
