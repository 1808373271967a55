"""The row-sharded Iman-Conover phase calls, one C-ABI entry point per call, at their shard cuts.

    pbh_sorted_check        k_check_sorted: 4 pairs a thread across 256-thread seams, the grid-stride
                            step above 4096 x 1024 elements
    pbh_run_heads           k_heads_count / k_heads_write: the 4096-position tile, the running offset
                            over 16 rows of 256, the scan's second partial block above 2048 tiles,
                            first_is_prev and t0 up to 2^32 - 2
    pbh_sort_heads          k_sort_heads: the bitonic network padded to the next power of two
    pbh_lhs_sorted_ppf      every generator family of gen_sorted, whole and in segments
    pbh_lhs_sorted_counts   the counts and run heads of a segment (the boundary searches of the
                            discrete families, the scan of the others, the certificate), summed
                            over shards that overlap by one stratum (t0 = row0 - 1)
    pbh_lhs_scores          k_perm_scores / run_average_rank: the head table in LDS (<= 4096 heads)
                            or in global memory, the last run, row ranges
    pbh_lhs_values_at       the BYROW placement kernels: blocks of 4096 rows, a ragged last block,
                            a strided y
    pbh_ic_factor           corrcoef of a summed Gram matrix and its Cholesky factor (host)

The references are numpy / scipy on the host, or a call that another file pins (pbh_lhs_ppf:
test_gpu_ppf_kernels.py; pbh_ic_column_scores: test_gpu_sortrank.py), never another mode of the
call under test.  float64 buffers are strided views inside NaN-sentinel buffers (abi_views.py);
the u32 arrays, which take no stride, lie between sentinel words (Words below).  Every buffer is
read back whole.

Mutation check (each change built into a scratch library, this file run against it on an MI355X;
the number of tests that fail, of the 51 that run in this process, and which):
    is_head: p == 0 ? !first_is_prev -> true               2   run_heads_* (every first_is_prev call)
    k_heads_write: shift -> t0                             2   run_heads_* (first_is_prev with a head)
    k_check_sorted: in = t + 1 < n -> t + 2 < n            2   sorted_check_* (the last pair)
    k_check_sorted: !(a <= b) -> a > b                     2   sorted_check_* (the NaN inputs)
    run_average_rank: (e - s) / 2.0 -> integer division    1   lhs_scores_tied (runs of even length)
    run_average_rank: last run's end n -> n - 1            1   lhs_scores_tied (the last run)
    k_perm_scores: nheads - 1 entries staged in LDS        2   lhs_scores_tied, lhs_scores_row_ranges
    k_sort_heads: pad 0xFFFFFFFF -> 0                      1   sort_heads (nh no power of two)
    gen_sorted: t0 a head of every segment                 9   sorted_counts_segments_and_shards (6),
                                                               sorted_counts_heads_overflow (3)
"""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from abi_views import Flag, View
from conftest import assert_close

pytestmark = pytest.mark.gpu

SEED, COL = 20240611, 2
WSENT = 0xA55A5EED  # the sentinel word around (and, before a call, in) every u32 array
WPAD = 64


def _ro(a):
    a.setflags(write=False)
    return a


def lib():
    from probabilit_amd import _lib

    return _lib.load()


def stream():
    from probabilit_amd import device

    return device.stream()


class Words:
    """n u32 words between WPAD sentinel words on each side; the words start as `values`, or as
    sentinels too."""

    def __init__(self, n, values=None):
        import torch

        from probabilit_amd import device

        self.n = int(n)
        h = np.full(self.n + 2 * WPAD, WSENT, dtype=np.uint32)
        if values is not None:
            h[WPAD:WPAD + self.n] = np.asarray(values, dtype=np.uint32)
        self.buf = torch.from_numpy(h.view(np.int32)).to(device.device())
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + 4 * WPAD)

    def read(self):
        """(the n words, the padding around them) as host u32 arrays."""
        a = self.buf.cpu().numpy().view(np.uint32)
        return a[WPAD:WPAD + self.n], np.concatenate((a[:WPAD], a[WPAD + self.n:]))

    def words(self):
        w, pad = self.read()
        assert (pad == WSENT).all(), "a write next to a u32 array"
        return w


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------- 1. pbh_sorted_check
CHECK_N = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2049]
CHECK_BIG = 4096 * 1024 + 5  # the grid is capped at 4096 blocks of 1024 pairs: block 0 takes a second step


def check_inputs(n):
    """(label, x): the inputs of the issue that fit in n elements."""
    inc = np.arange(n) * 0.5 - 3.0
    out = [("increasing", inc), ("equal", np.full(n, 2.5)), ("runs", np.floor(np.arange(n) / 3.0))]
    for t in sorted({255, 256, 1023, 1024, n - 2}):
        if 0 <= t < n - 1:  # x[t] > x[t + 1], and still below x[t + 2]
            x = np.arange(n, dtype=np.float64)
            x[t] = x[t + 1] + 0.5
            out.append((f"inversion@{t}", x))
    if n >= 1:
        x = inc.copy()
        x[n // 2] = np.nan
        out.append(("nan", x))
    if n >= 2:
        x = np.arange(n) - n // 2 + 0.5
        x[n // 2 - 1], x[n // 2] = -0.0, 0.0
        assert n < 4 or (x[n // 2 - 2] < 0 < x[n // 2 + 1])
        out.append(("zeros", x))
        x = inc.copy()
        x[-2:] = np.inf
        if n >= 4:
            x[:2] = -np.inf
        out.append(("inf", x))
    return out


def check_ref(x):
    if len(x) < 2:
        return 0, 0
    return int((x[:-1] == x[1:]).sum()), int((~(x[:-1] <= x[1:])).sum())


def sorted_check(x, off):
    n = len(x)
    xv, ws = View(n, off, 1, x), View(32)
    ties, inv = ctypes.c_int64(-7), ctypes.c_int64(-7)
    st = lib().pbh_sorted_check(xv.ptr, n, ctypes.byref(ties), ctypes.byref(inv), ws.ptr, stream())
    assert st == 0
    assert xv.intact() and ws.intact(), "a write outside x or outside the 256 bytes of workspace"
    np.testing.assert_array_equal(xv.host(np.int64), bits(x), err_msg="x changed")
    return ties.value, inv.value


def test_sorted_check_against_numpy(gpu):
    """ties = #(x[t] == x[t + 1]), inversions = #!(x[t] <= x[t + 1]): a NaN is two inversions and
    no tie, -0.0 / +0.0 and inf / inf are ties."""
    cases = 0
    for n in CHECK_N:
        for label, x in check_inputs(n):
            for off in (0, 1):
                assert sorted_check(x, off) == check_ref(x), (n, label, off)
                cases += 1
    assert check_ref(np.array([1.0, np.nan, 2.0])) == (0, 2) and check_ref(np.array([-0.0, 0.0, np.inf, np.inf])) == (2, 0)
    print(f"sorted_check: {cases} sub-cases")


def test_sorted_check_second_grid_step(gpu):
    """n = 4096 x 1024 + 5 (34 MB): runs of three, a NaN in the middle, and an inversion in the
    last pair, which only the second grid-stride step of block 0 reads."""
    n = CHECK_BIG
    x = np.floor(np.arange(n) / 3.0)
    x[n // 2] = np.nan
    x[n - 2] = x[n - 1] + 1.0
    ref = check_ref(x)
    assert ref[1] == 3 and ref[0] > n // 2
    assert sorted_check(x, 1) == ref


# ---------------------------------------------------------------------------- 2. pbh_run_heads
HEADS_M = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 1]
HEADS_BIG = 2048 * 4096 + 4097  # 2050 tiles: the scan of the tile counts takes a second partial block


def from_heads(m, heads):
    """x[p] = the number of heads at or before p, less one: a sorted column with exactly these run heads."""
    h = np.zeros(m, dtype=bool)
    h[[p for p in heads if 0 < p < m]] = True
    return np.cumsum(h).astype(np.float64)


def heads_inputs(m):
    out = [("equal", np.full(m, 1.5)), ("distinct", np.arange(m) * 0.25),
           ("edges", from_heads(m, [255, 256, 4095, 4096, 4097])),
           ("empty_tile", from_heads(m, [4000, 8200, m - 1])),  # no head in [4096, 8192)
           ("pairs", np.floor(np.arange(m) / 2.0))]
    z = np.where(np.arange(m) % 2 == 0, -0.0, 0.0)  # -0.0 / +0.0 neighbours: one run
    z[m // 2:] = 1.0
    out.append(("zeros", z))
    return out


def heads_ref(x, t0, first_is_prev):
    m = len(x)
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    h = np.empty(m, dtype=bool)
    h[0] = not first_is_prev
    h[1:] = x[1:] != x[:-1]
    return (t0 - 1 if first_is_prev else t0) + np.flatnonzero(h)


def heads_workspace(m):
    import torch

    from probabilit_amd import device

    nb = ctypes.c_size_t()
    assert lib().pbh_run_heads_workspace_size(m, ctypes.byref(nb)) == 0
    ws = torch.full((nb.value + 256,), 0x5A, dtype=torch.uint8, device=device.device())
    return ws, nb.value


def run_heads(xv, m, t0, first_is_prev, ws, nbytes, short=0):
    hw = Words(m)  # at most m heads, whatever the call does
    count = ctypes.c_int64(-7)
    st = lib().pbh_run_heads(xv.ptr, m, t0, int(first_is_prev), hw.ptr, ctypes.byref(count), ws.data_ptr(),
                             nbytes - short, stream())
    w = hw.words()
    assert bool((ws[nbytes:] == 0x5A).all()), "a write past the workspace"
    return st, count.value, w


def run_heads_cases(m, inputs, t0s):
    from probabilit_amd import _lib

    ws, nbytes = heads_workspace(m)
    cases = 0
    for label, x in inputs:
        xv = View(m, 1, 1, x)
        for fip in (False, True):
            for t0 in t0s:
                ref = heads_ref(x, t0, fip)
                assert len(ref) == 0 or (0 <= ref[0] and ref[-1] < 2**32 - 1)
                st, count, w = run_heads(xv, m, t0, fip, ws, nbytes)
                what = (m, label, fip, t0)
                assert st == 0 and count == len(ref), (what, count, len(ref))
                np.testing.assert_array_equal(w[:count].astype(np.int64), ref, err_msg=str(what))
                assert (w[count:] == WSENT).all(), (what, "a word past count was written")
                cases += 1
        assert xv.intact()
        np.testing.assert_array_equal(xv.host(np.int64), bits(x), err_msg="x changed")
    st, count, w = run_heads(xv, m, 0, False, ws, nbytes, short=1)
    assert st == _lib.ERR_WORKSPACE and _lib.last_error(), m
    assert count == -7 and (w == WSENT).all(), "a workspace one byte short: nothing may be written"
    return cases


def test_run_heads_against_numpy(gpu):
    cases = 0
    for m in HEADS_M:
        cases += run_heads_cases(m, heads_inputs(m), (0, 1, 12345, 2**32 - 2 - m))
    print(f"run_heads: {cases} sub-cases")


def test_run_heads_second_scan_block(gpu):
    """m = 2048 x 4096 + 4097 (67 MB): heads every 1000 positions and on both sides of the tile that
    starts the second partial block of the scan; the reported strata end at 2^32 - 3."""
    m = HEADS_BIG
    h = list(range(1000, m, 1000)) + [2048 * 4096 - 1, 2048 * 4096, 2048 * 4096 + 1, m - 1]
    run_heads_cases(m, [("every1000", from_heads(m, h))], (2**32 - 2 - m,))


# ---------------------------------------------------------------------------- 3. pbh_sort_heads
def test_sort_heads_against_numpy(gpu):
    """nh on both sides of the powers of two the network is padded to; values up to 2^32 - 2, so a
    pad of 0xFFFFFFFF stays behind every one of them."""
    from probabilit_amd import _lib

    rng = np.random.default_rng(3)
    for nh in (0, 1, 2, 3, 1023, 1024, 1025, 4097, 16383, 16384):
        r = rng.integers(0, 2**32 - 1, size=nh, dtype=np.uint64).astype(np.uint32)
        if nh >= 3:
            r[rng.integers(0, nh, nh // 3)] = r[rng.integers(0, nh, nh // 3)]  # repeats
            r[0], r[1] = 2**32 - 2, 0
        for label, v in (("random", r), ("sorted", np.sort(r)), ("reversed", np.sort(r)[::-1])):
            hw = Words(nh, v)
            assert lib().pbh_sort_heads(hw.ptr, nh, stream()) == 0, (nh, label)
            np.testing.assert_array_equal(hw.words(), np.sort(v), err_msg=f"{nh} {label}")
    v = rng.integers(0, 2**32 - 1, size=16385, dtype=np.uint64).astype(np.uint32)
    hw = Words(16385, v)
    assert lib().pbh_sort_heads(hw.ptr, 16385, stream()) == _lib.ERR_INVALID and _lib.last_error()
    np.testing.assert_array_equal(hw.words(), v, err_msg="16385 heads: rejected, so unchanged")


# ---------------------------------------------------------------------------- generator families
# one column per family gen_create dispatches to (gen_sorted / place_launch / ext_gen_*): the
# per-wave tail kernels (norm, lognorm), the plain sweep (uniform, expon, triang), gamma with its
# guide table in LDS (a = 2) and a small shape (a = 0.1: most of the column in the slow tail), poisson
# with its CDF table in LDS (mu = 4) and in global memory (mu = 1e5: 10 000 entries > 3072), and the
# extended set: beta and truncnorm (tables), binom and bernoulli (discrete), weibull_min (closed form)
FAMILIES = [("norm", {"loc": 1.0, "scale": 2.0}), ("lognorm", {"s": 0.5, "scale": 2.0}),
            ("uniform", {"loc": -1.0, "scale": 3.0}), ("expon", {"scale": 2.5}),
            ("triang", {"c": 0.3, "loc": 1.0, "scale": 2.0}), ("gamma", {"a": 2.0}), ("gamma", {"a": 0.1}),
            ("poisson", {"mu": 4.0}), ("poisson", {"mu": 1e5}), ("beta", {"a": 2.0, "b": 3.0}),
            ("truncnorm", {"a": -1.0, "b": 2.0, "loc": 1.0, "scale": 1.0}), ("binom", {"n": 20, "p": 0.3}),
            ("bernoulli", {"p": 0.25}), ("weibull_min", {"c": 1.7})]
FAM_IDS = [f"{name}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for name, kw in FAMILIES]
CONTINUOUS = [i for i, (name, _) in enumerate(FAMILIES) if name not in ("poisson", "binom", "bernoulli")]
GAMMA = [i for i, (name, _) in enumerate(FAMILIES) if name == "gamma"]
SEG_N = [1, 2, 4097, 20011]


def params_of(fam):
    from probabilit_amd.modeling import _parse_scipy_args

    name, kw = fam
    p = [float(v) for v in _parse_scipy_args(name, (), kw)]
    return (ctypes.c_double * 4)(*(p + [0.0] * (4 - len(p)))), len(p)


def dist_id(fam):
    from probabilit_amd import _lib

    return _lib.DIST_IDS[fam[0]]


def sorted_ppf(fam, n, t0, nt):
    """pbh_lhs_sorted_ppf into a view of max(nt, 0) elements; (status, view, flag)."""
    prm, k = params_of(fam)
    out, flag = View(max(nt, 0), 1), Flag()
    st = lib().pbh_lhs_sorted_ppf(SEED, n, t0, nt, COL, dist_id(fam), prm, k, out.ptr, flag.ptr, stream())
    return st, out, flag.value()


@functools.lru_cache(maxsize=None)
def whole_column(f, n):
    """The sorted column of family f from one call, on the host."""
    st, out, flag = sorted_ppf(FAMILIES[f], n, 0, n)
    assert st == 0 and flag == 0 and out.intact(), (FAM_IDS[f], n)
    return _ro(out.host())


def partition(n):
    """The cuts of the issue inside (0, n), with 0 and n."""
    return [0] + sorted(c for c in {1, 255, 256, 257, 4096, n - 1} if 0 < c < n) + [n]


# ---------------------------------------------------------------------------- 4. pbh_lhs_sorted_ppf
@pytest.mark.parametrize("f", range(len(FAMILIES)), ids=FAM_IDS)
def test_sorted_ppf_whole_and_segments(gpu, f):
    """The whole column is np.sort of pbh_lhs_ppf's column bit for bit; every segment of a
    partition, and every shard segment that starts one stratum early, is a slice of it."""
    from probabilit_amd import _lib, native

    fam = FAMILIES[f]
    for n in SEG_N:
        whole = whole_column(f, n)
        rows = native.lhs_ppf(fam[0], SEED, n, COL, **fam[1])
        np.testing.assert_array_equal(bits(whole), bits(np.sort(rows)), err_msg=f"{FAM_IDS[f]} n={n}: not sort(lhs_ppf)")
        cuts = partition(n)
        segs = list(zip(cuts[:-1], cuts[1:])) + [(c - 1, n) for c in cuts[1:-1]] + [(c - 1, c + 1) for c in cuts[1:-1]]
        for a, b in segs:
            st, out, flag = sorted_ppf(fam, n, a, b - a)
            assert st == 0 and flag == 0 and out.intact(), (n, a, b)
            np.testing.assert_array_equal(out.host(np.int64), bits(whole[a:b]), err_msg=f"{FAM_IDS[f]} n={n} [{a}, {b})")
        for t0 in (0, n // 2, n):
            st, out, flag = sorted_ppf(fam, n, t0, 0)
            assert st == 0 and flag == 0 and out.untouched(), (n, t0, "nt = 0 writes nothing")
        for t0, nt in ((n, 1), (n - 1, 2), (0, n + 1)):
            prm, k = params_of(fam)
            out = View(nt, 1)
            st = lib().pbh_lhs_sorted_ppf(SEED, n, t0, nt, COL, dist_id(fam), prm, k, out.ptr, None, stream())
            assert st == _lib.ERR_INVALID and _lib.last_error(), (n, t0, nt)
            assert out.untouched(), (n, t0, nt)


# ---------------------------------------------------------------------------- 5. pbh_lhs_sorted_counts
# discrete columns: the boundary searches (k_discrete_heads, k_ext_discrete_heads); binom with a
# non-integer loc and the uniform column that ties take the stratum-by-stratum scan with heads
TIED_UNIFORM = ("uniform", {"loc": 2.0**44, "scale": 1.0})  # an ulp of 2^-8 spans 16 strata of n = 4099
COUNT_COLUMNS = [(("poisson", {"mu": 4.0}), 20011), (("binom", {"n": 20, "p": 0.3}), 20011),
                 (("bernoulli", {"p": 0.25}), 20011), (("poisson", {"mu": 4.0}), 4097),
                 (("binom", {"n": 12, "p": 0.6, "loc": 0.5}), 4097), (TIED_UNIFORM, 4099)]
HCAP = 16384


@functools.lru_cache(maxsize=None)
def count_column(i):
    fam, n = COUNT_COLUMNS[i]
    st, out, flag = sorted_ppf(fam, n, 0, n)
    assert st == 0 and flag == 0 and out.intact()
    return _ro(out.host())


def sorted_counts(fam, n, t0, nt, hcap=0, certify=0):
    """(counts, the heads array, hcur, flag); the heads array is None without heads."""
    prm, k = params_of(fam)
    counts, flag = View(2), Flag()
    hw, hc = (Words(hcap), Words(1, [WSENT])) if hcap else (None, None)
    st = lib().pbh_lhs_sorted_counts(SEED, n, t0, nt, COL, dist_id(fam), prm, k, counts.ptr, hw.ptr if hcap else None,
                                     hc.ptr if hcap else None, hcap, flag.ptr, certify, stream())
    assert st == 0, (fam, n, t0, nt)
    assert counts.intact()
    return counts.host(np.int64).tolist(), hw.words() if hcap else None, int(hc.words()[0]) if hcap else None, flag.value()


def segment_ref(x, t0, nt):
    """(ties, inversions) over the pairs inside [t0, t0 + nt) and the run heads in (t0, t0 + nt),
    plus 0 when t0 == 0."""
    xs = x[t0:t0 + nt]
    t = np.arange(t0 + 1, t0 + nt)
    heads = set(t[x[t] != x[t - 1]].tolist()) | ({0} if t0 == 0 else set())
    return [check_ref(xs)[0], check_ref(xs)[1]], heads


def checked_segment(i, t0, nt, cache):
    """One segment against numpy; (counts, heads written) for the sums over shards."""
    if (t0, nt) not in cache:
        fam, n = COUNT_COLUMNS[i]
        counts, w, hcur, flag = sorted_counts(fam, n, t0, nt, HCAP)
        ref_counts, ref_heads = segment_ref(count_column(i), t0, nt)
        what = (fam, n, t0, nt)
        assert flag == 0, what
        assert counts == ref_counts, (what, counts, ref_counts)
        assert hcur == len(ref_heads), (what, hcur, len(ref_heads))
        assert sorted(w[:hcur].tolist()) == sorted(ref_heads), what
        assert (w[hcur:] == WSENT).all(), what
        cache[(t0, nt)] = (counts, w[:hcur].tolist())
    return cache[(t0, nt)]


def change_cuts(x):
    """Cuts at the first, a middle and the last change of value, one stratum before and one after."""
    n = len(x)
    ch = np.flatnonzero(x[1:] != x[:-1]) + 1
    pick = sorted({int(ch[0]), int(ch[len(ch) // 2]), int(ch[-1])})
    return sorted(c for c in {p + d for p in pick for d in (-1, 0, 1)} | {1, 256, 4096, n - 1} if 0 < c < n)


@pytest.mark.parametrize("i", range(len(COUNT_COLUMNS)), ids=[f"{f[0]}-{n}" for f, n in COUNT_COLUMNS])
def test_sorted_counts_segments_and_shards(gpu, i):
    """Every segment against numpy on the materialised column; shards that start at t0 = row0 - 1
    add up to the whole column (the pair across a cut counted once, no head twice) for cuts at a
    change of value, one stratum before and one after it.  A cut at row 1 is the one exception the
    header records: that shard's t0 is 0 too, so both shards report stratum 0 (a second 0 at the
    front of the sorted list leaves every rank as it is: test_lhs_scores_tied)."""
    fam, n = COUNT_COLUMNS[i]
    x = count_column(i)
    cache = {}
    whole_counts, whole_heads = checked_segment(i, 0, n, cache)
    assert whole_counts[1] == 0 and len(whole_heads) >= 2
    cuts = partition(n)
    for a, b in list(zip(cuts[:-1], cuts[1:])) + [(0, 0), (n // 2, n // 2), (n - 1, n)]:
        checked_segment(i, a, b - a, cache)
    cc = change_cuts(x)
    splits = [(c,) for c in cc] + list(zip(cc[:-1], cc[1:])) + [(cc[0], cc[-1])]
    for split in splits:
        rows = [0, *split, n]
        parts = [checked_segment(i, max(a - 1, 0), b - max(a - 1, 0), cache) for a, b in zip(rows[:-1], rows[1:])]
        assert [sum(p[0][j] for p in parts) for j in (0, 1)] == whole_counts, (fam, split)
        heads = [h for p in parts for h in p[1]]
        if split[0] == 1:  # the shard of row0 = 1 passes t0 = 0 as well: stratum 0 from both, and nothing else
            assert sorted(heads) == sorted(whole_heads + [0]), (fam, split)
        else:
            assert len(heads) == len(set(heads)), (fam, split, "a head appears twice")
            assert sorted(heads) == sorted(whole_heads), (fam, split)
    print(f"sorted_counts {fam[0]}: {len(cache)} segments, {len(splits)} partitions")


@pytest.mark.parametrize("i", [0, 1, 5], ids=["poisson", "binom", "uniform_ties"])
def test_sorted_counts_heads_overflow(gpu, i):
    """hcap below the number of heads: hcap distinct heads of the column are written, the words
    past hcap keep the sentinel, *hcur counts all heads."""
    fam, n = COUNT_COLUMNS[i]
    x = count_column(i)
    for t0, nt in ((0, n), (n // 3 - 1, n - n // 3 + 1)):
        ref_counts, ref_heads = segment_ref(x, t0, nt)
        assert len(ref_heads) > 3
        for hcap in (1, 3):
            hw, hc = Words(hcap + 32), Words(1)
            prm, k = params_of(fam)
            counts, flag = View(2), Flag()
            st = lib().pbh_lhs_sorted_counts(SEED, n, t0, nt, COL, dist_id(fam), prm, k, counts.ptr, hw.ptr, hc.ptr, hcap,
                                             flag.ptr, 0, stream())
            w = hw.words()
            assert st == 0 and flag.value() == 0
            assert counts.host(np.int64).tolist() == ref_counts
            assert int(hc.words()[0]) == len(ref_heads)
            assert (w[hcap:] == WSENT).all(), "a head past hcap"
            assert len(set(w[:hcap].tolist())) == hcap and set(w[:hcap].tolist()) <= ref_heads


def test_sorted_counts_continuous_and_certificate(gpu):
    """Continuous columns: the exact counts equal numpy's on the materialised column; the
    certificate's counts are non-zero whenever numpy's are, and [0, 0] only when numpy's are."""
    tied = count_column(5)
    assert check_ref(tied)[0] > 0
    for fam, n, x in [(TIED_UNIFORM, 4099, tied)] + [(FAMILIES[f], n, whole_column(f, n)) for f in CONTINUOUS
                                                      for n in (4097, 20011)]:
        for t0, nt in ((0, n), (255, n - 255), (4095, 2), (n - 1, 1), (7, 0)):
            ref = segment_ref(x, t0, nt)[0]
            exact, _, _, flag = sorted_counts(fam, n, t0, nt)
            assert exact == ref and flag == 0, (fam, n, t0, nt, exact, ref)
            cert, _, _, flag = sorted_counts(fam, n, t0, nt, certify=1)
            assert flag == 0
            if ref != [0, 0]:
                assert cert != [0, 0], (fam, n, t0, nt, "a tie or inversion was certified away")
            if cert == [0, 0]:
                assert ref == [0, 0], (fam, n, t0, nt)


# ---------------------------------------------------------------------------- 6. pbh_lhs_scores
@functools.lru_cache(maxsize=None)
def strata(n):
    """t[r] = rankdata(q, 'ordinal') - 1 of column COL of pbh_fill_lhs."""
    import scipy.stats

    from probabilit_amd import native

    q = np.ascontiguousarray(native.fill_lhs(SEED, n, COL + 1)[:, COL])
    assert len(np.unique(q)) == n, "the quantiles tie: choose another seed"
    return _ro(scipy.stats.rankdata(q, method="ordinal").astype(np.int64) - 1)


def lhs_scores(n, row0, nrows, H=None):
    out = View(nrows, 1)
    hw = Words(len(H), H) if H is not None else None
    st = lib().pbh_lhs_scores(SEED, n, COL, row0, nrows, hw.ptr if hw else None, len(H) if hw else 0, out.ptr, stream())
    assert st == 0, (n, row0, nrows)
    if hw:
        np.testing.assert_array_equal(hw.words(), H, err_msg="the heads changed")
    return out


def tied_ranks(H, n, t):
    """scipy's 'average' rank of stratum t, from the run heads."""
    H = np.asarray(H, dtype=np.int64)
    run = np.searchsorted(H, t, side="right") - 1
    s = H[run]
    e = np.concatenate((H[1:], [n]))[run] - 1
    return s + 1 + (e - s) / 2, run


def head_lists(n, rng):
    """len(H) on both sides of the 4096 heads staged in LDS; last runs of one stratum and long."""
    out = {}
    for k in (1, 2, 4095, 4096, 4097):
        out[f"{k}"] = np.concatenate(([0], np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False))))
    for k in (2, 4096, 4097):
        body = np.sort(rng.choice(np.arange(1, n - 5000), size=k - 2, replace=False))
        out[f"{k}-last1"] = np.concatenate(([0], body, [n - 1]))
        out[f"{k}-lastlong"] = np.concatenate(([0], body, [n - 5000]))
    return out


def test_lhs_scores_untied(gpu):
    import scipy.special

    for n in (1, 2, 513, 20011):
        t = strata(n)
        out = lhs_scores(n, 0, n)
        assert out.intact()
        assert_close(out.host(), scipy.special.ndtri((t + 1) / (n + 1)), rtol=1e-10, what=f"untied n={n}")


def test_lhs_scores_tied(gpu):
    """The run average of an arbitrary head list against scipy's ndtri within 1e-10, and bit for
    bit against pbh_ic_column_scores of x[r] = the run of row r (same rank formula, same ppnd16)."""
    import scipy.special
    import scipy.stats

    from probabilit_amd import device
    from probabilit_amd.distributed import HipPhases

    n = 20011
    t = strata(n)
    for label, H in head_lists(n, np.random.default_rng(6)).items():
        assert H[0] == 0 and (np.diff(H) > 0).all() and H[-1] < n
        ranks, run = tied_ranks(H, n, t)
        x = run.astype(np.float64)
        np.testing.assert_array_equal(ranks, scipy.stats.rankdata(x), err_msg="the reference ranks are not scipy's")
        out = lhs_scores(n, 0, n, H)
        assert out.intact(), label
        assert_close(out.host(), scipy.special.ndtri(ranks / (n + 1)), rtol=1e-10, what=f"tied {label}")
        pinned, sx, flag = device.empty(n), device.empty(n), device.zeros(1, "int32")
        HipPhases().column_scores(device.to_device(x), pinned, sx, flag)
        np.testing.assert_array_equal(out.host(np.int64), bits(device.to_host(pinned)),
                                      err_msg=f"tied {label}: not the bits of pbh_ic_column_scores")
        if label in ("1", "4095", "4096"):  # stratum 0 reported by two shards (row0 = 1): an empty run
            twice = lhs_scores(n, 0, n, np.concatenate(([0], H)))
            np.testing.assert_array_equal(twice.host(np.int64), out.host(np.int64), err_msg=f"tied {label}: 0 twice")


def test_lhs_scores_row_ranges(gpu):
    """Rows [row0, row0 + nrows) are the same rows of the whole call bit for bit, untied and with
    heads in LDS and in global memory; nothing is written outside the range."""
    for n in (1, 2, 513, 20011):
        lists = [None, np.arange(0, n, 3)]  # 6671 heads at n = 20011: global memory
        if n == 20011:
            lists.append(np.concatenate(([0], np.arange(5, n - 1, 5), [n - 1])))  # 4003: LDS
        for H in lists:
            whole = lhs_scores(n, 0, n, H).host(np.int64)
            for row0, nrows in ((0, n), (0, 1), (1, 511), (512, 1), (511, 2), (n - 1, 1), (min(7, n), 0)):
                if row0 + nrows > n:
                    continue
                out = lhs_scores(n, row0, nrows, H)
                what = (n, row0, nrows, None if H is None else len(H))
                assert out.intact(), what
                np.testing.assert_array_equal(out.host(np.int64), whole[row0:row0 + nrows], err_msg=str(what))


# ---------------------------------------------------------------------------- 7. pbh_lhs_values_at
VALUES_M = [0, 1, 255, 4095, 4096, 4097, 8193]
VALUES_N = [4097, 20011]


def index_patterns(n, m):
    rng = np.random.default_rng([7, n, m])
    return {"permutation": np.resize(rng.permutation(n), m), "reversed": (n - 1 - np.arange(m)) % n,
            "zeros": np.zeros(m, dtype=np.int64), "last": np.full(m, n - 1), "repeats": rng.integers(0, n, m)}


def values_at(fam, n, p, y_rs):
    from probabilit_amd import _lib

    prm, k = params_of(fam)
    col = _lib.ICColumn(SEED, COL, dist_id(fam), prm, k, None)
    m = len(p)
    pw, y = Words(m, p), View(m, 1, y_rs)
    st = lib().pbh_lhs_values_at(ctypes.byref(col), n, pw.ptr, m, y.ptr, y_rs, stream())
    assert st == 0, (fam, n, m, y_rs)
    assert y.intact(), (fam, n, m, y_rs, "a write outside y")
    np.testing.assert_array_equal(pw.words(), p, err_msg="p changed")
    return y.host(np.int64)


def values_at_outputs(f):
    """key -> the bits of y for every (n, m, pattern, y_rs) of family f."""
    out = {}
    for n in VALUES_N:
        for m in VALUES_M:
            for label, p in index_patterns(n, m).items():
                for y_rs in (1, 3):
                    out[f"{n}_{m}_{label}_{y_rs}"] = values_at(FAMILIES[f], n, p, y_rs)
    return out


def check_values_at(f, outputs):
    for n in VALUES_N:
        whole = bits(whole_column(f, n))
        for m in VALUES_M:
            for label, p in index_patterns(n, m).items():
                for y_rs in (1, 3):
                    key = f"{n}_{m}_{label}_{y_rs}"
                    np.testing.assert_array_equal(outputs[key], whole[p], err_msg=f"{FAM_IDS[f]} {key}")


@pytest.mark.parametrize("f", range(len(FAMILIES)), ids=FAM_IDS)
def test_values_at(gpu, f):
    """y[i * y_rs] == sorted_whole[p[i]] bit for bit: one block, a ragged block, two blocks and one row."""
    check_values_at(f, values_at_outputs(f))


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_phase_kernels as t
for f in t.GAMMA:
    np.savez({path!r} + str(f) + ".npz", **t.values_at_outputs(f))
"""


def test_values_at_gamma_lds_kernel_in_a_fresh_process(gpu, tmp_path):
    """PBH_GAMMA_WIN=0 (read once per process) sends the gamma columns to k_place_gen_gamma instead
    of the window kernels: the same values, against this process's sorted column."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "gamma")
    script = _CHILD.format(root=root, tests=os.path.join(root, "tests"), path=path)
    r = subprocess.run([sys.executable, "-c", script], env={**os.environ, "PBH_GAMMA_WIN": "0"}, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for f in GAMMA:
        with np.load(path + str(f) + ".npz") as there:
            check_values_at(f, there)


# ---------------------------------------------------------------------------- 8. pbh_ic_factor
U = 2.0**-53  # unit roundoff
NOT_PD = ("Rank data correlation not positive definite.There are perfect correlations in the ranked data."
          "Supply more data (rows in X) or sample differently.")
HPAD = 16


def ic_factor(G, n):
    """pbh_ic_factor on host buffers with NaN padding around the two outputs; (status, corr, L)."""
    k = G.shape[0]
    g = np.ascontiguousarray(G, dtype=np.float64)
    g0 = g.copy()
    bufs = [np.full(k * k + 2 * HPAD, np.nan) for _ in range(2)]
    ptr = [b.ctypes.data + 8 * HPAD for b in bufs]
    st = lib().pbh_ic_factor(g.ctypes.data, n, k, ptr[0], ptr[1])
    np.testing.assert_array_equal(g, g0, err_msg="the Gram matrix changed")
    for b in bufs:
        assert np.isnan(b[:HPAD]).all() and np.isnan(b[-HPAD:]).all(), "a write next to an output"
    return st, bufs[0][HPAD:-HPAD].reshape(k, k), bufs[1][HPAD:-HPAD].reshape(k, k)


def cholesky_longdouble(A):
    A = A.astype(np.longdouble)
    k = A.shape[0]
    Lm = np.zeros((k, k), dtype=np.longdouble)
    for j in range(k):
        d = np.sqrt(A[j, j] - Lm[j, :j] @ Lm[j, :j])
        Lm[j, j] = d
        Lm[j + 1:, j] = (A[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / d
    return Lm


def inverse_lower_longdouble(Lm):
    k = Lm.shape[0]
    X = np.zeros((k, k), dtype=np.longdouble)
    for j in range(k):  # forward substitution, one row at a time
        rhs = -(Lm[j, :j] @ X[:j, :])
        rhs[j] += 1.0
        X[j, :] = rhs / Lm[j, j]
    return X


@pytest.mark.parametrize("k", [1, 2, 33, 128])
def test_ic_factor_against_numpy(gpu, k):
    """corr: np.corrcoef's recipe in longdouble.  An entry is fl(fl(fl(G f) / sd_i) / sd_j) with
    f = fl(1 / (n - 1)) and sd = fl(sqrt(fl(G_ii f))): G f carries 2 roundings (f's and its own);
    each sd carries half of the 2 under its root plus its own, 2 in all; the two divisions add
    their operand's 2 and 1 of their own each: 2 + 3 + 3 = 8 roundings of relative size U = 2^-53,
    that is 4 ulp at most.  The clip to [-1, 1] moves both sides towards each other.
    L: against np.linalg.cholesky(corr).  Either factorisation of A = corr is the exact factor of
    A + dA with |dA| <= g |L||L^T|, g = (k + 1) U / (1 - (k + 1) U) (Higham, Accuracy and Stability,
    theorem 10.3), so ||dA||_F <= g ||L||_F^2 = g trace(A) = g k; to first order the factor moves by
    ||dL||_F <= kappa_2(A) ||dA||_F ||L||_2 / (sqrt(2) ||A||_2) (Sun's bound for the Cholesky factor),
    ||L||_2^2 = ||A||_2 >= 1 for a unit diagonal.  Two factorisations, and a factor 2 for the
    terms beyond first order: ||L - L_numpy||_F <= 4 kappa g k / sqrt(2), with kappa from the
    Frobenius norms of A and its inverse in longdouble (>= kappa_2).  The residual L L^T - A is held
    to the backward bound g |L||L^T| itself, entry by entry."""
    from probabilit_amd import _lib

    n = 1000
    rng = np.random.default_rng(k)
    S = rng.normal(size=(n, k)) @ (np.eye(k) + 0.3 * rng.normal(size=(k, k)) / np.sqrt(k))
    Sc = S - S.mean(axis=0)
    G = Sc.T @ Sc
    st, corr, Lg = ic_factor(G, n)
    assert st == 0, _lib.last_error()
    Gl = G.astype(np.longdouble)
    sd = np.sqrt(np.diag(Gl) / (n - 1))
    ref = np.clip(Gl / (n - 1) / sd[:, None] / sd[None, :], -1.0, 1.0)
    err = np.abs(corr.astype(np.longdouble) - ref)
    print(f"k={k}: corr max error {float((err / np.abs(ref)).max() / U):.2f} U")
    slack = 8.0 * float(np.finfo(np.longdouble).eps)  # the reference's own roundings
    assert (err <= (8.0 * U * (1.0 + 8.0 * U) + slack) * np.abs(ref)).all(), float((err / np.abs(ref)).max() / U)
    assert np.abs(np.diag(corr) - 1.0).max() <= 8.0 * U and np.abs(corr).max() <= 1.0

    assert (Lg[np.triu_indices(k, 1)] == 0.0).all(), "L is not lower triangular"
    Ll = cholesky_longdouble(corr)
    Ainv = inverse_lower_longdouble(Ll)
    Ainv = Ainv.T @ Ainv
    kappa = float(np.sqrt((corr.astype(np.longdouble)**2).sum()) * np.sqrt((Ainv**2).sum()))
    g = (k + 1) * U / (1.0 - (k + 1) * U)
    bound = 4.0 * kappa * g * k / np.sqrt(2.0)
    diff = float(np.sqrt(((Lg - np.linalg.cholesky(corr))**2).sum()))
    print(f"k={k}: kappa {kappa:.3g}, ||L - L_numpy||_F {diff:.3g}, bound {bound:.3g}")
    assert diff <= bound
    Lq = Lg.astype(np.longdouble)
    resid = np.abs(Lq @ Lq.T - corr.astype(np.longdouble))
    assert (resid <= g * (np.abs(Lq) @ np.abs(Lq).T)).all(), float(resid.max())


def test_ic_factor_not_positive_definite(gpu):
    """Two identical columns: n - 1 = 1024 and squares of 2 and 3 on the diagonal keep every
    rounding exact, so corr[0, 1] is exactly 1, the second pivot exactly 0, and the call fails
    with the reference's message; corr is still handed out."""
    from probabilit_amd import _lib

    G = 1024.0 * np.array([[4.0, 4.0, 3.0], [4.0, 4.0, 3.0], [3.0, 3.0, 9.0]])
    st, corr, _ = ic_factor(G, 1025)
    assert st == _lib.ERR_NOT_PD
    assert _lib.last_error() == NOT_PD
    np.testing.assert_array_equal(corr, [[1.0, 1.0, 0.5], [1.0, 1.0, 0.5], [0.5, 0.5, 1.0]])
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(corr)
