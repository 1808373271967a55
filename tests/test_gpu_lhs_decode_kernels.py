"""The device decode of the reference LHS shuffles (csrc/pbh_lhs_dev.hip) at the C ABI, at its own
boundaries: pbh_lhs_reference_strata called directly, q written into an abi_views.Block
(ldq = n + 3) and the strata into a Block32 (lds = n + 3), both inside sentinel buffers whose gap
rows, trailing column and padding must stay clean after every call, on the device path and on the
host path alike.

The reference is numpy itself: a Generator(PCG64()) set to the case's state, increment and
buffered half, u = g.uniform(size=(n, d)), d calls of g.shuffle on arange(1, n + 1),
q = (perms.T - u) / n and strata = perms.T - 1, compared bit for bit.

The decode checks itself and falls back to the host shuffles, so most defects in it never give a
wrong matrix: they only lose the device path.  Every case here therefore also reads
pbh_lhs_reference_stats and, unless it says otherwise, asserts device == 1 and attempts == 1.
Preconditions that make a case reach its edge (a column's draw count, the parity of a column's
first draw, tcap / 4096) are asserted from tests/lhs_mirror.py (pinned to numpy in
test_lhs_band_host.py) and pbh_lhs_reference_band_table before the call.

Mutations of pbh_lhs_dev.hip on a scratch copy, against this file (with test_lhs_band_host.py) and
against the decode tests the suite had (test_gpu_streams.py -k reference_lhs), 70 and 18 tests.
Four mutants were judged by reading and not run: they hang or read out of bounds by construction.

   mutation                                         this file                        old tests
 1 k_perm_links: M[t] = st, no st != t exception    not run: M[t] = t makes          not run
                                                    perm_value's chase endless; every
                                                    size with a self-targeting group
                                                    head, test_top_step_targets_itself
                                                    by construction
 2 column_to_q: bits / 8 passes                     47 fail (n < 128 is refused, 258 <  14 of 18 fail
                                                    n: wrong matrix); survives at n in
                                                    {255 .. 258, 65535 .. 65538, 2^24,
                                                    2^24 + 1} [a]
 3 q + c * n, strata + c * n at the call site       62 fail (all with d > 1)         pass (ldq = n)
 4 k_dec_classify: halves swapped                   65 fail with a wrong matrix and  16 of 18 fail
                                                    device == 1: the check re-reads
                                                    the same words, so it agrees
 5 k_dec_finish: P[c + 1] = p0 + tau0 + j           51 fail, wrong matrix likewise   15 of 18 fail
 6 k_scan_small: per = m / 1024                     not run: below 1024 blocks (all   not run
                                                    cases but three) no prefix is
                                                    written and dec[] is read at what
                                                    the buffer held; at 1025 and 2049
                                                    blocks the last block's prefix is
                                                    missing; right only at 1024
 7 k_dec_compact: no clamp of x                     survives [b]                     pass
 8 host walk: S <= N1 in the flagged branch         survives [c]                     pass
 9 Pinned::ensure returns early when cap > 0        not run: the copy of 2 488 114   not run
                                                    entries into 65536 overruns the
                                                    pinned buffer in test_staging_reuse
                                                    (fourth call), test_everything_
                                                    ambiguous[1000] and _under_the_cap
10 band_table: lo = (m + 1) / 2 + 1                 not run: hi = lo - 1 = 2^k keeps  --
                                                    its mask, band_table never returns;
                                                    test_lhs_band_host.py stops at its
                                                    first table, with no GPU
11 draw_band: no + 2.0                              3 fail: the ambiguous count falls pass
                                                    below the count draw_band restated
                                                    on the host gives (_under_the_cap,
                                                    test_staging_reuse)

[a] equivalent at those sizes: the sort runs the same passes at bits = 8, 16, 24, and at
    n = 2^k + 1 or + 2 the digit the dropped pass would sort is set in the keys of at most two
    steps, each of which almost never targets that high (1 / n); a lone key wherever it lands is
    still a group of one, which is all k_perm_links reads.  test_top_step_targets_itself puts one
    such key there on purpose and is, for that reason, still equivalent; two would take a search
    over 2^-25 events.
[b] equivalent below n ~ 2^30: a negative x stored as uint32 has bit 31 set, so the walk reads it
    as {A | 2^31, 0} with A = 2^31 + x >= n - 1 and rejects, as extra < 0 does.
[c] equivalent: the changed decision is the one at S = n - 1, after the column's last step;
    k_dec_finish looks at no draw with S >= n - 1 and the one accept too many only raises
    prefixes that are already past the end.
"""

import ctypes

import numpy as np
import pytest

import lhs_mirror as lm
from abi_views import Block, Block32

pytestmark = pytest.mark.gpu

BLK = 4096  # draws per block of the decode (kBlk)
CAP = 1 << 22  # ambiguous draws a column may hand to the host walk


# ---------------------------------------------------------------- helpers
def _state(tag, has32):
    """(state, inc, has32, buf32) of a case; buf32 is set even when has32 = 0 (it must be ignored)."""
    rng = np.random.default_rng(tag)
    state = int(rng.integers(0, 2**63)) << 64 | int(rng.integers(0, 2**63))
    inc = (int(rng.integers(0, 2**62)) << 1) | 1
    return state, inc, int(has32), int(rng.integers(1, 2**32))


def _seed_state(seed):
    st = np.random.default_rng(seed).bit_generator.state
    return st["state"]["state"], st["state"]["inc"], 0, 0


def _numpy_lhs(case, n, d):
    """(q, strata), both (n, d), from numpy's own uniform and shuffle."""
    g = lm.generator(*case)
    u = g.uniform(size=(n, d))
    perms = np.empty((d, n), dtype=np.int64)
    for c in range(d):
        x = np.arange(1, n + 1)
        g.shuffle(x)
        perms[c] = x
    return (perms.T - u) / n, perms.T - 1


def _mirror_columns(case, n, d):
    """The d columns' (start, end, steps, targets) in draws from the first shuffle draw."""
    g = lm.generator(*case)
    g.uniform(size=(n, d))
    return lm.columns(g, n, d)


def _stats():
    from probabilit_amd import _lib

    dev, att, amb = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    _lib.check(_lib.load().pbh_lhs_reference_stats(ctypes.byref(dev), ctypes.byref(att), ctypes.byref(amb)))
    return dev.value, att.value, amb.value


def _workspace(n, d):
    from probabilit_amd import _lib, device

    need = ctypes.c_size_t()
    _lib.check(_lib.load().pbh_lhs_reference_workspace_size(n, d, ctypes.byref(need)))
    return device.empty(int(need.value), "uint8")


def _call(case, n, d, ws=None, q=None, t=None):
    """(status, q block, strata block) of one pbh_lhs_reference_strata call on the current stream."""
    from probabilit_amd import _lib, device
    from probabilit_amd.qmc import _u128_words

    state, inc, has32, buf32 = case
    ws = _workspace(n, d) if ws is None else ws
    q = Block(n, d) if q is None else q
    t = Block32(n, d) if t is None else t
    s, i = _u128_words(state), _u128_words(inc)
    st = _lib.load().pbh_lhs_reference_strata(_lib.np_ptr(s), _lib.np_ptr(i), has32, buf32, n, d, q.ptr, q.ld, t.ptr,
                                              t.ld, ws.data_ptr(), ws.numel(), device.stream())
    return st, q, t


def _check(case, n, d, ws=None, ref=None, what=""):
    """One call compared with numpy, gaps included; returns the call's (device, attempts, ambiguous)."""
    from probabilit_amd import _lib

    st, q, t = _call(case, n, d, ws)
    assert st == 0, _lib.last_error()
    stats = _stats()
    rq, rt = _numpy_lhs(case, n, d) if ref is None else ref
    what = f"{what} n={n} d={d} has32={case[2]} stats={stats}"
    q.assert_bits(rq, "q " + what)
    t.assert_equal(rt, "strata " + what)
    return stats


class _band:
    """pbh_lhs_reference_band(width) for a block, restored on the way out."""

    def __init__(self, width):
        self.width = width

    def __enter__(self):
        from probabilit_amd import _lib

        self.prev = ctypes.c_double()
        _lib.check(_lib.load().pbh_lhs_reference_band(self.width, ctypes.byref(self.prev)))

    def __exit__(self, *exc):
        from probabilit_amd import _lib

        _lib.check(_lib.load().pbh_lhs_reference_band(self.prev.value, None))


def _tcap(n, sigmas=6.0):
    from probabilit_amd import _lib

    nband, tcap = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().pbh_lhs_reference_band_table(n, sigmas, None, 0, ctypes.byref(nband), ctypes.byref(tcap)))
    return tcap.value


# ---------------------------------------------------------------- sizes
SWEEP = [2, 3, 4, 5, 8, 9, 16, 17, 255, 256, 257, 258, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 65538]


@pytest.mark.parametrize("has32", [0, 1])
@pytest.mark.parametrize("n", SWEEP)
def test_size_sweep(gpu, n, has32):
    """n - 1 at 2^k - 1, 2^k and 2^k + 1: the mask boundaries of the first steps, the radix sort's
    passes 1 -> 2 (targets < 2^8) and 2 -> 3 (< 2^16), and rows at the 4096 boundary."""
    assert _check(_state(n, has32), n, 3)[:2] == (1, 1)


@pytest.mark.parametrize("n,has32", [(2**24, 0), (2**24 + 1, 1)])
def test_sort_passes_three_to_four(gpu, n, has32):
    """Targets below 2^24 sort in 3 passes; n = 2^24 + 1 has the target 2^24 and needs the fourth."""
    assert _check(_state(n, has32), n, 1)[:2] == (1, 1)


@pytest.mark.parametrize("n", [2, 257, 65537])
def test_top_step_targets_itself(gpu, n):
    """The buffered half is the first shuffle draw: with buf32 = n - 1 step n - 1 takes it and
    targets itself, the one key with bit log2(n - 1) set (the last sort pass has a single key in
    its upper digits) and a group whose first step is its own target (k_perm_links' st != t)."""
    state, inc, _, _ = _state(300 + n, 1)
    case = (state, inc, 1, n - 1)
    assert _mirror_columns(case, n, 1)[0][3][n - 1] == n - 1
    assert _check(case, n, 2)[:2] == (1, 1)


def test_single_row(gpu):
    """n = 1: no shuffle steps (k_single_row with ldq = 4, the strata's 4-byte memsets)."""
    case = _state(1, 1)
    st, q, t = _call(case, 1, 5)
    assert st == 0 and q.ld == 4 and t.ld == 4
    rq, rt = _numpy_lhs(case, 1, 5)
    assert np.all(rt == 0)
    q.assert_bits(rq, "n=1 q")
    t.assert_equal(rt, "n=1 strata")
    assert _stats()[:2] == (1, 0)  # on the device, with no decode attempt


# ---------------------------------------------------------------- column hand-over
@pytest.mark.parametrize("has32", [0, 1])
def test_column_hand_over(gpu, has32):
    """32 columns in a row: column c + 1 starts at the draw after column c's last accept
    (P[c + 1]).  Precondition: the columns start on both halves of a 64-bit output (the parity of
    p0 - h in k_dec_classify), and at least one column's last accept is the last of a thread's 16
    draws."""
    n, d = 1000, 32
    case = _state(100, has32)
    cols = _mirror_columns(case, n, d)
    assert {(start - has32) % 2 for start, _, _, _ in cols} == {0, 1}
    assert any((end - start) % 16 == 0 for start, end, _, _ in cols)
    assert _check(case, n, d)[:2] == (1, 1)


@pytest.mark.parametrize("seed,draws", [(18, 4095), (119, 4096), (278, 4097)])
def test_column_ends_on_block_edge(gpu, seed, draws):
    """Column 0 of default_rng(seed)'s stream consumes 4095, 4096 and 4097 draws: its last accept
    is the draw before the last of block 0, the last draw of block 0 (P[1] = 4096) and the first
    draw of block 1."""
    n, d = 2790, 2
    case = _seed_state(seed)
    cols = _mirror_columns(case, n, d)
    assert cols[0][1] == draws, cols[0][1]
    assert _check(case, n, d)[:2] == (1, 1)


# ---------------------------------------------------------------- k_scan_small
@pytest.mark.parametrize("n,blocks", [(2_838_720, 1024), (2_841_491, 1025), (5_689_299, 2049)])
def test_scan_small_run_lengths(gpu, n, blocks):
    """k_scan_small's run per thread goes 1 -> 2 at 1025 blocks and 2 -> 3 at 2049."""
    assert _tcap(n) == blocks * BLK, _tcap(n) // BLK
    assert _check(_state(blocks, 0), n, 1)[:2] == (1, 1)


# ---------------------------------------------------------------- every draw ambiguous
def _surely_ambiguous(n, sigmas):
    """(count, tcap): the draws 0 .. count - 1 of a column are ambiguous whatever their value: the
    band (draw_band restated on the host) has more than one mask boundary inside, which
    k_dec_classify never decides.  count is all of tcap but the tail, where the band's lower end
    runs past the column's last step."""
    from test_lhs_band_host import band_table, draw_band

    table, tcap = band_table(n, sigmas)
    inside, slo, shi = draw_band(table, n, np.arange(tcap))
    ihi, ilo = np.maximum(n - 1 - slo, 1), np.maximum(n - 1 - shi, 1)  # (outside the band: not counted)
    mask = lambda x: (1 << (np.floor(np.log2(x)).astype(np.int64) + 1)) - 1  # noqa: E731
    sure = inside & (mask(ihi) > 2 * mask(ilo) + 1)
    count = int(sure.sum())
    assert sure[:count].all() and tcap - 2 * BLK <= count
    return count, tcap


@pytest.mark.parametrize("n", [3, 1000, 5000, 70000])
def test_everything_ambiguous(gpu, n):
    """A band of 1e5 sigma: the host walks every draw ({A | 2^31, w} entries across the mask
    boundaries, x clamped), still on the device path in one attempt.

    At n = 5000 and n = 70000 the decode classifies 6 201 344 and 22 077 440 draws per column at
    this width, all ambiguous: more than the 2^22 the walk takes.  The decode used to give such a
    call to the host shuffles at once ((device, attempts) = (0, 3), which this test found); now
    the walk takes the first 2^22, and these columns end inside them, after about 1.4 n draws."""
    d = 2
    case = _state(7000 + n, 1)
    consumed = _mirror_columns(case, n, d)[-1][1]
    with _band(1e5):
        dev, att, amb = _check(case, n, d)
    assert (dev, att) == (1, 1), (dev, att, amb, _tcap(n, 1e5))
    assert amb >= consumed, (amb, consumed)


@pytest.mark.parametrize("n,sigmas", [(5000, 65536.0), (70000, 16384.0)])
def test_everything_ambiguous_under_the_cap(gpu, n, sigmas):
    """The same at the widest power of two that keeps tcap under the cap of 2^22 ambiguous draws:
    still all but the last draws classified are ambiguous with a band over several mask boundaries
    (asserted, the draws every column consumes among them), so the host walk decides them all."""
    d = 2
    sure, tcap = _surely_ambiguous(n, sigmas)
    assert tcap <= CAP < _tcap(n, 2 * sigmas)
    case = _state(7000 + n, 1)
    assert all(end - start < sure for start, end, _, _ in _mirror_columns(case, n, d))
    with _band(sigmas):
        dev, att, amb = _check(case, n, d)
    assert (dev, att) == (1, 1), (dev, att, amb)
    assert d * sure <= amb <= d * tcap, (amb, sure, tcap)


def test_over_the_cap(gpu):
    """More ambiguous draws than the walk takes (2^22) before the column ends, on every attempt:
    the column needs 4.41e6 draws on average (sd 1.4e3), all of them ambiguous.  Three attempts,
    then the host shuffles and k_lhs_combine, which must honour ldq and lds as well."""
    n = 3_000_000
    from test_lhs_band_host import expected_draws

    assert _tcap(n, 1e5) > CAP and float(expected_draws(n)[-1]) > 1.05 * CAP
    with _band(1e5):
        dev, att, amb = _check(_state(8000, 0), n, 1)
    assert (dev, att) == (0, 3), (dev, att, amb)


# ---------------------------------------------------------------- retries
RETRY_WIDTHS = [0.25, 0.5, 1.0, 2.0, 3.0]


def test_retry_that_succeeds(gpu):
    """Bands too narrow for the first attempt: the matrix is numpy's at every width, and the
    record is consistent (device == 1 with 1 .. 3 attempts, or device == 0 after all 3).  At
    least one width must succeed on a retry (device == 1, attempts >= 2).

    Measured on an MI355X, (device, attempts, ambiguous draws of the last attempt):
        0.25 sigma  (0, 3, 22777)   still too narrow at 1 sigma: the host shuffles
        0.5  sigma  (1, 3, 37933)   passes at 2 sigma
        1    sigma  (1, 2, 37933)   passes at 2 sigma: the successful retry
        2    sigma  (1, 1, 37933)
        3    sigma  (1, 1, 50779)"""
    n, d = 200_000, 3
    case = _state(9000, 1)
    ref = _numpy_lhs(case, n, d)
    seen = {}
    for w in RETRY_WIDTHS:
        with _band(w):
            seen[w] = dev, att, amb = _check(case, n, d, ref=ref, what=f"width {w}")
        assert (dev == 1 and 1 <= att <= 3) or (dev == 0 and att == 3), (w, dev, att, amb)
    print("retry widths (device, attempts, ambiguous):", seen)
    assert any(dev == 1 and att >= 2 for dev, att, _ in seen.values()), seen


def test_staging_reuse(gpu):
    """One workspace, calls in a row whose pinned staging needs differ: the initial 65536 entries,
    then 2^22 (n = 300 000 at 1e5 sigma: 4.8e7 ambiguous draws per column, of which the walk takes
    2^22 and the column about 4.2e5), the small size again, then a list of 2 488 114 or more
    (n = 1000 at 1e5 sigma), and the small size once more."""
    d = 2
    small, big = _state(9100, 1), _state(9101, 0)
    ws = _workspace(300_000, d)
    assert _check(small, 1000, d, ws)[:2] == (1, 1)
    with _band(1e5):
        dev, att, amb = _check(big, 300_000, d, ws)
    assert (dev, att) == (1, 1) and amb > d * CAP, (dev, att, amb)
    assert _check(small, 1000, d, ws)[:2] == (1, 1)
    with _band(1e5):
        dev, att, amb = _check(small, 1000, d, ws)
    assert (dev, att) == (1, 1) and amb >= d * _surely_ambiguous(1000, 1e5)[0] > 65536, (dev, att, amb)
    assert _check(small, 1000, d, ws)[:2] == (1, 1)


# ---------------------------------------------------------------- streams
def test_caller_streams(gpu):
    """The permutations run on a side stream that is joined to the caller's stream by events on
    every call: the same case on the current stream, on a fresh stream (results compared on that
    stream, with no device-wide synchronize in between) and on the first stream again."""
    import torch

    n, d = 100_003, 3
    case = _state(9200, 1)
    ref = _numpy_lhs(case, n, d)
    assert _check(case, n, d, ref=ref, what="first stream")[:2] == (1, 1)
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        from probabilit_amd import device

        assert device.stream() == other.cuda_stream
        assert _check(case, n, d, ref=ref, what="fresh stream")[:2] == (1, 1)
    assert _check(case, n, d, ref=ref, what="first stream again")[:2] == (1, 1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- refusals
def _refused(status, code, q, t):
    from probabilit_amd import _lib

    assert status == code, (status, _lib.last_error())
    assert "pbh_lhs_reference" in _lib.last_error(), _lib.last_error()
    assert q.untouched() and t.untouched(), "a refused call wrote"


def test_refusals(gpu):
    from probabilit_amd import _lib, device
    from probabilit_amd.qmc import _u128_words

    lib = _lib.load()
    n, d = 100, 3
    state, inc, has32, buf32 = _state(9300, 1)
    sw, iw = _u128_words(state), _u128_words(inc)
    s, i = _lib.np_ptr(sw), _lib.np_ptr(iw)
    ws = _workspace(n, d)
    q, t = Block(n, d), Block32(n, d)
    stream = device.stream()

    def call(s=s, i=i, n=n, d=d, qp=q.ptr, ldq=q.ld, tp=t.ptr, lds=t.ld, wp=ws.data_ptr(), wb=ws.numel()):
        return lib.pbh_lhs_reference_strata(s, i, has32, buf32, n, d, qp, ldq, tp, lds, wp, wb, stream)

    for kw in [dict(ldq=n - 1), dict(lds=n - 1), dict(n=0), dict(d=0), dict(n=2**31, ldq=2**31 + 3, lds=2**31 + 3),
               dict(qp=None), dict(wp=None), dict(s=None), dict(i=None)]:
        _refused(call(**kw), _lib.ERR_INVALID, q, t)
    _refused(call(wb=ws.numel() - 1), _lib.ERR_WORKSPACE, q, t)
    assert "workspace" in _lib.last_error()
    # lds is not looked at without strata, and the call then goes through
    assert call(tp=None, lds=0) == 0, _lib.last_error()
    q.assert_bits(_numpy_lhs((state, inc, has32, buf32), n, d)[0], "no strata")
    assert t.untouched()


def test_band_refusals(gpu):
    from probabilit_amd import _lib

    lib = _lib.load()
    cur, prev = ctypes.c_double(), ctypes.c_double(-1.0)
    _lib.check(lib.pbh_lhs_reference_band(0.0, ctypes.byref(cur)))
    assert cur.value == 6.0  # the default, which every test restores
    for bad in (-1.0, 1e6, float("nan")):
        assert lib.pbh_lhs_reference_band(bad, ctypes.byref(prev)) == _lib.ERR_INVALID
        assert "pbh_lhs_reference_band" in _lib.last_error() and prev.value == -1.0
    _lib.check(lib.pbh_lhs_reference_band(0.0, ctypes.byref(prev)))
    assert prev.value == cur.value
    _lib.check(lib.pbh_lhs_reference_band(0.0, ctypes.byref(prev)))  # and reading changed nothing
    assert prev.value == cur.value
