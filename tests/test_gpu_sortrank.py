"""The sort, rank and placement kernels, one entry point per call, at their own boundaries.

A  pbh_rankdata_average (raw, and through correlation.rankdata): k_load_keys with a stride, the
   64-bit one-sweep sort (k_digit_hist, k_digit_bases, k_onesweep<u64, u32>: tile 6144, pass
   skipping, the npass == 0 branch) and rank_finish in ranks mode (k_head_bounds, k_head_prefix,
   k_rank_finish: tile 4096, the carry across 256 tiles).  Reference: scipy.stats.rankdata,
   bit for bit.
B  pbh_ic_column_scores (HipPhases.column_scores, raw for stride 3): below n = 2^22 the same
   sort and rank_finish in scores mode with sorted_x; at and above it radix_sort_keys_top48
   (passes over bytes 2..7, k_fix_low16 with kFixCap = 64, the redo with every byte), the scores
   in rank order and the two-pass row placement (k_place_bases, k_onesweep<u32, f64>: tile 6144,
   k_place).  Reference: np.sort(x) exactly; ndtri(rankdata / (n + 1)) within atol = 1e-14 (the
   van der Waerden gate of test_column_scores_large_n); the flag 0 for finite and +-inf data, 1
   for one NaN.
C  pbh_ic_reorder, raw: k_make_codes, then PBH_STEP4 = lsd: four k_onesweep<u32, u32> passes
   (tile 9216) + k_runs_scan / k_runs_resolve (kMaxRun = 16), or = buckets: two passes +
   k_bucket_starts / k_code_buckets (kBucketCap = 2048, kBucketMaxRun = 16, 256 runs a bucket,
   resolve_run<4> / <16>); unset: buckets from n = 2^22 when the code histogram is flat.  Then
   one of three finishes: the placement (idx_out NULL: tie_fix_values, place_by_row with 0 / 1 / 2
   bucket passes for n <= 2^13, <= 2^21, above), the gather with eqprev (idx_out given:
   rank_finish in gather mode), or after a long run the 64-bit sort and the gather by keys.
   sorted_src[i] = i + 0.25, so y spells out the index.  Reference: r = rankdata(cs) as int64
   - 1; y[::y_rs] == sorted_src[r], idx_out == r.

Every input and output is a view into a wider device buffer of sentinels; the whole buffer is
compared after the call, so a write before, after or into the gaps of a strided view fails, and
so does an input that changed.

Which path a call took is read from the library's launch counters (pbh_timing_*: one count per
timed launch): the number of 64-bit passes (pass skipping), of k_load_keys launches (1 + the
redo of the top-48 sort; in C the 64-bit fallback), of placement passes.  The counts a test
expects come from the host mirrors of f64_to_key and code_of below, which are used to build
inputs and to assert their preconditions only, never as the reference of a result.

Mutation check (each change built into a scratch library, the 1666 cases of this file run against
it on an MI355X; failing cases):
    kFixCap 64 -> 63                                   2    column_scores_large[runs64] (the redo count)
    k_fix_low16 insertion compare > -> >=              0    equivalent: it only swaps the rows of equal
                                                            keys, which take one average rank
    kMaxRun / kBucketMaxRun loop bounds <= -> <      221    reorder: runs of 17 (lsd and buckets)
    pos without the (equal value, earlier) term       86    reorder with idx_out: every exact tie
                                                            (of the 438 gather cases: the rows are no
                                                            permutation then, so no placement was run)
    tie_fix_values midpoint (e - st + 1) / 2          74    reorder, placement finish: ties of even length
    k_rank_finish end - start - 1 in the last tile  1325    all three entry points
    k_head_prefix first carry 0 instead of -1          0    equivalent: position 0 is always a head, so
                                                            every last_head and prefix is >= 0 already
      (the forward carry not handed on instead)       10    rankdata_chunk_carry[*-1052673], large columns
    bucket size test > -> >= kBucketCap                2    reorder_bucket_limits[2048] (fallback count)
    nrun > 256 -> nrun > 255                           2    reorder_bucket_limits[256 pairs]
    pass skipping nonzero > 1 -> > 2                 185    every input with a key byte of exactly two
                                                            digits: twodigits*, rep*, tile_*, tiny and expon
                                                            scores, small n (wrong ranks, not only counts)
"""

import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
PAD = 64  # sentinel elements before and after every view

N_EDGE = [1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 8193, 9215, 9216, 9217,
          12287, 12288, 12289, 18431, 18432, 18433]
N_FEW = [4097, 6145, 9217, 18433]
N_CHUNK = [(1 << 20) - 1, 1 << 20, (1 << 20) + 4097]
N_PLACE = [(1 << 21) - 1, 1 << 21, (1 << 21) + 1]
N_LARGE = [1 << 22, (1 << 22) + 3]
RUN_LENGTHS = [2, 4, 5, 16, 17]


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------- host mirrors
def keys_of(x):
    """f64_to_key (pbh_common.h): the order-preserving 64-bit image of a double, -0.0 as +0.0."""
    b = (np.ascontiguousarray(x, dtype=np.float64) + 0.0).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def floats_of(keys):
    """key_to_f64."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    return np.where(k >> np.uint64(63), k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def varying_bytes(keys):
    """The byte positions (0 = lowest) on which the keys differ."""
    b = np.ascontiguousarray(keys, dtype="<u8").view(np.uint8).reshape(-1, 8)
    return [p for p in range(8) if b[:, p].min() != b[:, p].max()]


CODE_M, CODE_X0 = 1024, -8.5
CODE_W = 17.0 / CODE_M


@functools.lru_cache(maxsize=1)
def code_map():
    """code_map_host (pbh_ic.hip): bases and slopes of the piecewise-linear map through Phi."""
    import scipy.special

    j = np.arange(CODE_M + 1, dtype=np.float64)
    lo = CODE_X0 + j * CODE_W
    phi = 0.5 * scipy.special.erfc(-lo * 0.70710678118654752440)
    base = np.minimum(np.floor(phi * (4294967295.0 - CODE_M)) + j, 4294967295.0).astype(np.int64)
    scale = (base[1:] - base[:-1]).astype(np.float64) / CODE_W
    return _ro(base, scale)


def code_of(x):
    """code_of (pbh_ic.h) for finite or infinite x, as int64."""
    base, scale = code_map()
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - CODE_X0) * (1.0 / CODE_W)
        j = np.clip(np.nan_to_num(u, nan=0.0, posinf=0.0, neginf=0.0), 0, CODE_M - 1).astype(np.int64)
        lo = CODE_X0 + j.astype(np.float64) * CODE_W
        cnt = base[j + 1] - base[j]
        off = np.nan_to_num(np.floor((x - lo) * scale[j]), posinf=0.0, neginf=0.0)
    code = base[j] + np.clip(off, 0, cnt - 1).astype(np.int64)
    return np.where(~(u >= 0.0), 0, np.where(u >= CODE_M, 0xFFFFFFFF, code))


def x_of_code(c):
    """A double in the middle of code c's interval (c inside the map's range)."""
    base, scale = code_map()
    j = int(np.searchsorted(base, c, side="right") - 1)
    return CODE_X0 + j * CODE_W + (c - base[j] + 0.5) / scale[j]


def run_lengths(sorted_ids):
    """Lengths of the runs of equal entries of a sorted array."""
    n = len(sorted_ids)
    heads = np.flatnonzero(np.concatenate(([True], sorted_ids[1:] != sorted_ids[:-1])))
    return np.diff(np.concatenate((heads, [n])))


# ---------------------------------------------------------------------------- key families (A, B)
BASE_KEY = 0xBFF3C0CA428C59FB  # the key of 1.2345678...: byte 6 = 0xF3, so byte 7 = 0xFF would be a NaN


def fam_allbytes(n, rng):
    """Random 64-bit patterns: every key byte varies; both signs, subnormals, 1e+-300."""
    b = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    nonfinite = (b >> np.uint64(52)) & np.uint64(0x7FF) == np.uint64(0x7FF)
    b[nonfinite] &= ~np.uint64(1 << 62)  # the exponent of [1, 2): finite, and still distinct
    x = b.view(np.float64)
    special = np.array([5e-324, -5e-324, 1e300, -1e300, 1e-300, -1e-300, 1.1e-308, -3e-310])
    x[:min(n, 8)] = special[:min(n, 8)]
    return rng.permutation(x)


def fam_bytes(n, rng, positions, digits=None):
    """Keys equal to BASE_KEY outside the byte positions given, random digits there (`digits`: only
    these); the digit 0xFF of byte 7 would be a NaN and is not drawn."""
    k = np.full(n, BASE_KEY, dtype=np.uint64)
    for p in positions:
        allowed = np.array(digits if digits is not None else range(256 if p < 7 else 255), dtype=np.uint64)
        d = allowed[rng.integers(0, len(allowed), size=n)]
        k = (k & ~np.uint64(0xFF << (8 * p))) | (d << np.uint64(8 * p))
    x = floats_of(k)
    assert np.isfinite(x).all() and np.array_equal(keys_of(x), k)
    assert set(varying_bytes(k)) <= set(positions)
    return x


def fam_const(n, rng):
    return np.full(n, 3.75)


def fam_zeros(n, rng):
    return np.where(rng.integers(0, 2, size=n) == 1, 0.0, -0.0)


def fam_asc(n, rng):
    return np.arange(n) * 0.37 - 1000.0


def fam_desc(n, rng):
    return fam_asc(n, rng)[::-1].copy()


def fam_rep(n, rng, r, shuffle):
    x = np.repeat(np.arange((n + r - 1) // r), r)[:n] * 1.5 - 7.0
    return rng.permutation(x) if shuffle else x


def from_runs(n, rng, runs):
    """A shuffled multiset whose sorted order has tie runs on the inclusive position intervals
    `runs` (clipped to [0, n)) and distinct values elsewhere."""
    eq = np.zeros(n, dtype=bool)
    for s, e in runs:
        s, e = max(s, 0), min(e, n - 1)
        if e > s:
            eq[s + 1:e + 1] = True
    ids = np.cumsum(~eq)
    return rng.permutation(ids * 0.75 - 3.0)


def fam_tile_edges(n, rng):
    """Runs that end at 4095, start at 4096, end at 4097; end at 8192, start at 8193; straddle
    12288 from 12287 to 12289; cover 16383 and 16384 only."""
    return from_runs(n, rng, [(4093, 4095), (4096, 4097), (8190, 8192), (8193, 8195), (12287, 12289), (16383, 16384)])


def fam_tile_span(n, rng):
    """One run over [4000, 12400): two whole rank tiles lie inside it."""
    return from_runs(n, rng, [(4000, 12399)])


def chunk_positions(n):
    """The sorted positions where k_head_prefix carries from one chunk of 256 tiles to the next
    (forwards at 2^20; backwards it chunks from the end), and n - 2^20."""
    nt = (n + 4095) // 4096
    pos = {1 << 20, (nt - 256) * 4096, n - (1 << 20), (nt - 1) * 4096, n - 1}
    return sorted(p for p in pos if 0 < p < n)


def fam_chunk(n, rng, length):
    return from_runs(n, rng, [(p - length // 2, p - length // 2 + length - 1) for p in chunk_positions(n)])


def fam_inf(n, rng):
    x = rng.normal(size=n)
    rows = rng.choice(n, size=min(n, 9), replace=False)
    x[rows[:5]] = np.inf
    x[rows[5:]] = -np.inf
    return x


FAMILIES = {
    "allbytes": fam_allbytes,
    **{f"byte{p}": functools.partial(fam_bytes, positions=(p,)) for p in range(8)},
    "bytes07": functools.partial(fam_bytes, positions=(0, 7)),
    "twodigits2": functools.partial(fam_bytes, positions=(2,), digits=(0x11, 0x12)),
    "twodigits7": functools.partial(fam_bytes, positions=(7,), digits=(0x3F, 0xC0)),
    "const": fam_const,
    "zeros": fam_zeros,
    "asc": fam_asc,
    "desc": fam_desc,
    **{f"rep{r}{'s' if sh else ''}": functools.partial(fam_rep, r=r, shuffle=sh)
       for r in (2, 16, 17, 4096, 4097, 5000) for sh in (False, True)},
    "inf": fam_inf,
    "tile_edges": fam_tile_edges,
    "tile_span": fam_tile_span,
    "chunk2": functools.partial(fam_chunk, length=2),
    "chunk300000": functools.partial(fam_chunk, length=300_000),
}
ALL_N = ["allbytes"] + [f"byte{p}" for p in range(8)] + ["bytes07"]
FEW_N = [f for f in FAMILIES if f not in ALL_N and not f.startswith(("tile", "chunk"))]


def key_cases():
    """(family, n, stride): the first two families of the issue at every N_EDGE, the others at
    N_FEW, the tile families where the runs fit, and stride 3 at N_FEW."""
    out = [(f, n, 1) for n in N_EDGE for f in ALL_N]
    out += [(f, n, 1) for n in N_FEW for f in FEW_N]
    out += [("tile_edges", n, 1) for n in (18431, 18432, 18433)]
    out += [("tile_span", n, 1) for n in (12401, 16384, 18433)]
    out += [(f, n, 3) for n in N_FEW for f in ("allbytes", "byte1", "rep17s", "inf")] + [("tile_span", 18433, 3)]
    return out


KEY_CASES = key_cases()


def _id(case):
    return "-".join(str(c) for c in case)


def family(name, n):
    import zlib

    x = np.ascontiguousarray(FAMILIES[name](n, np.random.default_rng([11, zlib.crc32(name.encode()), n])),
                             dtype=np.float64)
    assert x.shape == (n,)
    return x


def rank_ref(x):
    import scipy.stats

    return scipy.stats.rankdata(x)


def scores_ref(ranks):
    import scipy.special

    return scipy.special.ndtri(ranks / (len(ranks) + 1))


# ---------------------------------------------------------------------------- device buffers
class View:
    """n elements with the given stride inside a device buffer of sentinels."""

    def __init__(self, n, stride=1, dtype=np.float64, host=None):
        import torch

        from probabilit_amd import device

        self.n, self.stride = n, stride
        self.sent = SENTINEL if dtype == np.float64 else -777
        self.size = PAD + n * stride + PAD
        self.buf = torch.full((self.size,), self.sent, dtype=torch.float64 if dtype == np.float64 else torch.int32,
                              device=device.device())
        self.view = self.buf[PAD:PAD + n * stride][::stride]
        assert self.view.shape[0] == n and (n == 1 or self.view.stride(0) == stride)
        self.host = None
        if host is not None:
            self.host = host
            self.view.copy_(torch.from_numpy(np.array(host)))

    def ptr(self):
        return self.view.data_ptr()

    def check(self, expected=None, what=""):
        """The whole buffer: `expected` (default: what was loaded) in the view, sentinels elsewhere."""
        got = self.buf.cpu().numpy()
        e = np.full(self.size, self.sent, dtype=got.dtype)
        e[PAD:PAD + self.n * self.stride][::self.stride] = self.host if expected is None else expected
        np.testing.assert_array_equal(got, e, err_msg=what)

    def get(self):
        return self.view.cpu().numpy()


class Launches:
    """The launch counts per timed kernel of the calls inside the block."""

    def __enter__(self):
        from probabilit_amd import _lib

        self.lib = _lib.load()
        self.lib.pbh_timing_reset()
        self.lib.pbh_timing_enable(1)
        self.count = {}
        return self

    def __exit__(self, *exc):
        from probabilit_amd import _lib

        self.lib.pbh_timing_enable(0)
        if exc[0] is None:
            for kid, name in enumerate(_lib.KERNELS):
                ms, c = ctypes.c_double(), ctypes.c_int64()
                _lib.check(self.lib.pbh_timing_read(kid, ctypes.byref(ms), ctypes.byref(c)))
                self.count[name] = int(c.value)
        self.lib.pbh_timing_reset()
        return False

    def __getitem__(self, name):
        return self.count[name]


def _ws(nbytes):
    from probabilit_amd import device

    return device.empty(int(nbytes), "uint8")


def rank_call(x, stride=1):
    """pbh_rankdata_average on a strided view of x; (ranks, launches)."""
    from probabilit_amd import _lib, device

    lib = _lib.load()
    n = len(x)
    xin, out = View(n, stride, host=x), View(n)
    nb = ctypes.c_size_t()
    _lib.check(lib.pbh_rank_workspace_size(n, ctypes.byref(nb)))
    ws = _ws(nb.value)
    with Launches() as L:
        _lib.check(lib.pbh_rankdata_average(xin.ptr(), stride, n, out.ptr(), ws.data_ptr(), nb.value, device.stream()),
                   "pbh_rankdata_average")
    xin.check(what="the input changed")
    return out, L


def scores_call(x, stride=1):
    """pbh_ic_column_scores; (scores, sorted_x, flag, launches)."""
    import torch

    from probabilit_amd import _lib, device
    from probabilit_amd.distributed import HipPhases

    lib = _lib.load()
    n = len(x)
    xin, s, sx = View(n, stride, host=x), View(n), View(n)
    flag = torch.zeros(3, dtype=torch.int32, device=device.device())
    with Launches() as L:
        if stride == 1:
            HipPhases().column_scores(xin.view, s.view, sx.view, flag[1:2])
        else:
            nb = ctypes.c_size_t()
            _lib.check(lib.pbh_rank_workspace_size(n, ctypes.byref(nb)))
            ws = _ws(nb.value)
            _lib.check(lib.pbh_ic_column_scores(xin.ptr(), stride, n, s.ptr(), sx.ptr(), flag[1:2].data_ptr(),
                                                ws.data_ptr(), nb.value, device.stream()), "pbh_ic_column_scores")
    xin.check(what="the input changed")
    f = flag.cpu().numpy()
    assert f[0] == 0 and f[2] == 0
    return s, sx, int(f[1]), L


def check_scores(s, sx, x, ranks):
    sx.check(np.sort(x), "sorted_x")
    s.check(s.get(), "scores: a write outside the view")
    np.testing.assert_allclose(s.get(), scores_ref(ranks), rtol=0, atol=1e-14)


# ---------------------------------------------------------------------------- A
@pytest.mark.parametrize("case", KEY_CASES, ids=_id)
def test_rankdata(gpu, case):
    """Ranks bit for bit; one 64-bit pass per varying key byte, one when none varies."""
    name, n, stride = case
    x = family(name, n)
    out, L = rank_call(x, stride)
    out.check(rank_ref(x), "ranks")
    assert L["k_scatter"] == max(1, len(varying_bytes(keys_of(x)))), "64-bit passes"
    assert L["k_load_keys"] == 1


@pytest.mark.parametrize("case", [(f, n) for n in N_CHUNK for f in ("chunk2", "chunk300000", "allbytes")], ids=_id)
def test_rankdata_chunk_carry(gpu, case):
    """n around 2^20: 256 rank tiles and more; tie runs of 2 and of 300 000 across the positions
    where k_head_prefix carries between chunks of 256 tiles, forwards and backwards."""
    name, n = case
    x = family(name, n)
    out, _ = rank_call(x)
    out.check(rank_ref(x), "ranks")


@pytest.mark.parametrize("n", [1, 4097, 18433])
def test_rankdata_wrapper(gpu, n):
    """correlation.rankdata: a host array, and a device view with stride 3 taken as it is."""
    from probabilit_amd.correlation import rankdata

    x = family("rep17s", n)
    ref = rank_ref(x)
    np.testing.assert_array_equal(rankdata(x), ref)
    xin = View(n, 3, host=x)
    np.testing.assert_array_equal(rankdata(xin.view).cpu().numpy(), ref)
    xin.check()


# ---------------------------------------------------------------------------- B
@pytest.mark.parametrize("case", KEY_CASES, ids=_id)
def test_column_scores(gpu, case):
    name, n, stride = case
    x = family(name, n)
    s, sx, flag, L = scores_call(x, stride)
    check_scores(s, sx, x, rank_ref(x))
    assert flag == 0
    assert L["k_scatter"] == max(1, len(varying_bytes(keys_of(x)))), "64-bit passes"


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("n", [1, 65, 6145])
def test_column_scores_nan_flag(gpu, n, stride):
    """A single NaN sets the flag (the outputs are undefined then and not looked at)."""
    x = family("allbytes", n)
    x[n // 2] = np.nan
    assert scores_call(x, stride)[2] == 1


def planted_runs(n, rng, lengths, redo_column=False):
    """A normal draw with runs of keys that share their top 48 bits planted on disjoint rows in
    shuffled order: bit patterns base + j (v + j ulp away from zero), low 16 bits of base zero.
    Per length one run at a positive and one at a negative base; a run of 5 at the column's
    minimum (-7.5) and one at its maximum (7.5); one run of 16 with duplicates inside."""
    x = rng.normal(size=n)
    groups = []
    for i, length in enumerate(lengths):
        for base in (1.0 + (i + 1) / 64.0, -(1.0 + (i + 1) / 64.0)):
            groups.append(np.array([base]).view(np.uint64)[0] + np.arange(length, dtype=np.uint64))
    groups.append(np.array([-7.5]).view(np.uint64)[0] + np.arange(5, dtype=np.uint64))
    groups.append(np.array([7.5]).view(np.uint64)[0] + np.arange(5, dtype=np.uint64))
    groups.append(np.array([0.375]).view(np.uint64)[0] + np.array([0, 0, 1, 1, 1, 2, 3, 3, 4, 5, 6, 6, 6, 6, 7, 8],
                                                                   dtype=np.uint64))
    planted = [5, 5, 16] + [ln for ln in lengths for _ in (0, 1)]
    vals = np.concatenate([rng.permutation(g) for g in groups]).view(np.float64)
    rows = rng.choice(n, size=len(vals), replace=False)
    x[rows] = vals
    # precondition: the runs of equal top-48 key bits longer than 2 are exactly the planted ones
    # (a normal draw has a few chance pairs), and they sit at sorted positions 0 and n - 1 too
    k = np.sort(keys_of(x))
    rl = run_lengths(k >> np.uint64(16))
    assert sorted(rl[rl > 2]) == sorted(p for p in planted if p > 2), sorted(rl[rl > 2])
    assert rl[0] == 5 and rl[-1] == 5
    assert len(varying_bytes(k)) == 8
    return x


@functools.lru_cache(maxsize=1)
def large_column(name, n):
    rng = np.random.default_rng([12, n, len(name)])
    if name == "normal":
        x = rng.normal(size=n)
    elif name == "allbytes":
        x = fam_allbytes(n, rng)
    elif name == "runs64":
        x = planted_runs(n, rng, [2, 3, 5, 16, 63, 64])
    elif name == "runs65":
        x = planted_runs(n, rng, [2, 3, 5, 16, 63, 64, 65])
    elif name == "integers":
        x = np.round(np.abs(rng.normal(size=n)) * 1000.0)
        assert set(varying_bytes(keys_of(x))) <= {2, 3, 4, 5, 6, 7}
    elif name == "integers_signed":  # the low key bytes are 0x00 (positive) or 0xFF (negative): long runs of ties
        x = np.round(rng.normal(size=n) * 1000.0)
        assert {0, 1} <= set(varying_bytes(keys_of(x)))
    elif name == "low16":
        x = (np.array([1.5]).view(np.uint64)[0] + rng.integers(0, 1 << 16, size=n, dtype=np.uint64)).view(np.float64)
        assert varying_bytes(keys_of(x)) == [0, 1]
    ranks = rank_ref(x)
    return _ro(x, ranks)


# name -> k_load_keys launches: 2 when a run longer than kFixCap = 64 makes the sort start again
LARGE_COLUMNS = {"normal": 1, "allbytes": 1, "runs64": 1, "runs65": 2, "integers": 1, "integers_signed": 2, "low16": 2}


@pytest.mark.parametrize("case", [(c, n) for n in N_LARGE for c in LARGE_COLUMNS], ids=_id)
def test_column_scores_large(gpu, case):
    """n >= 2^22: the top-48-bit sort.  Runs of up to 64 keys with equal top 48 bits are ordered
    by k_fix_low16 (k_load_keys runs once); a run of 65, or a column that is one run, takes the
    redo (twice); non-negative integers have constant low bytes and nothing to fix, integers of
    both signs two digits in them and ties far longer than 64."""
    name, n = case
    x, ranks = large_column(name, n)
    s, sx, flag, L = scores_call(x)
    check_scores(s, sx, x, ranks)
    assert flag == 0
    assert L["k_load_keys"] == LARGE_COLUMNS[name], "k_load_keys launches (1 + redo)"
    assert L["k_scatter<place>"] == 2 and L["k_place"] == 1


# ---------------------------------------------------------------------------- C
def plant(n, rng, groups):
    """A normal draw with the values of `groups` on disjoint rows in shuffled order."""
    cs = rng.normal(size=n)
    vals = np.concatenate([np.asarray(g, dtype=np.float64) for g in groups])
    cs[rng.choice(n, size=len(vals), replace=False)] = rng.permutation(vals)
    return cs


def chain(base, length):
    """`length` consecutive doubles from `base` upwards: distinct values, one code."""
    out = [base]
    for _ in range(length - 1):
        out.append(np.nextafter(out[-1], np.inf))
    c = np.array(out)
    assert len(set(code_of(c))) == 1, "the chain leaves its code"
    return c


def pat_dups(n, rng, lengths):
    return plant(n, rng, [np.full(ln, b + 0.01 * ln) for ln in lengths for b in (0.3, -1.7, 2.9)])


def pat_chains(n, rng, lengths):
    return plant(n, rng, [chain(b + 0.01 * ln, ln) for ln in lengths for b in (0.3, -1.7, 2.9)])


def pat_chain_mixed(n, rng):
    """Chains of 16 and of 5 members that mix duplicates with distinct neighbours."""
    c16, c5 = chain(0.3, 9), chain(-1.7, 3)
    return plant(n, rng, [c16[[0, 0, 1, 2, 2, 2, 3, 4, 5, 5, 6, 7, 7, 8, 8, 8]], c5[[0, 1, 1, 2, 2]]])


def pat_out_of_range(n, rng, k):
    """k values with code 0 (below -8.5, -8.5 itself, -1e300, two -inf) and k with the last code."""
    lo = np.concatenate(([-8.5, -1e300, -np.inf, -np.inf], -8.5 - np.arange(1, k - 3) * 0.125))
    assert len(lo) == k and (code_of(lo) == 0).all()
    assert run_lengths(np.sort(code_of(-lo))).max() in (k - 1, k)  # 8.5 itself may take the code before the last
    return plant(n, rng, [lo, -lo])


def pat_zero(n, rng):
    """Subnormals and +-0.0: one code, -0.0 ties with 0.0."""
    z = np.array([0.0, -0.0, 0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-310, 2.5e-308, -2.5e-308])
    assert len(set(code_of(z))) == 1
    return plant(n, rng, [z])


def pat_sorted(n, rng, descending):
    cs = np.sort(rng.normal(size=n))
    return cs[::-1].copy() if descending else cs


PATTERNS = {
    "normal": lambda n, rng: rng.normal(size=n),
    **{f"dup{ln}": functools.partial(pat_dups, lengths=(ln,)) for ln in RUN_LENGTHS},
    "dups": functools.partial(pat_dups, lengths=RUN_LENGTHS),
    **{f"chain{ln}": functools.partial(pat_chains, lengths=(ln,)) for ln in RUN_LENGTHS},
    "chains": functools.partial(pat_chains, lengths=RUN_LENGTHS),
    "chain_mixed": pat_chain_mixed,
    "oor10": functools.partial(pat_out_of_range, k=10),
    "oor20": functools.partial(pat_out_of_range, k=20),
    "zero": pat_zero,
    "round2": lambda n, rng: np.round(rng.normal(size=n), 2),
    "integer": lambda n, rng: np.round(rng.normal(size=n) * 3.0),
    "tiny": lambda n, rng: 1e-7 * rng.uniform(size=n),
    "expon": lambda n, rng: 100.0 * rng.exponential(size=n),
    "const": lambda n, rng: np.full(n, 0.5),
    "asc": functools.partial(pat_sorted, descending=False),
    "desc": functools.partial(pat_sorted, descending=True),
    # n >= 2^22: everything the bucket finish resolves / one run it does not
    "planted16": lambda n, rng: plant(n, rng, [np.full(ln, b + 0.01 * ln) for ln in (2, 4, 5, 16) for b in (0.3, -1.7)]
                                      + [chain(b + 0.01 * ln, ln) for ln in (2, 4, 5, 16) for b in (0.4, -1.6)]
                                      + [[-8.5, -1e300, -np.inf, -np.inf, -9.0, 8.5, 1e300, np.inf, np.inf, 9.0]]),
    "planted17": lambda n, rng: plant(n, rng, [chain(0.3, 17)]),
}
# the longest run of equal codes the planted values make (None: not planned, whatever comes)
LONGEST = {"normal": 1, **{f"dup{ln}": ln for ln in RUN_LENGTHS}, "dups": 17,
           **{f"chain{ln}": ln for ln in RUN_LENGTHS}, "chains": 17, "chain_mixed": 16, "oor10": 10, "oor20": 20,
           "zero": 10, "asc": 1, "desc": 1, "planted16": 16, "planted17": 17}
ENVS = [None, "lsd", "buckets"]


def pattern(name, n):
    import zlib

    cs = np.ascontiguousarray(PATTERNS[name](n, np.random.default_rng([13, zlib.crc32(name.encode()), n])),
                              dtype=np.float64)
    assert cs.shape == (n,)
    s = np.sort(cs)
    assert (np.diff(code_of(s)) >= 0).all(), "the code is not monotone in x"
    return cs


def index_ref(cs):
    import scipy.stats

    return scipy.stats.rankdata(cs).astype(np.int64) - 1


def reorder_cases():
    """(pattern, n, y_rs, idx_out given, PBH_STEP4)."""
    out = [("normal", n, y_rs, idx, env) for n in N_EDGE for y_rs in (1, 3) for idx in (False, True) for env in ENVS]
    for name in PATTERNS:
        if name in ("normal", "planted16", "planted17"):
            continue
        out += [(name, n, y_rs, idx, env) for n in N_FEW for y_rs, idx in ((1, False), (3, True)) for env in ENVS]
    return [c for c in out if not (c[4] == "buckets" and c[1] < 2)]


def reorder_call(cs, y_rs, with_idx, env, monkeypatch):
    """pbh_ic_reorder with sorted_src[i] = i + 0.25; checks y, idx_out and the inputs against the
    reference ranks r; returns the launches."""
    from probabilit_amd import _lib, device

    if env is None:
        monkeypatch.delenv("PBH_STEP4", raising=False)
    else:
        monkeypatch.setenv("PBH_STEP4", env)
    lib = _lib.load()
    n = len(cs)
    cin, src = View(n, host=cs), View(n, host=np.arange(n) + 0.25)
    y = View(n, y_rs)
    idx = View(n, dtype=np.int32) if with_idx else None
    nb = ctypes.c_size_t()
    _lib.check(lib.pbh_ic_reorder_workspace_size(n, ctypes.byref(nb)))
    ws = _ws(nb.value)
    with Launches() as L:
        _lib.check(lib.pbh_ic_reorder(cin.ptr(), n, src.ptr(), y.ptr(), y_rs, idx.ptr() if with_idx else None,
                                      ws.data_ptr(), nb.value, device.stream()), "pbh_ic_reorder")
    return cin, src, y, idx, L


def check_reorder(res, r):
    cin, src, y, idx, L = res
    y.check(r + 0.25, "y")
    if idx is not None:
        idx.check(r, "idx_out")
    cin.check(what="cs changed")
    src.check(what="sorted_src changed")


def place_passes(n):
    return 0 if n <= 1 << 13 else 1 if n <= 1 << 21 else 2


def check_path(L, name, n, with_idx, buckets):
    """What the launch counters must show: the code sort taken, the 64-bit fallback exactly when a
    run of equal codes is longer than 16 (or a forced bucket holds more than 2048), and the finish."""
    longest = LONGEST.get(name)
    if buckets:
        assert L["k_scatter<u32>"] == 2, "the bucket path sorts bytes 2 and 3 only"
    else:
        assert 1 <= L["k_scatter<u32>"] <= 4
    if longest is not None:
        assert L["k_load_keys"] == (1 if longest > 16 else 0), "64-bit fallback"
    fallback = L["k_load_keys"] == 1
    if not fallback:
        assert L["k_scatter"] == 0
    if not with_idx and not fallback:
        assert L["k_place"] == 1 and L["k_scatter<place>"] == place_passes(n), "placement passes"
        assert L["k_rank_finish<gather>"] == 0
    else:
        assert L["k_place"] == 0 and L["k_rank_finish<gather>"] == 1


@pytest.mark.parametrize("case", reorder_cases(), ids=_id)
def test_reorder(gpu, monkeypatch, case):
    name, n, y_rs, with_idx, env = case
    cs = pattern(name, n)
    res = reorder_call(cs, y_rs, with_idx, env, monkeypatch)
    check_reorder(res, index_ref(cs))
    check_path(res[4], name, n, with_idx, env == "buckets")


@functools.lru_cache(maxsize=1)
def big_pattern(name, n):
    cs = pattern(name, n)
    return _ro(cs, index_ref(cs))


@pytest.mark.parametrize("n", N_PLACE)
def test_reorder_placement_passes(gpu, monkeypatch, n):
    """n = 2^21 - 1, 2^21 (one bucket pass of the placement) and 2^21 + 1 (two)."""
    cs, r = big_pattern("normal", n)
    res = reorder_call(cs, 1, False, None, monkeypatch)
    check_reorder(res, r)
    check_path(res[4], "normal", n, False, False)


LARGE_REORDER = [("normal", 1, False), ("planted16", 1, False), ("planted16", 3, True), ("planted17", 1, False)]


@pytest.mark.parametrize("case", [(p, n, y_rs, idx) for n in N_LARGE for p, y_rs, idx in LARGE_REORDER], ids=_id)
def test_reorder_large(gpu, monkeypatch, case):
    """n >= 2^22 with PBH_STEP4 unset: N(0, 1)-shaped scores take the buckets; runs of up to 16
    equal codes, exact ties and the out-of-range codes are finished there, a run of 17 falls
    back to the 64-bit sort."""
    name, n, y_rs, with_idx = case
    cs, r = big_pattern(name, n)
    res = reorder_call(cs, y_rs, with_idx, None, monkeypatch)
    check_reorder(res, r)
    check_path(res[4], name, n, with_idx, True)


@pytest.mark.parametrize("name", ["round2", "integer", "tiny", "expon", "const"])
def test_reorder_large_not_flat(gpu, monkeypatch, name):
    """n = 2^22 with PBH_STEP4 unset: columns that are not N(0, 1)-shaped go to the four passes
    (the flatness test) or through the overflow flag to the 64-bit sort; the result is exact."""
    n = 1 << 22
    cs, r = big_pattern(name, n)
    res = reorder_call(cs, 1, False, None, monkeypatch)
    check_reorder(res, r)


def bucket_cluster(count, pairs):
    """n = 20 000 normal scores of which none lies in the top-16 bucket of code_of(0.3), plus, inside
    that bucket and 12 000 codes from its edges: `count` values with distinct codes 20 apart
    (pairs = False), or `count` pairs (x, nextafter(x)) of equal codes 100 apart."""
    n = 20_000
    rng = np.random.default_rng([14, count, int(pairs)])
    b = int(code_of(0.3)) >> 16
    cs = rng.normal(size=n)
    inside = np.flatnonzero(code_of(cs) >> 16 == b)
    cs[inside] = 2.0 + 0.001 * np.arange(len(inside))
    step = 100 if pairs else 20
    assert 12_000 + step * count < 65536 - 12_000
    x = np.array([x_of_code((b << 16) + 12_000 + step * i) for i in range(count)])
    vals = np.concatenate((x, np.nextafter(x, np.inf))) if pairs else x
    cs[rng.choice(n, size=len(vals), replace=False)] = rng.permutation(vals)
    # preconditions, by the mirror of the code map
    codes = np.sort(code_of(cs))
    assert (np.diff(codes) >= 0).all()
    mine = codes[codes >> 16 == b]
    rl = run_lengths(mine)
    if pairs:
        assert len(mine) == 2 * count and (rl == 2).all() and len(rl) == count
    else:
        assert len(mine) == count and (rl == 1).all()
    assert run_lengths(codes).max() <= 2 and np.bincount(codes >> 16).max() == len(mine)
    return cs


# (values or pairs in the bucket, pairs?, falls back to the 64-bit sort?)
BUCKET_LIMITS = [(2048, False, False), (2049, False, True), (256, True, False), (257, True, True)]


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("limit", BUCKET_LIMITS, ids=_id)
def test_reorder_bucket_limits(gpu, monkeypatch, limit, with_idx):
    """PBH_STEP4=buckets: a top-16 bucket of exactly kBucketCap = 2048 codes is finished in LDS,
    one of 2049 overflows; 256 runs of equal codes in a bucket fill the run table, 257 overflow.
    Overflow means the 64-bit sort: k_load_keys runs."""
    count, pairs, fallback = limit
    cs = bucket_cluster(count, pairs)
    res = reorder_call(cs, 3 if with_idx else 1, with_idx, "buckets", monkeypatch)
    check_reorder(res, index_ref(cs))
    L = res[4]
    assert L["k_scatter<u32>"] == 2
    assert L["k_load_keys"] == (1 if fallback else 0), "64-bit fallback"
