"""The stream generators of csrc/pbh_streams.hip at the C ABI, at their own launch boundaries:
k_mt_words / k_mt_block / k_mt_doubles (pbh_mt19937_random, pbh_mt19937_advance), k_pcg_random
(pbh_pcg64_random) and k_fill_halton (pbh_fill_halton).

test_gpu_streams.py reaches these kernels through qmc.make_source, which always passes a leading
dimension equal to nrows, column 0 and sizes below every grid cap.  Here every call writes a block
at an element offset inside a sentinel buffer with a leading dimension of nrows + 3 (abi_views.Block):
the three gap rows of every column, the column after the last and the padding must keep their
sentinels, and the values equal numpy's (RandomState / MT19937 / Generator(PCG64)) or scipy's
(Halton, van_der_corput) bit for bit.  Two comparisons take their expected values from the library
itself, each anchored by a numpy or scipy comparison in this file: shard against whole (Halton grid
stride, the PCG64 row shard is against numpy), and the composition of MT19937 jumps
(test_mt19937_jump_composition)."""

import ctypes

import numpy as np
import pytest

from abi_views import Block

pytestmark = pytest.mark.gpu

MT_LIMIT = 2 ** 44  # words of one key block's sequence the jump table reaches (mt::kJumpBits)


def _workspace(size_fn, *args):
    from probabilit_amd import _lib, device

    need = ctypes.c_size_t()
    _lib.check(size_fn(*args, ctypes.byref(need)))
    return device.empty(max(int(need.value), 1), "uint8")


# ---------------------------------------------------------------- MT19937
def _mt_key(seed, blocks=0):
    """A key block of numpy's: RandomState(seed)'s, `blocks` twists on."""
    rs = np.random.RandomState(seed)
    if blocks:
        rs.random_sample(312 * blocks)
    return np.ascontiguousarray(rs.get_state(legacy=False)["state"]["key"], dtype=np.uint32)


def _mt_numpy(key, pos, row0, nrows, d):
    rs = np.random.RandomState()
    st = rs.get_state(legacy=False)
    st["state"] = {"key": key, "pos": pos}
    rs.set_state(st)
    rs.random(row0 * d)
    return rs.random((nrows, d))


def _mt_random(key, pos, row0, nrows, d, after=None):
    """(status, block) of pbh_mt19937_random into a block with ldq = nrows + 3."""
    from probabilit_amd import _lib, device

    lib = _lib.load()
    ws = _workspace(lib.pbh_mt19937_workspace_size, nrows, d)
    blk = Block(nrows, d, after=after)
    st = lib.pbh_mt19937_random(_lib.np_ptr(key), pos, row0, nrows, d, blk.ptr, blk.ld, ws.data_ptr(), ws.numel(),
                                device.stream())
    return st, blk


def _mt_check(key, pos, row0, nrows, d, after=None):
    from probabilit_amd import _lib

    st, blk = _mt_random(key, pos, row0, nrows, d, after)
    assert st == 0, _lib.last_error()
    blk.assert_bits(_mt_numpy(key, pos, row0, nrows, d), f"MT19937 pos={pos} row0={row0} nrows={nrows} d={d}")


def _mt_advance(key, pos, nwords):
    """(status, key_out, pos_out) of pbh_mt19937_advance; the outputs start as 0xA5 bytes and -7."""
    from probabilit_amd import _lib, device

    lib = _lib.load()
    ws = _workspace(lib.pbh_mt19937_workspace_size, 0, 0)
    key_out = np.full(624, 0xA5A5A5A5, dtype=np.uint32)
    pos_out = ctypes.c_int32(-7)
    st = lib.pbh_mt19937_advance(_lib.np_ptr(key), pos, nwords, _lib.np_ptr(key_out), ctypes.byref(pos_out),
                                 ws.data_ptr(), ws.numel(), device.stream())
    return st, key_out, int(pos_out.value)


@pytest.mark.parametrize("nrows,d", [(1, 1), (257, 3), (1000, 33)])
def test_mt19937_block_geometry(gpu, nrows, d):
    """ldq = nrows + 3 at every position of the key block a RandomState can be in (pos 0 is what
    set_state accepts: with row0 = 0 it is the one start that needs no jump, the g0 == 0 branch of
    k_mt_words) and at a row shard."""
    key = _mt_key(5, blocks=2)
    for pos in (0, 1, 623, 624):
        for row0 in (0, 777):
            _mt_check(key, pos, row0, nrows, d)


@pytest.mark.parametrize("nrows,d,row0", [(2048, 1, 0), (2049, 1, 0), (683, 3, 777),  # 2 n d = 4096, 4098, 4098
                                          (4_194_304, 1, 0), (4_194_305, 1, 0)])
def test_mt19937_segment_edges(gpu, nrows, d, row0):
    """One 4096-word segment; a second segment that holds one pair of words; and the two sides of
    mt_segment's switch from 4096-word to 8192-word segments at 2 n d = 4096 * 2048."""
    _mt_check(_mt_key(6), 624, row0, nrows, d, after=4096)


def test_mt19937_doubles_grid_stride(gpu):
    """k_mt_doubles caps its grid at 65536 blocks of 256: 257 elements more take the stride loop."""
    _mt_check(_mt_key(7), 624, 0, 65536 * 256 + 257, 1, after=4096)


@pytest.mark.parametrize("distance,pos,d", [(2 ** 24 - 1, 624, 8), (2 ** 23 + 2 ** 11 + 1, 624, 3)])
def test_mt19937_offsets_against_numpy(gpu, distance, pos, d):
    """A shard whose first segment jumps pos + 2 row0 d - 1 = `distance` words: every polynomial
    x^(2^i), i < 24, in one jump, and a sparse distance, against numpy's own prefix."""
    row0, rem = divmod(distance + 1 - pos, 2 * d)
    assert rem == 0 and pos + 2 * row0 * d - 1 == distance
    _mt_check(_mt_key(8), pos, row0, 300, d)


@pytest.mark.parametrize("pos", [1, 623, 624])
def test_mt19937_advance_against_numpy(gpu, pos):
    from probabilit_amd import _lib

    key = _mt_key(9, blocks=1)
    for nwords in (0, 1, 2, 623, 624, 625, 1248):
        bg = np.random.MT19937()
        st = bg.state
        st["state"] = {"key": key, "pos": pos}
        bg.state = st
        bg.random_raw(nwords)
        status, key_out, pos_out = _mt_advance(key, pos, nwords)
        assert status == 0, _lib.last_error()
        assert pos_out == bg.state["state"]["pos"], (pos, nwords)
        np.testing.assert_array_equal(key_out, bg.state["state"]["key"], err_msg=f"pos={pos} nwords={nwords}")


def test_mt19937_jump_composition(gpu):
    """The jump polynomials x^(2^i) for i >= 24, which numpy cannot reach cheaply.

    This is a consistency argument, not a comparison with numpy.  With A = 624 * floor(2^i / 624):

      (a) advancing by A twice lands on the state of advancing by 2 A once (key and pos), i = 24 .. 42;
      (b) 64 draws at row0 = A / 2 (d = 1) from K equal the first 64 draws from the state advanced by
          A words, i = 24 .. 43.

    The jump distances are A - 1 (both steps of the left side of (a), and the right side of (b)),
    2 A - 1 (right side of (a)) and A + 623 (left side of (b)): A - 1 < 2^i uses only polynomials
    below i, while 2 A - 1 and A + 623 lie in [2^i, 2^(i+1)) and use polynomial i once.  So each
    identity ties polynomial i to polynomials below it; by induction from the numpy cases of this
    file (every polynomial below 24: test_mt19937_offsets_against_numpy) all 44 are anchored.  A wrong
    polynomial p' != x^(2^i) mod phi cannot satisfy them: phi is irreducible and p' - x^(2^i) has a
    lower degree, so (p' - x^(2^i))(T) maps no nonzero state to zero, and the state it lands on, and
    the words drawn from it, differ.  A jump loop that drops or misreads bit i of the distance lands
    2^i words short on one side only and fails the same way."""
    from probabilit_amd import _lib

    key = _mt_key(10, blocks=3)

    def adv(k, pos, w):
        st, k2, p2 = _mt_advance(k, pos, w)
        assert st == 0, _lib.last_error()
        return k2, p2

    def rnd(k, pos, row0):
        st, blk = _mt_random(k, pos, row0, 64, 1)
        assert st == 0, _lib.last_error()
        blk.assert_clean()
        return blk.rows()

    for i in range(24, 44):
        A = 624 * (2 ** i // 624)
        k1, p1 = adv(key, 624, A)
        if i <= 42:
            k2, p2 = adv(k1, p1, A)
            k3, p3 = adv(key, 624, 2 * A)
            assert p2 == p3, i
            np.testing.assert_array_equal(k2, k3, err_msg=f"advance by A twice != advance by 2A, i = {i}")
        np.testing.assert_array_equal(rnd(key, 624, A // 2), rnd(k1, p1, 0), err_msg=f"draws at row0 = A/2, i = {i}")
    # the anchor of the right side of (b): the draws from an advanced state are numpy's
    k1, p1 = adv(key, 624, 1248)
    np.testing.assert_array_equal(rnd(k1, p1, 0), _mt_numpy(key, 624, 624, 64, 1))


def test_mt19937_range_guard(gpu):
    """The jump table reaches words below 2^44 of the key block's sequence.  A call whose last word
    lies below the limit succeeds (and gives the draws that follow the advanced state); one whose
    last word is at or beyond it is an error that names the limit and writes nothing."""
    from probabilit_amd import _lib

    key = _mt_key(11)
    # random: words [pos + 2 row0, pos + 2 row0 + 2) of one draw
    inside = [(624, MT_LIMIT // 2 - 313), (623, MT_LIMIT // 2 - 313)]  # last word 2^44 - 1, 2^44 - 2
    outside = [(624, MT_LIMIT // 2 - 312),  # first word 2^44
               (623, MT_LIMIT // 2 - 312),  # first word 2^44 - 1, last word 2^44: straddles the limit
               (624, 2 ** 62)]              # 2 row0 d overflows an int64
    for pos, row0 in inside:
        st, blk = _mt_random(key, pos, row0, 1, 1)
        assert st == 0, _lib.last_error()
        blk.assert_clean()
        st2, k2, p2 = _mt_advance(key, pos, 2 * row0)
        assert st2 == 0, _lib.last_error()
        st3, blk3 = _mt_random(k2, p2, 0, 1, 1)
        assert st3 == 0, _lib.last_error()
        np.testing.assert_array_equal(blk.rows(), blk3.rows())
    for pos, row0 in outside:
        for nrows, d in [(1, 1), (3, 128)]:
            st, blk = _mt_random(key, pos, row0, nrows, d)
            assert st != 0, (pos, row0, nrows, d)
            assert "2^44" in _lib.last_error(), _lib.last_error()
            assert blk.untouched()
    # advance: the last word drawn is pos + nwords - 1
    st, _, _ = _mt_advance(key, 624, MT_LIMIT - 624)
    assert st == 0, _lib.last_error()
    for pos, nwords in [(624, MT_LIMIT - 623), (1, MT_LIMIT), (624, 2 ** 63 - 1)]:
        st, key_out, pos_out = _mt_advance(key, pos, nwords)
        assert st != 0, (pos, nwords)
        assert "2^44" in _lib.last_error(), _lib.last_error()
        assert (key_out == 0xA5A5A5A5).all() and pos_out == -7


# ---------------------------------------------------------------- PCG64
BIT127 = 1 << 127
PCG_STATE = 0x0123456789ABCDEF_0FEDCBA987654321  # bit 127 clear
PCG_INC = 0x1BADC0DE5EEDF00D_0DDBA11C0FFEE123  # odd (as numpy's always is), bit 127 clear


def _pcg_numpy(state, inc, draw0, nrows, d):
    bg = np.random.PCG64()
    st = bg.state
    st["state"] = {"state": state, "inc": inc}
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    bg.advance(draw0)
    return np.random.Generator(bg).random((nrows, d))


def _pcg_random(state, inc, draw0, nrows, d, after=None):
    from probabilit_amd import _lib, device
    from probabilit_amd.qmc import _u128_words

    lib = _lib.load()
    ws = _workspace(lib.pbh_pcg64_workspace_size)
    blk = Block(nrows, d, after=after)
    s, i = _u128_words(state), _u128_words(inc)
    st = lib.pbh_pcg64_random(_lib.np_ptr(s), _lib.np_ptr(i), draw0, nrows, d, blk.ptr, blk.ld, ws.data_ptr(),
                              ws.numel(), device.stream())
    assert st == 0, _lib.last_error()
    return blk


@pytest.mark.parametrize("draw0", [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62 + 12345])
def test_pcg64_draw0_and_high_words(gpu, draw0):
    """A base draw given directly (below, at and far beyond 2^32), and states and increments with
    and without bit 127 (the high bit of the high 64-bit word the ABI passes), against
    PCG64.advance(draw0) + Generator.random."""
    assert PCG_STATE < BIT127 and PCG_INC < BIT127 and PCG_INC & 1
    for state in (PCG_STATE, PCG_STATE | BIT127):
        for inc in (PCG_INC, PCG_INC | BIT127):
            for d in (1, 3, 128):
                for nrows in (1, 257):
                    blk = _pcg_random(state, inc, draw0, nrows, d)
                    blk.assert_bits(_pcg_numpy(state, inc, draw0, nrows, d),
                                    f"PCG64 draw0={draw0} state>>127={state >> 127} inc>>127={inc >> 127} "
                                    f"nrows={nrows} d={d}")


def test_pcg64_row_shard(gpu):
    """draw0 = row0 * d is rows row0 onward of the full matrix (what a row shard passes)."""
    row0, nrows, d = 70_001, 257, 3
    full = _pcg_numpy(PCG_STATE | BIT127, PCG_INC, 0, row0 + nrows, d)
    _pcg_random(PCG_STATE | BIT127, PCG_INC, row0 * d, nrows, d).assert_bits(full[row0:], "PCG64 row shard")


def test_pcg64_grid_stride(gpu):
    """k_pcg_random caps its grid at 65536 blocks of 256 rows: 257 rows more take the stride loop."""
    nrows = 65536 * 256 + 257
    blk = _pcg_random(PCG_STATE, PCG_INC | BIT127, 5, nrows, 1, after=4096)
    blk.assert_bits(_pcg_numpy(PCG_STATE, PCG_INC | BIT127, 5, nrows, 1), "PCG64 grid stride")


# ---------------------------------------------------------------- scrambled Halton
class _Halton:
    """scipy.stats.qmc.Halton(d, rng=seed)'s bases and digit permutations, and pbh_fill_halton."""

    def __init__(self, d, seed):
        from probabilit_amd import _lib, qmc

        self.d = d
        self.bases, self.counts, perms = qmc.halton_setup(d, seed)
        self.perms = np.ascontiguousarray(perms)
        self.by_dim = np.split(self.perms, np.cumsum(self.counts * self.bases)[:-1])
        lib = _lib.load()
        self.ws = _workspace(lib.pbh_halton_workspace_size, _lib.np_ptr(self.bases), _lib.np_ptr(self.counts), d)

    def fill(self, row0, nrows, col0, ncols, after=None):
        from probabilit_amd import _lib, device

        blk = Block(nrows, ncols, after=after)
        st = _lib.load().pbh_fill_halton(_lib.np_ptr(self.bases), _lib.np_ptr(self.counts), _lib.np_ptr(self.perms),
                                         self.d, row0, nrows, col0, ncols, blk.ptr, blk.ld, self.ws.data_ptr(),
                                         self.ws.numel(), device.stream())
        assert st == 0, _lib.last_error()
        return blk

    def scipy(self, row0, nrows, col0, ncols):
        """The same rows and columns by scipy's van_der_corput on the same permutations."""
        from scipy.stats._qmc import van_der_corput

        cols = [van_der_corput(nrows, int(self.bases[c]), start_index=row0, scramble=True,
                               permutations=self.by_dim[c].reshape(self.counts[c], self.bases[c]))
                for c in range(col0, col0 + ncols)]
        return np.column_stack(cols)


@pytest.fixture(scope="module")
def halton33(gpu):
    return _Halton(33, 11)


@pytest.mark.parametrize("col0", [0, 5, 17])
def test_halton_column_blocks(gpu, halton33, col0):
    """Columns col0 .. d - 2 of d = 33 into a block with ldq = nrows + 3: the same rows and columns
    of the full (col0 = 0, ncols = d) call, and scipy's van_der_corput at start_index = row0."""
    h = halton33
    ncols = h.d - col0 - 1
    for row0 in (0, 777):
        for nrows in (1, 257):
            blk = h.fill(row0, nrows, col0, ncols)
            blk.assert_bits(h.scipy(row0, nrows, col0, ncols), f"Halton col0={col0} row0={row0} nrows={nrows}")
            full = h.fill(row0, nrows, 0, h.d)
            full.assert_clean()
            blk.assert_same(full.cols()[col0:col0 + ncols], "block vs the full call")


def test_halton_128_dimensions(gpu):
    """d = 128 (bases up to 719) against the engine itself."""
    import scipy.stats

    h = _Halton(128, 3)
    assert h.bases[-1] == 719
    h.fill(0, 300, 0, 128).assert_bits(scipy.stats.qmc.Halton(128, rng=3).random(300), "Halton d=128")


def test_halton_crosses_2_32_in_one_launch(gpu):
    """Rows 2^32 - 3 .. 2^32 + 3: the 32-bit and the 64-bit digit path in one call."""
    h = _Halton(5, 7)
    row0 = 2 ** 32 - 3
    h.fill(row0, 7, 0, 5).assert_bits(h.scipy(row0, 7, 0, 5), "Halton across 2^32")


def test_halton_grid_stride(gpu):
    """k_fill_halton caps its grid at 16384 blocks of 256 rows per column: 257 rows more take the
    stride loop.  Against two shard calls that each stay under the cap, and the first and last 257
    rows against scipy."""
    import torch

    h = _Halton(1, 9)
    cap = 16384 * 256
    nrows = cap + 257
    whole = h.fill(0, nrows, 0, 1, after=4096)
    whole.assert_clean()
    cut = 2_097_153
    a, b = h.fill(0, cut, 0, 1, after=4096), h.fill(cut, nrows - cut, 0, 1, after=4096)
    assert cut <= cap and nrows - cut <= cap
    a.assert_clean()
    b.assert_clean()
    whole.assert_same(torch.cat([a.cols(), b.cols()], dim=1), "whole vs shards")
    got = whole.cols().cpu().numpy().view(np.float64)[0]
    np.testing.assert_array_equal(got[:257], h.scipy(0, 257, 0, 1)[:, 0])
    np.testing.assert_array_equal(got[-257:], h.scipy(nrows - 257, 257, 0, 1)[:, 0])
