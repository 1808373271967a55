"""A plain Python mirror of numpy's Generator.shuffle on PCG64, draw by draw, for the tests of the
device decode of the reference LHS stream (test_lhs_band_host.py pins it to numpy itself;
test_gpu_lhs_decode_kernels.py takes its preconditions from it).

Generator.shuffle of a 1-d array of n elements runs i = n-1 .. 1, j = random_interval(i), swap
x[i], x[j].  random_interval(max) draws next_uint32() until (w & mask(max)) <= max, and PCG64's
next_uint32 hands out the low, then the high half of each 64-bit output, after a half a previous
call left buffered (has_uint32 / uinteger).  The mirror works on that paired 32-bit stream as a
list of words and keeps, for every draw, the number of steps done before it: the state the decode
has to bracket with its band.
"""

import numpy as np


def mask_of(x):
    x |= x >> 1
    x |= x >> 2
    x |= x >> 4
    x |= x >> 8
    x |= x >> 16
    return x


def generator(state, inc, has32=0, buf32=0):
    """A Generator(PCG64()) at the given 128-bit state and increment and 32-bit buffer."""
    g = np.random.Generator(np.random.PCG64())
    g.bit_generator.state = {"bit_generator": "PCG64", "state": {"state": int(state), "inc": int(inc)},
                             "has_uint32": int(has32), "uinteger": int(buf32)}
    return g


def words32(g, count):
    """The next `count` values of next_uint32() of Generator g, as Python ints; g is not advanced."""
    st = g.bit_generator.state
    bg = np.random.PCG64()
    bg.state = st
    has = int(st["has_uint32"])
    nraw = (count - has + 1) // 2 + 1
    raw = bg.random_raw(nraw)  # next_uint64: passes the 32-bit buffer by
    out = np.empty(2 * nraw, dtype=np.uint64)
    out[0::2] = raw & np.uint64(0xFFFFFFFF)
    out[1::2] = raw >> np.uint64(32)
    out = out.tolist()
    if has:
        out.insert(0, int(st["uinteger"]))
    return out[:count]


def column(words, n, start=0):
    """One shuffle of n elements reading words[start:].  Returns (end, steps, targets): the column
    consumes the draws start .. end - 1, steps[k] is the number of steps done before draw
    start + k, and targets[i] = j_i for i = 1 .. n-1 (targets[0] = 0)."""
    t = start
    steps = []
    targets = [0] * n
    for s, i in enumerate(range(n - 1, 0, -1)):
        m = mask_of(i)
        while True:
            v = words[t] & m
            t += 1
            steps.append(s)
            if v <= i:
                break
        targets[i] = v
    return t, steps, targets


def apply_targets(targets):
    """The swaps i = n-1 .. 1 with x[targets[i]], applied to arange(1, n + 1)."""
    n = len(targets)
    x = list(range(1, n + 1))
    for i in range(n - 1, 0, -1):
        j = targets[i]
        x[i], x[j] = x[j], x[i]
    return np.array(x, dtype=np.int64)


def draws_needed(n, d):
    """Words that d columns consume with room to spare: a step takes at most 2 draws on average."""
    return 2 * n * d + 64 * int(np.sqrt(n * d)) + 4096


def columns(g, n, d):
    """d shuffles in a row from Generator g's state (g is not advanced): a list of (start, end,
    steps, targets) per column, start and end in draws from the first."""
    words = words32(g, draws_needed(n, d))
    out, t = [], 0
    for _ in range(d):
        end, steps, targets = column(words, n, t)
        out.append((t, end, steps, targets))
        t = end
    return out
