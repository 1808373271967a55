"""What the tests of pbh_binned_sums and of inspection.binned_statistic / sensitivity compare with:
the per-bin sums by math.fsum over the terms rounded as the kernel rounds them, and the error
bound stated beside pbh_binned_sums in include/probabilit_hip.h, evaluated and propagated."""

import math

import numpy as np

U = 2.0 ** -53  # the unit roundoff of the header's bound


def bin_index(x, edges):
    """np.histogram's bin of every x among the edges (searchsorted right - 1, the last bin closed),
    -1 for a NaN and for a value outside [edges[0], edges[-1]]."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(edges, dtype=np.float64)
    b = np.searchsorted(e, x, "right") - 1
    b[x == e[-1]] = len(e) - 2
    with np.errstate(invalid="ignore"):
        inside = (x >= e[0]) & (x <= e[-1])
    return np.where(inside, b, -1)


def _fsum(v):
    try:
        return math.fsum(v)
    except (ValueError, OverflowError):  # inf - inf, or finite terms beyond the range
        with np.errstate(all="ignore"):
            return float(np.sum(v))


def raw_sums(x, y, edges, centre):
    """Per bin of x: count (int64), s1 = sum d, s2 = sum d^2, a1 = sum |d|, with d = fl(y - centre)
    and d^2 rounded once, each sum correctly rounded (s2 is also the header's sum |t| for s2)."""
    y = np.asarray(y, dtype=np.float64)
    m = len(edges) - 1
    b = bin_index(x, edges)
    order = np.argsort(b, kind="stable")
    cuts = np.searchsorted(b[order], np.arange(m + 1))
    with np.errstate(all="ignore"):
        d = y - centre
        q = d * d
    count, s1, s2, a1 = np.zeros(m, np.int64), np.zeros(m), np.zeros(m), np.zeros(m)
    for i in range(m):
        rows = order[cuts[i]:cuts[i + 1]]
        count[i] = len(rows)
        if len(rows):
            s1[i], s2[i], a1[i] = _fsum(d[rows]), _fsum(q[rows]), _fsum(np.abs(d[rows]))
    return count, s1, s2, a1


def sum_bounds(count, s2, a1):
    """The header's bounds: |s1 - exact| <= m u sum |y - c| and |s2 - exact| <= (m + 2) u sum (y - c)^2
    for the m = count rows of a bin."""
    count = np.asarray(count, dtype=np.float64)
    return count * U * a1, (count + 2) * U * s2


def finish_bounds(count, s1, s2, a1, centre):
    """The header's bounds carried through inspection.binned_finish, per bin, to first order, as
    {statistic: bound}.  With m rows, m1 = s1 / m, A1 = a1 / m, A2 = s2 / m and B1, B2 the bounds of
    s1 and s2:
      sum  = s1 + m c:   B1, and two roundings (the product, the sum): 2 u (|s1| + m |c|)
      mean = c + s1 / m: B1 / m, and two roundings (the quotient, the sum): 2 u (|m1| + |c|)
      var  = s2 / m - m1^2: B2 / m + 2 |m1| B1 / m, and four roundings (two quotients, the square, the
             difference), each at most u (A2 + m1^2); with |m1| <= A1 and A1^2 <= A2 this is at most
             E = u ((m + 2) A2 + 2 m A2 + 8 A2) = (3 m + 10) u A2
      std  = sqrt(max(var, 0)): |sqrt(a) - sqrt(b)| <= min(sqrt |a - b|, |a - b| / sqrt(max(a, b))), so
             min(sqrt(E), E / std) and one rounding of the root, u std."""
    m = np.maximum(np.asarray(count, dtype=np.float64), 1.0)
    b1, _ = sum_bounds(m, s2, a1)
    with np.errstate(all="ignore"):
        m1, A2 = s1 / m, s2 / m
        E = (3 * m + 10) * U * A2
        std = np.sqrt(np.maximum(A2 - m1 * m1, 0.0))
        std_bound = np.where(std > 0, np.minimum(np.sqrt(E), E / np.where(std > 0, std, 1.0)), np.sqrt(E)) + U * std
    return {"count": np.zeros_like(m), "sum": b1 + 2 * U * (np.abs(s1) + m * abs(centre)),
            "mean": b1 / m + 2 * U * (np.abs(m1) + abs(centre)), "std": std_bound}


def reference_allowance(x, y, edges, statistic):
    """What scipy.stats.binned_statistic's own result may be off by, per bin.  Its sum is
    np.bincount's serial sum of the m values: (m - 1) u sum |y|; its mean that over m, one more
    rounding; its std is np.std of the bin's values: the mean by numpy's pairwise sum (at most
    L = 17 + log2 m additions deep, so off by at most L u mean |y|, which shifts every deviation
    alike and adds its square to the variance), the deviations rounded once, their squares once,
    summed L deep and divided: (L + 4) u var + (L u mean |y|)^2 on the variance, through the root as
    in finish_bounds."""
    y = np.asarray(y, dtype=np.float64)
    m_bins = len(edges) - 1
    b = bin_index(x, edges)
    out = np.zeros(m_bins)
    for i in range(m_bins):
        v = y[b == i]
        m = len(v)
        if m == 0 or statistic == "count":
            continue
        ay = float(np.abs(v).sum())
        if statistic == "sum":
            out[i] = m * U * ay
        elif statistic == "mean":
            out[i] = (m + 1) * U * ay / m
        else:
            L = 17 + math.log2(m)
            var = float(np.var(v))
            E = (L + 4) * U * var + (L * U * ay / m) ** 2
            out[i] = min(math.sqrt(E), E / math.sqrt(var)) if var > 0 else math.sqrt(E)
            out[i] += U * math.sqrt(var)
    return out


def exact_correlation_ratio(x, y, edges):
    """Var(E[Y | X]) / Var(Y) = sum_b n_b (mean_b - mean)^2 / sum (y - mean)^2 over the rows whose x
    is inside the edges, in exact rational arithmetic, rounded once (NaN for a constant y)."""
    from fractions import Fraction

    b = bin_index(x, edges)
    total, squares, per_bin = Fraction(0), Fraction(0), {}
    for bi, v in zip(b.tolist(), np.asarray(y, dtype=np.float64).tolist()):
        if bi < 0:
            continue
        f = Fraction(v)
        total += f
        squares += f * f
        n_b, t_b = per_bin.get(bi, (0, Fraction(0)))
        per_bin[bi] = (n_b + 1, t_b + f)
    N = sum(n_b for n_b, _ in per_bin.values())
    den = squares - total * total / N
    if den <= 0:
        return float("nan")
    num = sum(t_b * t_b / n_b for n_b, t_b in per_bin.values()) - total * total / N
    return float(num / den)


def correlation_ratio_bound(count, s1, s2, a1):
    """The header's bounds carried through inspection.correlation_ratio, to first order.  With
    N = sum m_b, S1 = sum s1_b, S2 = sum s2_b, num = sum m_b (s1_b / m_b - S1 / N)^2 and
    den = S2 - S1^2 / N: every s1_b moves by at most B1_b and S1 by sum B1_b, so each deviation
    dev_b by at most B1_b / m_b + sum B1 / N and num by 2 sum m_b |dev_b| of that; den moves by
    sum B2_b + 2 |S1 / N| sum B1_b.  The host arithmetic adds roundings of relative size u: at most
    (nb + 6) of them on num's terms (nb bins summed) and on den's, (nb + 4) u (S2 + S1^2 / N).
    eta^2 = num / den then moves by (d num + eta^2 d den) / den, and one more rounding."""
    m = np.asarray(count, dtype=np.float64)
    has = m > 0
    m, s1, s2, a1 = m[has], np.asarray(s1)[has], np.asarray(s2)[has], np.asarray(a1)[has]
    b1, b2 = sum_bounds(m, s2, a1)
    N, S1, S2, nb = m.sum(), s1.sum(), s2.sum(), len(m)
    dev = s1 / m - S1 / N
    num = float((m * dev * dev).sum())
    den = S2 - S1 * S1 / N
    d_dev = b1 / m + b1.sum() / N + 3 * U * (np.abs(s1 / m) + abs(S1 / N))
    d_num = float((2 * m * np.abs(dev) * d_dev).sum()) + (nb + 6) * U * num
    d_den = b2.sum() + 2 * abs(S1 / N) * b1.sum() + (nb + 4) * U * (S2 + S1 * S1 / N)
    eta = num / den
    return (d_num + eta * d_den) / den + U * eta
