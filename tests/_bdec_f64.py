"""Float64 numpy restatement of the order statistics of montecosmo_amd/bdec.py (montecosmo/bdec.py: quantile, qbci, sci_noweights, sci), for
its tests.  Nothing is imported from the package; every function takes pooled draws a[n, D] (one column per dimension).

Order: the IEEE total order of the values through unsigned 64-bit keys (negative values have every bit flipped, the others the sign bit
set; every NaN becomes the quiet NaN first), sorted by np.sort: -inf .. -0 +0 .. +inf NaN.
quantile (unweighted, ord 1): cdf_k = (k + 1) / n; i = clip(first k with cdf_k >= p, 1, n - 1), found by a loop;
    q = clip(x_(i-1) + (p - cdf_(i-1)) (x_(i) - x_(i-1)) / (cdf_i - cdf_(i-1)), x_(i-1), x_(i)); n = 1: the value.
sci_noweights: L = min(int(rint(p n)), n - 1); plain loop over i = 0 .. n - L - 1 for the first smallest x_(i+L) - x_(i), a NaN length as
    +inf; a column with a NaN gives NaN, NaN, -1.
quantile_weighted / sci_weighted: the reference's algorithms for weights and ord = 2, one column and one probability at a time.
"""
import math

import numpy as np

_SIGN = np.uint64(1 << 63)


def sort_total(a):
    a = np.array(a, dtype=np.float64, ndmin=2)
    bits = a.view(np.uint64).copy()
    bits[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    keys = np.where(bits & _SIGN != 0, ~bits, bits | _SIGN)
    keys = np.sort(keys, axis=0)
    back = np.where(keys & _SIGN != 0, keys & ~_SIGN, ~keys)
    return back.view(np.float64)


def rank_high(p, n):
    i = n
    for k in range(n):
        if (k + 1) / n >= p:
            i = k
            break
    return min(max(i, 1), n - 1)


def quantile(a, p):
    """(*p.shape, D)"""
    xs = sort_total(a)
    n, d = xs.shape
    p = np.asarray(p, dtype=np.float64)
    out = np.empty((p.size, d))
    for j, pj in enumerate(p.reshape(-1)):
        if n == 1:
            out[j] = xs[0]
            continue
        i = rank_high(pj, n)
        lo, hi = xs[i - 1], xs[i]
        with np.errstate(all="ignore"):
            q = lo + (pj - i / n) * (hi - lo) / ((i + 1) / n - i / n)
            out[j] = np.minimum(np.maximum(q, lo), hi)
    return out.reshape(p.shape + (d,))


def qbci(a, p, type):
    p = np.asarray(p, dtype=np.float64)
    p_low = {"low": 0. * p, "med": (1. - p) / 2., "high": 1. - p}[type]
    return np.stack([quantile(a, p_low), quantile(a, p_low + p)], axis=-1)


def sci_length(p, n):
    return min(int(np.rint(p * n)), n - 1)


def sci_noweights(a, p):
    """(low[D], high[D], index[D])"""
    xs = sort_total(a)
    n, d = xs.shape
    L = sci_length(p, n)
    low, high, idx = np.empty(d), np.empty(d), np.empty(d, dtype=np.int32)
    for c in range(d):
        col = xs[:, c]
        if math.isnan(col[n - 1]):
            low[c], high[c], idx[c] = np.nan, np.nan, -1
            continue
        best, best_i = None, 0
        for i in range(n - L):
            with np.errstate(all="ignore"):
                ln = col[i + L] - col[i]
            if math.isnan(ln):
                ln = math.inf
            if best is None or ln < best:
                best, best_i = ln, i
        low[c], high[c], idx[c] = col[best_i], col[best_i + L], best_i
    return low, high, idx


def counts(a, truth):
    a = np.asarray(a, dtype=np.float64)
    t = np.asarray(truth, dtype=np.float64).reshape(1, -1)
    return (a < t).sum(axis=0).astype(np.int32), (a == t).sum(axis=0).astype(np.int32)


def coverage(a, truth, p):
    low, high, _ = sci_noweights(a, p)
    t = np.asarray(truth, dtype=np.float64).reshape(-1)
    return float(np.mean((low <= t) & (t <= high)))


# ---- the weighted algorithms, one column at a time ---------------------------------------------------------------------------------
def _div0(a, b):
    return 0. if b == 0 else a / b


def _column_cdf(x, w, ord):
    """x sorted with its weights; returns (cdf normalised, weights as the interpolation uses them)."""
    n = len(x)
    cdf = np.zeros(n)
    if ord == 1:
        s = 0.
        for k in range(n):
            s += w[k]
            cdf[k] = s
    else:
        for k in range(1, n):
            cdf[k] = cdf[k - 1] + (x[k] - x[k - 1]) * (w[k] + w[k - 1]) / 2.
        w = np.array([_div0(v, cdf[-1]) for v in w])
    total = cdf[-1]
    return np.array([_div0(v, total) for v in cdf]), w


def _column_quantile(x, w, p, ord):
    n = len(x)
    if n == 1:
        return x[0]
    cdf, w = _column_cdf(x, w, ord)
    i = n
    for k in range(n):
        if cdf[k] >= p:
            i = k
            break
    i = min(max(i, 1), n - 1)
    lo, hi = x[i - 1], x[i]
    if ord == 1:
        q = lo + (p - cdf[i - 1]) * _div0(hi - lo, cdf[i] - cdf[i - 1])
    else:
        alpha = _div0(w[i] - w[i - 1], hi - lo)
        dp = p - cdf[i - 1]
        disc = max(w[i - 1] ** 2 + 2. * alpha * dp, 0.)
        q = lo + (_div0(dp, w[i - 1]) if alpha == 0 else _div0(-w[i - 1] + math.sqrt(disc), alpha))
    return min(max(q, lo), hi)


def _sorted_with_weights(a, w):
    a = np.array(a, dtype=np.float64, ndmin=2)
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), a.shape)
    order = np.argsort(a, axis=0, kind="stable")
    return np.take_along_axis(a, order, 0), np.take_along_axis(w, order, 0)


def quantile_weighted(a, w, p, ord=1):
    """(*p.shape, D); w broadcasts to a."""
    xs, ws = _sorted_with_weights(a, w)
    p = np.asarray(p, dtype=np.float64)
    out = np.array([[_column_quantile(xs[:, c], ws[:, c], pj, ord) for c in range(xs.shape[1])] for pj in p.reshape(-1)])
    return out.reshape(p.shape + (xs.shape[1],))


def sci_weighted(a, w, p, ord=1):
    """(*p.shape, D, 2)"""
    xs, ws = _sorted_with_weights(a, w)
    n, d = xs.shape
    p = np.asarray(p, dtype=np.float64)
    out = np.empty((p.size, d, 2))
    for c in range(d):
        x = xs[:, c]
        cdf, wn = _column_cdf(x, ws[:, c], ord)
        for j, pj in enumerate(p.reshape(-1)):
            best, pair = None, None
            for k in range(n):
                lo = x[k] if cdf[k] <= 1. - pj else x[0]
                hi = _column_quantile(x, wn, cdf[k] + pj, ord)
                if best is None or hi - lo < best:
                    best, pair = hi - lo, (lo, hi)
            out[j, c] = pair
    return out.reshape(p.shape + (d, 2))
