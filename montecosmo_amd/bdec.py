"""Bayesian decision utilities (montecosmo/bdec.py): quantiles and credible intervals of draws, on the HIP path for chains.

    q = bdec.quantile(x, [.05, .5, .95], axis=(0, 1))      # x: (C, N, *dims) -> float64 (3, *dims)
    ci = bdec.credint(x, .95, axis=(0, 1))                 # smallest interval -> (*dims, 2)
    ch.credint(), ch.quantile(.5), ch.coverage(truth)      # the same per entry of a chains.Chains

`axis` is one axis or a tuple of axes whose draws are pooled; axis=(0, 1) pools chains and draws of a (C, N, *dims) array, and is what the
device reads in place.  Outputs are float64 numpy arrays: (*p.shape, *out_shape) for `quantile`, with a trailing axis of 2 (low, high) for
the intervals.  `qbcs` and `scs` (a stub in the reference) are not built.

Order.  The n pooled draws of a dimension are put in the IEEE total order of their values, x_(0) <= .. <= x_(n-1): -inf first, -0 before
+0, +inf before NaN, every NaN alike and last.

quantile, unweighted, ord = 1 (the reference's interpolation of the empirical cdf, restated):
    cdf_k = (k + 1) / n                                         a float64 division
    i = clip(first k with cdf_k >= p, 1, n - 1)                 found on the host: the two ranks i - 1, i depend on (p, n) only
    q = x_(i-1) + (p - cdf_(i-1)) (x_(i) - x_(i-1)) / (cdf_i - cdf_(i-1)),  then clipped to [x_(i-1), x_(i)]
  all in float64, the product before the quotient; n = 1 returns the value.  A dimension that holds NaNs has them at its upper ranks.
quantile with weights w (ord = 1): cdf = cumsum(w sorted with x) / its last value, i as above on that cdf, the slope formed first:
    q = x_(i-1) + (p - cdf_(i-1)) safe_div(x_(i) - x_(i-1), cdf_i - cdf_(i-1)), clipped;        safe_div(a, 0) = 0.
  Without weights the weights are ones.
quantile, ord = 2 (the density w at x, integrated by trapezes): cdf_0 = 0, cdf_k = sum_{t < k} (x_(t+1) - x_(t)) (w_t + w_(t+1)) / 2; w and cdf
  are divided by cdf_(n-1); i as above; with alpha = safe_div(w_i - w_(i-1), x_(i) - x_(i-1)), dp = p - cdf_(i-1) and
  disc = max(w_(i-1)^2 + 2 alpha dp, 0):  q = x_(i-1) + (safe_div(dp, w_(i-1)) if alpha = 0 else safe_div(sqrt(disc) - w_(i-1), alpha)), clipped.
qbci(p, type): (quantile(p_low), quantile(p_low + p)) with p_low = 0, (1 - p) / 2, 1 - p for 'low', 'med', 'high'.
sci_noweights(p), p a scalar: L = min(int(rint(p n)), n - 1), rounding half to even; the interval is (x_(i), x_(i+L)) for the first i in
  0 .. n - L - 1 that minimises x_(i+L) - x_(i), the difference taken in float64 (of the float32 values on the device); a length that is
  NaN (both ends the same infinity) counts as +inf.  A dimension that holds a NaN gives (NaN, NaN): the reference's argmin over NaN
  lengths is an accident, not a definition.
sci(p), weighted: with the normalised cdf of `quantile` (either order), every k offers the interval from (x_(k) if cdf_k <= 1 - p else x_(0))
  to quantile(cdf_k + p); the first k of the smallest length is taken.
argmedian(a, axis): the index of the median along `axis`, the upper one of the two for an even length.
rank_counts(x, truth): the number of pooled draws below, and equal to, truth (IEEE comparisons), int32: what a rank histogram is made of.
  The device compares float32 draws with truth rounded to float32, the host float64 with float64.

backend 'hip': float32 draws, unweighted, ord = 1, through `mcpm_bdec_sort_f32` (csrc/bdec.hip): every dimension's pooled draws are sorted in
LDS and only the order statistics that were asked for come back (the values at the few ranks, the smallest window and its index, the
counts against a truth).  The float64 interpolation above is then a handful of torch float64 operations on [ranks, D] tensors.  A CUDA tensor
(C, N, *dims) whose trailing axes are contiguous is read in place whatever its chain and draw strides are; a host float32 array is uploaded
in pieces of at most `metrics.CHUNK_BYTES` (chains._chunks).  No tensor of the size of the draws is made beside them.  More than LDS_MAX_M
pooled draws per dimension do not fit the LDS tile: such chains take the GENERAL path, torch.sort of the same integer keys on a transposed
copy of as many dimensions at a time as keep its working set under `metrics.CHUNK_BYTES`, with bitwise the same outputs.  Other pooled axes
than the leading ones are moved to the front first, which copies a device tensor.
backend 'host': everything above in numpy float64, weights, ord = 2 and the weighted `sci` included: the slow complete path.  'auto': 'hip'
when a GPU is present, the draws are float32, there are no weights and ord = 1 (chains._backend), else 'host'; 'hip' with weights or
ord = 2 raises TypeError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, chains

__all__ = ["quantile", "qbci", "sci_noweights", "sci", "credint", "argmedian", "rank_counts", "sort_draws"]

LDS_MAX_M = 32768      # pooled draws per dimension the LDS tile of csrc/bdec.hip holds (MCPM_BDEC_MAX_M); above it: the general path
MAX_RANKS = 64         # ranks per call (MCPM_BDEC_MAX_RANKS); more go in several calls
GENERAL_BYTES_PER_DRAW = 64      # working set of the general path per pooled draw: the copy, the keys, torch.sort's values, indices and scratch


# ------------------------------------------------------------------------------------------------
# arguments
def _as_array(x):
    if isinstance(x, torch.Tensor):
        return x if x.ndim else x[None]
    return np.atleast_1d(np.asarray(x))


def _axis_tuple(ndim, axis):
    ax = (axis,) if isinstance(axis, (int, np.integer)) else tuple(axis)
    if not ax or any(not -ndim <= a < ndim for a in ax):
        raise ValueError(f"axis {axis!r} does not fit {ndim} axes")
    ax = tuple(int(a) % ndim for a in ax)
    if len(set(ax)) != len(ax):
        raise ValueError(f"axis {axis!r} names an axis twice")
    return ax


def _pooled_front(x, ax):
    """x as (C, N, *out_shape): the pooled axes `ax` in front, one of them as C = 1 chain, more than two with the later ones merged."""
    k = len(ax)
    if ax != tuple(range(k)):
        x = torch.movedim(x, ax, tuple(range(k))) if isinstance(x, torch.Tensor) else np.moveaxis(x, ax, tuple(range(k)))
    if k == 1:
        x = x[None]
    elif k > 2:
        x = x.reshape((x.shape[0], -1) + tuple(x.shape[k:]))
    return x


def _weights(w, shape, ax):
    """Weights broadcast to the draws: a vector goes along a single pooled axis, an array of the pooled shape along leading pooled axes."""
    w = np.asarray(_np(w), dtype=np.float64)
    if w.ndim <= 1 and len(ax) == 1:
        w = w.reshape(w.shape + (1,) * (len(shape) - ax[0] - w.ndim))
    elif ax == tuple(range(len(ax))) and w.shape == tuple(shape[:len(ax)]):
        w = w.reshape(w.shape + (1,) * (len(shape) - len(ax)))
    return np.broadcast_to(w, tuple(shape))


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t


def _backend(x, backend, weights=None, ord=1):
    if ord not in (1, 2):
        raise NotImplementedError("only ord = 1 and ord = 2 are implemented")
    if weights is not None or ord != 1:
        if backend == "hip":
            raise TypeError("backend 'hip' takes unweighted draws and ord = 1; use backend 'host' (or 'auto')")
        if backend == "auto":
            return "host"
    return chains._backend(x, backend)


def _prepare(x, axis):
    """(x as (C, N, *out_shape), the pooled axes, out_shape)."""
    x = _as_array(x)
    ax = _axis_tuple(x.ndim, axis)
    x3 = chains._check(_pooled_front(x, ax), 1, "draws")
    return x3, ax, tuple(x3.shape[2:])


def _ranks(p, n):
    """i = clip(first k with (k + 1) / n >= p, 1, n - 1) for every p (n >= 2)."""
    cdf = np.arange(1, n + 1) / n
    return np.clip(np.searchsorted(cdf, p, side="left"), 1, n - 1)


def _sci_length(p, n):
    if np.ndim(p) != 0:
        raise TypeError("sci_noweights takes a scalar p, as the reference does")
    return min(int(np.rint(float(p) * n)), n - 1)


# ------------------------------------------------------------------------------------------------
# host side: numpy float64
def _safe_div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        zero = b == 0
        return np.where(zero, 0., a / np.where(zero, 1., b))


def _sort64(a, order=False):
    """float64 columns sorted along axis 0 in the IEEE total order, every NaN last; with `order` also the permutation."""
    u = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    u = np.where(np.isnan(a), np.int64(0x7ff8000000000000), u)
    key = u ^ ((u >> 63) & np.int64(0x7fffffffffffffff))      # signed order of the keys = total order of the values
    if order:
        perm = np.argsort(key, axis=0, kind="stable")
        key = np.take_along_axis(key, perm, 0)
    else:
        perm = None
        key = np.sort(key, axis=0)
    val = (key ^ ((key >> 63) & np.int64(0x7fffffffffffffff))).view(np.float64)
    return (val, perm) if order else val


def _host_pooled(x3):
    """Pooled float64 columns (C N, d) of the draws, a piece of the dimensions at a time."""
    for a in chains._host_chunks(x3):
        yield a.reshape(a.shape[0] * a.shape[1], -1)


def _interp(lo, hi, p, cdf_lo, cdf_hi):
    with np.errstate(invalid="ignore", over="ignore"):
        q = lo + (p - cdf_lo) * (hi - lo) / (cdf_hi - cdf_lo)
        return np.minimum(np.maximum(q, lo), hi)


def _host_quantile_plain(xs, p):
    """Unweighted ord = 1 quantiles (P, d) of sorted columns xs (n, d)."""
    n = xs.shape[0]
    if n == 1:
        return np.broadcast_to(xs[0], (len(p), xs.shape[1])).copy()
    i = _ranks(p, n)
    return _interp(xs[i - 1], xs[i], p[:, None], (i / n)[:, None], ((i + 1) / n)[:, None])


def _cdf_1d(xs, ws, ord):
    """(normalised cdf, weights as the interpolation uses them) of one sorted column."""
    if ord == 1:
        cdf = np.cumsum(ws)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            cdf = np.concatenate([[0.], np.cumsum(np.diff(xs) * (ws[1:] + ws[:-1]) / 2.)])
        ws = _safe_div(ws, cdf[-1])      # the integral is not the sum of the weights: they are renormalised with it
    return _safe_div(cdf, cdf[-1]), ws


def _quantile_1d(xs, ws, p, ord):
    """Weighted quantiles of one sorted column at probabilities p (any shape)."""
    n = len(xs)
    if n == 1:
        return np.full(np.shape(p), xs[0])
    cdf, ws = _cdf_1d(xs, ws, ord)
    i = np.clip(np.searchsorted(cdf, p, side="left"), 1, n - 1)
    lo, hi, cdf_lo = xs[i - 1], xs[i], cdf[i - 1]
    with np.errstate(invalid="ignore", over="ignore"):
        if ord == 1:
            q = lo + (p - cdf_lo) * _safe_div(hi - lo, cdf[i] - cdf_lo)
        else:
            w_lo, w_hi = ws[i - 1], ws[i]
            alpha = _safe_div(w_hi - w_lo, hi - lo)
            dp = p - cdf_lo
            disc = np.maximum(w_lo ** 2 + 2. * alpha * dp, 0.)      # rounding and the two ends
            q = lo + np.where(alpha == 0, _safe_div(dp, w_lo), _safe_div(-w_lo + disc ** .5, alpha))
        return np.minimum(np.maximum(q, lo), hi)


def _host_weighted(x3, weights, ax, shape):
    """Sorted pooled columns and their weights, (n, D) each."""
    w3 = _pooled_front(_weights(weights, shape, ax), ax)
    xs = chains._host64(x3).reshape(x3.shape[0] * x3.shape[1], -1)
    ws = np.ascontiguousarray(w3, dtype=np.float64).reshape(xs.shape)
    xs, perm = _sort64(xs, order=True)
    return xs, np.take_along_axis(ws, perm, 0)


def _host_sci_noweights(xs, L):
    """(low, high, index) of the smallest window of L + 1 order statistics of sorted columns xs (n, d)."""
    n = xs.shape[0]
    with np.errstate(invalid="ignore"):
        lens = xs[L:] - xs[:n - L]
    lens = np.where(np.isnan(lens), np.inf, lens)
    i = np.argmin(lens, axis=0)
    lo, hi = np.take_along_axis(xs, i[None], 0)[0], np.take_along_axis(xs, (i + L)[None], 0)[0]
    bad = np.isnan(xs[n - 1])
    return np.where(bad, np.nan, lo), np.where(bad, np.nan, hi), np.where(bad, -1, i).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# device side
def _dev_lds(r, ranks, L, truth, want_sorted):
    """One resident piece through the kernel: dict of device tensors (rank [R, d], sci [2, d], sci_idx, below, equal [d], sorted [M, d])."""
    m = r.c * r.n
    dev = r.device
    out = {}
    if L is not None:
        out["sci"] = torch.empty((2, r.d), dtype=torch.float32, device=dev)
        out["sci_idx"] = torch.empty(r.d, dtype=torch.int32, device=dev)
    if truth is not None:
        out["below"] = torch.empty(r.d, dtype=torch.int32, device=dev)
        out["equal"] = torch.empty(r.d, dtype=torch.int32, device=dev)
    if want_sorted:
        out["sorted"] = torch.empty((m, r.d), dtype=torch.float32, device=dev)
    ask = list(ranks) if len(ranks) else [0]
    rank = torch.empty((len(ask), r.d), dtype=torch.float32, device=dev)
    for lo in range(0, len(ask), MAX_RANKS):
        batch = ask[lo:lo + MAX_RANKS]
        first = lo == 0      # the options ride on the first call
        _lib.call("mcpm_bdec_sort_f32", chains._stream(dev), r.ptr, 0, r.d, r.c, r.sc, r.n, r.sd, (C.c_int * len(batch))(*batch), len(batch),
                  rank[lo:lo + len(batch)], L if (first and L is not None) else -1, out.get("sci") if first else None,
                  out.get("sci_idx") if first else None, truth if first else None, out.get("below") if first else None,
                  out.get("equal") if first else None, out.get("sorted") if first else None)
    out["rank"] = rank[:len(ranks)]
    return out


def _dev_general(r, ranks, L, truth, want_sorted):
    """The same outputs, bitwise, for any number of pooled draws: torch.sort of the integer keys of a transposed copy, a few dimensions at a time."""
    from . import metrics
    m = r.c * r.n
    v = r.keep.flatten(2) if r.keep.ndim > 2 else r.keep[:, :, None]      # (C, N, d), a view
    per = max(1, int(metrics.CHUNK_BYTES) // (GENERAL_BYTES_PER_DRAW * m))
    idx = torch.as_tensor(list(ranks), dtype=torch.int64, device=r.device)
    parts = []
    for lo in range(0, r.d, per):
        bits = v[:, :, lo:lo + per].reshape(m, -1).t().clone(memory_format=torch.contiguous_format).view(torch.int32)      # [d', M], always a copy
        bits[(bits & 0x7fffffff) > 0x7f800000] = 0x7fc00000                              # every NaN alike
        bits ^= (bits >> 31) & 0x7fffffff                                                 # signed order of the keys = total order of the values
        keys = torch.sort(bits, dim=1).values
        del bits
        keys ^= (keys >> 31) & 0x7fffffff
        vals = keys.view(torch.float32)
        o = {"rank": vals[:, idx].t().contiguous()}
        if L is not None:
            ln = vals[:, L:].double() - vals[:, :m - L].double()
            ln[torch.isnan(ln)] = float("inf")
            i = torch.argmin(ln, dim=1)      # the first of equal minima
            del ln
            bad = torch.isnan(vals[:, m - 1])
            pair = torch.stack([vals.gather(1, i[:, None])[:, 0], vals.gather(1, (i + L)[:, None])[:, 0]])
            pair[:, bad] = float("nan")
            o["sci"] = pair
            o["sci_idx"] = torch.where(bad, -1, i).to(torch.int32)
        if truth is not None:
            t = truth[lo:lo + per, None]
            o["below"] = (vals < t).sum(dim=1, dtype=torch.int32)
            o["equal"] = (vals == t).sum(dim=1, dtype=torch.int32)
        if want_sorted:
            o["sorted"] = vals.t().contiguous()
        del keys, vals
        parts.append(o)
    return {k: torch.cat([p[k] for p in parts], dim=-1) if len(parts) > 1 else parts[0][k] for k in parts[0]}


def _dev_stats(x3, ranks=(), L=None, truth=None, want_sorted=False):
    """Order statistics of the draws x3 (C, N, *dims) on the device, all dimensions flattened last: dict of device tensors."""
    parts, lo = [], 0
    for r in chains._chunks(x3):
        t = None
        if truth is not None:
            t = torch.from_numpy(np.ascontiguousarray(truth[lo:lo + r.d])).to(r.device)
        fn = _dev_lds if r.c * r.n <= LDS_MAX_M else _dev_general
        parts.append(fn(r, ranks, L, t, want_sorted))
        lo += r.d
    return {k: torch.cat([p[k] for p in parts], dim=-1) if len(parts) > 1 else parts[0][k] for k in parts[0]}


def _flat_truth(truth, dims):
    t = np.asarray(_np(truth)).astype(np.float32, copy=False)      # (the device compares float32 with float32)
    if t.shape != tuple(dims):
        raise ValueError(f"truth must have shape {tuple(dims)}, got {t.shape}")
    return t.reshape(-1)


def _dev_quantile(x3, p):
    """Unweighted ord = 1 quantiles (P, D) float64 numpy of the draws at the probabilities p (P,)."""
    n = x3.shape[0] * x3.shape[1]
    if n == 1:
        v = _dev_stats(x3, ranks=[0])["rank"][0].double()
        return np.broadcast_to(_np(v), (len(p), v.shape[0])).copy()
    i = _ranks(p, n)
    uniq, inv = np.unique(np.concatenate([i - 1, i]), return_inverse=True)
    rank = _dev_stats(x3, ranks=[int(u) for u in uniq])["rank"]
    dev = rank.device
    inv = torch.as_tensor(inv.reshape(2, -1), device=dev)
    lo, hi = rank[inv[0]].double(), rank[inv[1]].double()
    col = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)[:, None]
    q = lo + (col(p) - col(i / n)) * (hi - lo) / (col((i + 1) / n) - col(i / n))
    return _np(torch.minimum(torch.maximum(q, lo), hi))


# ------------------------------------------------------------------------------------------------
# public functions
def quantile(x, p, axis=0, weights=None, ord=1, backend="auto"):
    """Quantiles of the draws pooled along `axis` at the probabilities p: float64 (*p.shape, *out_shape)."""
    p = np.asarray(p, dtype=np.float64)
    pf = p.reshape(-1)
    x3, ax, dims = _prepare(x, axis)
    be = _backend(x3, backend, weights, ord)
    if be == "hip":
        q = _dev_quantile(x3, pf)
    elif weights is None and ord == 1:
        q = np.concatenate([_host_quantile_plain(_sort64(a), pf) for a in _host_pooled(x3)], axis=1)
    else:
        xs, ws = _host_weighted(x3, np.ones(()) if weights is None else weights, ax, _as_array(x).shape)
        q = np.stack([_quantile_1d(xs[:, j], ws[:, j], pf, ord) for j in range(xs.shape[1])], axis=1)
    return q.reshape(p.shape + dims)


def qbci(x, p=.95, axis=0, weights=None, type="med", ord=1, backend="auto"):
    """Quantile-based credible interval of probability p: the lowest ('low'), the equal-tailed ('med') or the highest ('high')."""
    p = np.asarray(p, dtype=np.float64)
    if type == "low":
        p_low = np.zeros_like(p)
    elif type == "med":
        p_low = (1. - p) / 2.
    elif type == "high":
        p_low = 1. - p
    else:
        raise ValueError(f"type must be 'low', 'med' or 'high', not {type!r}")
    q = quantile(x, np.stack([p_low, p_low + p]), axis, weights, ord, backend)      # one sort for both ends
    return np.stack([q[0], q[1]], axis=-1)


def sci_noweights(x, p=.95, axis=0, backend="auto", return_index=False):
    """Smallest credible interval of the unweighted draws, p a scalar: float64 (*out_shape, 2); with return_index also the rank i of its
    lower end, int32 (-1 where the dimension holds a NaN)."""
    x3, ax, dims = _prepare(x, axis)
    L = _sci_length(p, x3.shape[0] * x3.shape[1])
    if _backend(x3, backend) == "hip":
        st = _dev_stats(x3, L=L)
        pair, idx = _np(st["sci"].double()), _np(st["sci_idx"])
    else:
        parts = [_host_sci_noweights(_sort64(a), L) for a in _host_pooled(x3)]
        pair = np.stack([np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])])
        idx = np.concatenate([q[2] for q in parts])
    ci = np.stack([pair[0], pair[1]], axis=-1).reshape(dims + (2,))
    return (ci, idx.reshape(dims)) if return_index else ci


def sci(x, p=.95, axis=0, weights=None, ord=1, backend="auto"):
    """Smallest credible interval from the interpolated weighted cdf: float64 (*p.shape, *out_shape, 2).  Host only."""
    if backend not in ("auto", "hip", "host"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'host', not {backend!r}")
    if backend == "hip":
        raise TypeError("sci is the weighted algorithm and runs on the host; sci_noweights has the device path")
    if ord not in (1, 2):
        raise NotImplementedError("only ord = 1 and ord = 2 are implemented")
    p = np.asarray(p, dtype=np.float64)
    pf = p.reshape(-1)
    x3, ax, dims = _prepare(x, axis)
    xs, ws = _host_weighted(x3, np.ones(()) if weights is None else weights, ax, _as_array(x).shape)
    out = np.empty((len(pf), xs.shape[1], 2))
    for j in range(xs.shape[1]):
        cdf, wj = _cdf_1d(xs[:, j], ws[:, j], ord)
        for k, pk in enumerate(pf):
            lows = np.where(cdf <= 1. - pk, xs[:, j], xs[0, j])
            highs = _quantile_1d(xs[:, j], wj, cdf + pk, ord)
            with np.errstate(invalid="ignore"):
                i = np.argmin(highs - lows)
            out[k, j] = lows[i], highs[i]
    return out.reshape(p.shape + dims + (2,))


def credint(x, p=.95, axis=0, weights=None, type="small", ord=1, backend="auto"):
    """Credible interval of probability p: the smallest ('small'), or the quantile-based 'low', 'med', 'high'."""
    _backend(_as_array(x), backend, weights, ord)      # ('hip' with weights or ord = 2: TypeError, whatever the type)
    if type == "small":
        if weights is None:
            return sci_noweights(x, p, axis, backend)      # (no order enters it)
        return sci(x, p, axis, weights, ord, "host")
    return qbci(x, p, axis, weights, type, ord, backend)


def argmedian(a, axis=-1):
    """Indices of the median along `axis` (None: of the flattened array); the upper of the two candidates for an even length."""
    a = np.asarray(_np(a))
    if axis is None:
        a, axis = a.reshape(-1), 0
    k = a.shape[axis] // 2
    return np.argpartition(a, k, axis).take(k, axis)


def rank_counts(x, truth, axis=0, backend="auto"):
    """(below, equal): per dimension the number of pooled draws x < truth and x == truth, int32 arrays of out_shape."""
    x3, ax, dims = _prepare(x, axis)
    if _backend(x3, backend) == "hip":
        st = _dev_stats(x3, truth=_flat_truth(truth, dims))
        below, equal = _np(st["below"]), _np(st["equal"])
    else:
        t = np.asarray(_np(truth), dtype=np.float64).reshape(-1)
        if t.size != int(np.prod(dims, dtype=np.int64)):
            raise ValueError(f"truth must have shape {dims}")
        parts, lo = [], 0
        for a in _host_pooled(x3):
            tt = t[lo:lo + a.shape[1]]
            parts.append(((a < tt).sum(axis=0), (a == tt).sum(axis=0)))
            lo += a.shape[1]
        below, equal = (np.concatenate([q[i] for q in parts]).astype(np.int32) for i in (0, 1))
    return below.reshape(dims), equal.reshape(dims)


def sort_draws(x, axis=0, backend="auto"):
    """The pooled draws of every dimension in order: float64 (n, *out_shape).  For scalar chains and tests: it is as large as the draws."""
    x3, ax, dims = _prepare(x, axis)
    if _backend(x3, backend) == "hip":
        s = _np(_dev_stats(x3, want_sorted=True)["sorted"]).astype(np.float64)
    else:
        s = np.concatenate([_sort64(a) for a in _host_pooled(x3)], axis=1)
    return s.reshape((s.shape[0],) + dims)
