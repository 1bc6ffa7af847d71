"""Chain diagnostics (montecosmo/chains.py:342-536, montecosmo/metrics.py:562-579): effective sample size, R-hat and moments of every
sampled dimension, the field included, on the HIP path.

    ess = chains.effective_sample_size(x)            # x: (C, N, *dims) -> float64 array of shape dims
    rhat = chains.split_gelman_rubin(x)
    ch = chains.Chains.load_runs(paths, 1, 10, layout=flat.layout())
    ch.eval_per_ess(), ch.summary()

The formulas are numpyro.diagnostics' (effective_sample_size, gelman_rubin, split_gelman_rubin), restated.  For x[c, t, ...] with C
chains and N draws every trailing index is an independent dimension:
    m_c = mean_t x,  v_c = sum_t (x - m_c)^2 / (N - 1),  W = mean_c v_c,  V = W (N - 1) / N + var_c(m_c, ddof=1)   (C = 1: W = V)
    gelman_rubin = sqrt(V / W);  split_gelman_rubin: the same of the 2 C halves x[:, :h], x[:, -h:], h = N // 2
    gamma_c(k) = sum_{t < N - k} (x_t - m_c)(x_{t+k} - m_c) / N   (bias=False: / (N - k)),  rho_k = 1 - (W - mean_c gamma_c(k)) / V,  rho_0 = 1
    P_j = rho_2j + rho_2j+1 (j < N_even / 2);  tau = -1 + 2 (P_0 + sum_{j >= 1} cummin_j max(P_j, 0));  ess = C N / tau
A constant dimension gives NaN (0 / 0), and ess may be negative or huge at tiny N: that is the formula.

backend 'hip': float32 draws through `mcpm_chain_moments_f32` / `mcpm_chain_tau_f32` (csrc/chains.hip), everything in float64 from the
float32 input, one lane per dimension in a fixed order: bitwise reproducible, and a dimension's result does not depend on the others.  A
CUDA tensor whose trailing axes are contiguous is read in place whatever its chain and draw strides are (a slice of flat states serves); a
host float32 array is uploaded along the flattened dimension axis in chunks of at most `metrics.CHUNK_BYTES`, which changes no bit.
backend 'host': the same formulas in numpy float64 (float64 scalar chains, machines without a GPU).  'auto': 'hip' when a GPU is
present and the draws are float32, else 'host'.  Outputs are float64 numpy arrays of shape dims; `multi_ess` / `multi_gr` reduce where
the per-dimension values are and copy back only the reduced ones.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib, nbody

__all__ = ["effective_sample_size", "autocorr_time", "gelman_rubin", "split_gelman_rubin", "chain_moments", "segment_moments",
           "multi_ess", "multi_gr", "quantile", "credint", "harmean", "geomean", "Chains"]

HOST_CHUNK_BYTES = 1 << 28      # float64 working set of one host chunk


# ------------------------------------------------------------------------------------------------
# reductions (montecosmo/metrics.py:562-579)
def harmean(a, axis=None):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1. / np.mean(1. / a, axis=axis)


def geomean(a, axis=None):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(np.mean(np.log(a), axis=axis))


# ------------------------------------------------------------------------------------------------
# arguments
def _check(x, min_draws=2, what="chains"):
    """x as it came (numpy array or tensor), checked: (C, N, *dims) with N >= min_draws."""
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x)
    if x.ndim < 2:
        raise ValueError(f"{what} must have shape (chains, draws, *dims), got {tuple(x.shape)}")
    if x.shape[1] < min_draws:
        raise ValueError(f"{what} need at least {min_draws} draws, got {x.shape[1]}")
    if x.shape[0] < 1 or any(s < 1 for s in x.shape[2:]):
        raise ValueError(f"{what} have an empty axis: shape {tuple(x.shape)}")
    return x


def _is_f32(x):
    return x.dtype == (torch.float32 if isinstance(x, torch.Tensor) else np.float32)


def _backend(x, backend):
    if backend == "auto":
        return "hip" if (_is_f32(x) and torch.cuda.is_available()) else "host"
    if backend == "hip":
        if not _is_f32(x):
            raise TypeError(f"backend 'hip' takes float32 draws, got {x.dtype}; use backend 'host' (or 'auto')")
        return backend
    if backend == "host":
        return backend
    raise ValueError(f"backend must be 'auto', 'hip' or 'host', not {backend!r}")


def _host64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------
# device side
class _Resident:
    """Float32 draws on the device seen as (C, N, D): pointer, strides in elements, and the tensor that keeps them alive."""

    def __init__(self, t):
        c, n = int(t.shape[0]), int(t.shape[1])
        d = int(np.prod(t.shape[2:], dtype=np.int64))
        inner = t[0, 0]
        if not (inner.is_contiguous() and t.stride(0) >= 0 and t.stride(1) >= 0 and (t.stride(1) >= d or n == 1)):
            t = t.contiguous()
        self.keep, self.c, self.n, self.d = t, c, n, d
        self.sc, self.sd = int(t.stride(0)), int(t.stride(1))
        self.ptr = C.c_void_p(t.data_ptr())
        self.device = t.device


def _chunks(x):
    """The draws as _Resident pieces along the flattened dimension axis: a CUDA tensor in one piece, in place; host float32 data in
    uploads of at most metrics.CHUNK_BYTES."""
    from . import metrics      # (imports this module for its re-exports)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        yield _Resident(x.detach())
        return
    dev = nbody._device()
    a = x.detach().numpy() if isinstance(x, torch.Tensor) else x
    c, n = a.shape[:2]
    a = a.reshape(c, n, -1)
    d = a.shape[2]
    per = max(1, int(metrics.CHUNK_BYTES) // (4 * c * n))
    for lo in range(0, d, per):
        yield _Resident(torch.from_numpy(np.ascontiguousarray(a[:, :, lo:lo + per])).to(dev))


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _dev_moments(r, n_part=1, part_draws=None, first_draw=0, part_step=None):
    """(mean, m2) float64 device tensors [C n_part, D] of the segments (c, p): draws first_draw + p part_step + [0, part_draws) of chain c."""
    n = r.n if part_draws is None else int(part_draws)
    step = n if part_step is None else int(part_step)
    if not (n >= 1 and n_part >= 1 and first_draw >= 0 and step >= 0 and first_draw + (n_part - 1) * step + n <= r.n):
        raise ValueError(f"{n_part} segments of {n} draws, {step} apart from draw {first_draw}, do not fit in {r.n} draws")
    mean = torch.empty((r.c * n_part, r.d), dtype=torch.float64, device=r.device)
    m2 = torch.empty_like(mean)
    _lib.call("mcpm_chain_moments_f32", _stream(r.device), r.ptr, first_draw * r.sd, r.d, r.c, r.sc, n_part, step * r.sd, n, r.sd, mean, m2)
    return mean, m2


def _dev_split_moments(r):
    """Moments of the 2 C halves, segment 2 c + p = half p of chain c: the middle draw of an odd N is in neither."""
    h = r.n // 2
    return _dev_moments(r, 2, h, 0, r.n - h)


def _dev_tau(r, mean, m2, bias):
    tau = torch.empty(r.d, dtype=torch.float64, device=r.device)
    lags = torch.empty(r.d, dtype=torch.int32, device=r.device)
    _lib.call("mcpm_chain_tau_f32", _stream(r.device), r.ptr, 0, r.d, r.c, r.sc, 1, 0, r.n, r.sd, mean, m2, int(bool(bias)), tau, lags)
    return tau, lags


def _dev_rhat(mean, m2, n):
    """sqrt(V / W) from the segments' moments: a handful of float64 operations on [S, D] tensors."""
    s = mean.shape[0]
    w = (m2 / (n - 1)).mean(dim=0)
    v = w * (n - 1) / n
    if s > 1:
        v = v + mean.var(dim=0, unbiased=True)
    else:
        w = v
    return torch.sqrt(v / w)


def _dev_per_dim(x, fn):
    """fn(resident) -> tuple of [.., D] device tensors, over the chunks; the tuple of device tensors joined along the last axis."""
    parts = [fn(r) for r in _chunks(x)]
    return tuple(torch.cat([p[i] for p in parts], dim=-1) if len(parts) > 1 else parts[0][i] for i in range(len(parts[0])))


# ------------------------------------------------------------------------------------------------
# host side: the same formulas in numpy float64; the autocovariance by a zero-padded FFT of a power-of-two length
def _host_chunks(x):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
    c, n = a.shape[:2]
    a = a.reshape(c, n, -1)
    per = max(1, HOST_CHUNK_BYTES // (8 * 4 * c * n))
    for lo in range(0, a.shape[2], per):
        yield np.asarray(a[:, :, lo:lo + per], dtype=np.float64)


def _host_wv(mean, m2, n):
    w = np.mean(m2 / (n - 1), axis=0)
    v = w * (n - 1) / n
    if mean.shape[0] > 1:
        v = v + np.var(mean, axis=0, ddof=1)
    else:
        w = v
    return w, v


def _host_moments(a):
    mean = a.mean(axis=1)
    return mean, np.sum((a - mean[:, None]) ** 2, axis=1)


def _host_tau(a, bias):
    c, n = a.shape[:2]
    mean, m2 = _host_moments(a)
    w, v = _host_wv(mean, m2, n)
    size = 1 << int(2 * n - 1).bit_length()
    f = np.fft.rfft(a - mean[:, None], n=size, axis=1)
    s = np.fft.irfft((f * np.conj(f)).real, n=size, axis=1)[:, :n].sum(axis=0)      # [N, D]: sum over the chains of the lag sums
    div = float(n) if bias else (n - np.arange(n, dtype=np.float64))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = 1. - (w - s / div / c) / v
        rho[0] = 1.
        n_even = n - n % 2
        p = rho[:n_even].reshape(n_even // 2, 2, -1).sum(axis=1)
        tail = np.minimum.accumulate(np.maximum(p[1:], 0.), axis=0)
        tau = -1. + 2. * (p[0] + tail.sum(axis=0))
        stop = p[1:] <= 0.
    j_stop = np.where(stop.any(axis=0), stop.argmax(axis=0) + 1, n_even // 2 - 1)
    return tau, np.minimum(2 * (j_stop + 1), n_even).astype(np.int32)


def _split_host(a):
    h = a.shape[1] // 2
    return np.stack([a[:, :h], a[:, a.shape[1] - h:]], axis=1).reshape(2 * a.shape[0], h, -1)      # segment 2 c + p


# ------------------------------------------------------------------------------------------------
# public array functions
def _tau(x, bias, backend):
    """(x checked, tau, lags): device tensors [D] under 'hip', numpy arrays under 'host'."""
    x = _check(x)
    if _backend(x, backend) == "hip":
        def one(r):
            mean, m2 = _dev_moments(r)
            return _dev_tau(r, mean, m2, bias)
        return (x,) + _dev_per_dim(x, one)
    parts = [_host_tau(a, bias) for a in _host_chunks(x)]
    return x, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else t


def autocorr_time(x, bias=True, backend="auto", return_lags=False):
    """tau of every dimension (ess = C N / tau); with return_lags also the number of lags summed, int32."""
    x, tau, lags = _tau(x, bias, backend)
    dims = tuple(x.shape[2:])
    tau = _np(tau).reshape(dims)
    return (tau, _np(lags).reshape(dims)) if return_lags else tau


def effective_sample_size(x, bias=True, backend="auto", return_lags=False):
    """numpyro.diagnostics.effective_sample_size of every dimension; with return_lags also the number of lags summed."""
    x, tau, lags = _tau(x, bias, backend)
    dims = tuple(x.shape[2:])
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = x.shape[0] * x.shape[1] / _np(tau).reshape(dims)
    return (ess, _np(lags).reshape(dims)) if return_lags else ess


def _rhat(x, split, backend):
    """R-hat per flattened dimension where it was made (device tensor or numpy array), and dims."""
    x = _check(x, 4 if split else 2)
    dims = tuple(x.shape[2:])
    if _backend(x, backend) == "hip":
        if split:
            one = lambda r: (_dev_rhat(*_dev_split_moments(r), r.n // 2),)
        else:
            one = lambda r: (_dev_rhat(*_dev_moments(r), r.n),)
        return _dev_per_dim(x, one)[0], dims
    out = []
    for a in _host_chunks(x):
        if split:
            a = _split_host(a)
        w, v = _host_wv(*_host_moments(a), a.shape[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.sqrt(v / w))
    return np.concatenate(out), dims


def gelman_rubin(x, backend="auto"):
    r, dims = _rhat(x, False, backend)
    return _np(r).reshape(dims)


def split_gelman_rubin(x, backend="auto"):
    """R-hat of the 2 C half chains; for an odd N the middle draw belongs to neither half."""
    r, dims = _rhat(x, True, backend)
    return _np(r).reshape(dims)


def segment_moments(x, n_part=1, part_draws=None, first_draw=0, part_step=None, backend="auto"):
    """(mean, m2 = sum (x - mean)^2) float64 [C, n_part, *dims] of the segments (c, p) = draws first_draw + p part_step + [0, part_draws)
    of chain c (part_step defaults to part_draws: consecutive blocks), read in place: one kernel call."""
    x = _check(x, 1)
    n = x.shape[1] if part_draws is None else int(part_draws)
    step = n if part_step is None else int(part_step)
    if not (n >= 1 and n_part >= 1 and first_draw >= 0 and step >= 0 and first_draw + (n_part - 1) * step + n <= x.shape[1]):
        raise ValueError(f"{n_part} segments of {n} draws, {step} apart from draw {first_draw}, do not fit in {x.shape[1]} draws")
    shape = (x.shape[0], n_part) + tuple(x.shape[2:])
    if _backend(x, backend) == "hip":
        mean, m2 = _dev_per_dim(x, lambda r: _dev_moments(r, n_part, n, first_draw, step))
        return _np(mean).reshape(shape), _np(m2).reshape(shape)
    means, m2s = [], []
    for a in _host_chunks(x):
        mm = [_host_moments(a[:, first_draw + p * step:first_draw + p * step + n]) for p in range(n_part)]
        means.append(np.stack([m[0] for m in mm], axis=1))
        m2s.append(np.stack([m[1] for m in mm], axis=1))
    return np.concatenate(means, axis=-1).reshape(shape), np.concatenate(m2s, axis=-1).reshape(shape)


def _block_moments(x, blocks, backend):
    """(mean, m2) float64 [C, B, *dims] of the consecutive blocks of draws `blocks` = [(first, count, length)] (count blocks of
    `length` draws from draw `first`): one kernel call per entry."""
    ms = [segment_moments(x, cnt, ln, first, backend=backend) for first, cnt, ln in blocks]
    return np.concatenate([m[0] for m in ms], axis=1), np.concatenate([m[1] for m in ms], axis=1)


def chain_moments(x, backend="auto"):
    """(mean, std) of every chain and dimension, float64 [C, *dims]; std with ddof 0 (two sweeps, as numpy.std)."""
    x = _check(x, 1)
    n = x.shape[1]
    mean, m2 = segment_moments(x, backend=backend)
    return mean[:, 0], np.sqrt(m2[:, 0] / n)


def _reduce(v, dims, axis, fn_t, fn_np):
    if isinstance(v, torch.Tensor):
        v = v.reshape(dims)
        ax = tuple(range(v.ndim)) if axis is None else axis
        if v.ndim == 0 or ax == ():
            return _np(v)
        return _np(fn_t(v, ax))
    return fn_np(v.reshape(dims), axis)


def multi_ess(x, axis=None, backend="auto"):
    """harmean(effective_sample_size(x), axis): the harmonic mean over the dimensions (montecosmo/metrics.py:562-566)."""
    x, tau, _ = _tau(x, True, backend)
    cn = x.shape[0] * x.shape[1]
    if isinstance(tau, torch.Tensor):
        return _reduce(tau, tuple(x.shape[2:]), axis, lambda t, ax: cn / t.mean(dim=ax), None)      # 1 / mean(1 / ess), 1 / ess = tau / (C N)
    with np.errstate(divide="ignore", invalid="ignore"):
        return harmean(cn / tau.reshape(tuple(x.shape[2:])), axis)


def multi_gr(x, axis=None, backend="auto"):
    """sqrt(mean(gelman_rubin(x)^2, axis)) (montecosmo/metrics.py:568-572)."""
    r, dims = _rhat(x, False, backend)
    return _reduce(r, dims, axis, lambda t, ax: torch.sqrt((t * t).mean(dim=ax)), lambda a, ax: np.sqrt(np.mean(a ** 2, axis=ax)))


def quantile(x, p, backend="auto"):
    """bdec.quantile of the pooled chains and draws of x (C, N, *dims): float64 (*p.shape, *dims)."""
    from . import bdec      # (imports this module for its chunks)
    return bdec.quantile(_check(x, 1), p, axis=(0, 1), backend=backend)


def credint(x, p=.95, type="small", backend="auto"):
    """bdec.credint of the pooled chains and draws of x (C, N, *dims): float64 (*p.shape, *dims, 2); the smallest interval takes a scalar p."""
    from . import bdec
    return bdec.credint(_check(x, 1), p, axis=(0, 1), type=type, backend=backend)


# ------------------------------------------------------------------------------------------------
N_EVALS = "n_evals"


def _take(x, idx, axis):
    if isinstance(x, torch.Tensor):
        return x.index_select(axis, torch.as_tensor(idx, device=x.device))
    return np.take(x, idx, axis)


class Chains(dict):
    """A dict of named (C, N, ...) arrays (numpy or torch) with the metric transforms of montecosmo/chains.py:342-536.  The entry
    'n_evals' (evaluations per transition) is summed where the others are mapped.  Results are float64 numpy arrays."""

    def __init__(self, *args, backend="auto", **kwargs):
        super().__init__(*args, **kwargs)
        self.backend = backend

    def copy(self):
        return Chains(self, backend=self.backend)

    def _new(self, data):
        return Chains(data, backend=self.backend)

    # ---- construction ---------------------------------------------------------------------------------
    @classmethod
    def from_flat(cls, draws, layout, backend="auto"):
        """Named entries of flat states `draws` (C, N, d): layout name -> (start, stop, shape), as FlatLogDensity.layout() gives it.
        The entries are views: nothing is copied."""
        if not isinstance(draws, torch.Tensor):
            draws = np.asarray(draws)
        if draws.ndim != 3:
            raise ValueError(f"flat draws must have shape (chains, draws, d), got {tuple(draws.shape)}")
        out = {}
        for name, (start, stop, shape) in layout.items():
            if not 0 <= start <= stop <= draws.shape[2] or int(np.prod(shape, dtype=np.int64)) != stop - start:
                raise ValueError(f"layout of {name!r} does not fit: ({start}, {stop}, {shape}) in flat states of length {draws.shape[2]}")
            part = draws[:, :, start:stop]
            if isinstance(part, torch.Tensor):
                out[name] = part.unflatten(2, tuple(shape)) if len(shape) else part[:, :, 0]
            else:
                out[name] = part.reshape(draws.shape[:2] + tuple(shape))
        return cls(out, backend=backend)

    @classmethod
    def load_runs(cls, paths, start, end, layout=None, transforms=None, backend="auto"):
        """Chains from the files `{path}_{i}.npz`, i = start .. end, that samplers.save_run wrote: one path prefix per chain, the runs
        concatenated along the draws.  Per-transition fields are kept where 'warmup' is false.  A missing first run raises; a missing
        later run ends the range, as the reference does.  `transforms` (callables Chains -> Chains) apply to every run before it is
        joined; `layout` names the pieces of the flat 'samples'."""
        if isinstance(paths, (str, os.PathLike)):
            paths = [paths]
        per_chain = []
        for path in paths:
            runs = []
            for i in range(start, end + 1):
                name = f"{path}_{i}.npz"
                if not os.path.exists(name):
                    if i == start:
                        raise FileNotFoundError(f"first run {name} is missing")
                    break
                with np.load(name) as f:
                    part = {k: f[k] for k in f.files}
                keep = ~part.pop("warmup").astype(bool) if "warmup" in part else None
                for k in list(part):
                    if k != "samples" and keep is not None and len(part[k]) == len(keep):
                        part[k] = part[k][keep]
                runs.append(part)
            keys = [k for k in runs[0] if all(k in r for r in runs)]
            per_chain.append({k: np.concatenate([r[k] for r in runs], axis=0) for k in keys})
        keys = [k for k in per_chain[0] if all(k in p for p in per_chain)]
        data = {k: np.stack([p[k] for p in per_chain]) for k in keys}
        samples = data.pop("samples", None)
        out = cls(data, backend=backend)
        if samples is not None:
            if layout is None:
                out["samples"] = samples
            else:
                out.update(cls.from_flat(samples, layout))
        for tr in transforms or ():
            out = tr(out)
        return out

    # ---- metric transforms ------------------------------------------------------------------------------
    def metric(self, fn, *others, axis=None):
        """fn mapped over the entries (with the same entry of every `others`), except 'n_evals', which is summed along `axis`."""
        out = self._new({})
        for k, v in self.items():
            if k == N_EVALS:
                out[k] = np.sum(_host64(v), axis=axis)
            else:
                out[k] = fn(v, *(o[k] for o in others))
        return out

    def last(self, axis=1):
        return self.metric(lambda x: _host64(_take(x, [x.shape[axis] - 1], axis)).squeeze(axis), axis=axis)

    def _power_sums(self, x, m, blocks):
        """sum_t x^m over each block of draws, float64 [C, B, *dims, len(m)] (m a list) or [C, B, *dims] (m an int)."""
        ms = [m] if isinstance(m, (int, np.integer)) else [int(v) for v in m]
        shape = (x.shape[0], sum(b[1] for b in blocks)) + tuple(x.shape[2:])
        if set(ms) <= {0, 1, 2}:
            mean, m2 = _block_moments(x, blocks, self.backend)
            n = np.concatenate([np.full(cnt, float(ln)) for _, cnt, ln in blocks]).reshape((1, -1) + (1,) * (x.ndim - 2))
            sums = {0: np.broadcast_to(n, mean.shape), 1: n * mean, 2: m2 + n * mean * mean}      # raw power sums from mean and m2
            out = [sums[v].reshape(shape) for v in ms]
        else:
            a = _host64(x)
            out = [np.stack([np.sum(a[:, first + b * ln:first + (b + 1) * ln] ** v, axis=1) for first, cnt, ln in blocks for b in range(cnt)],
                            axis=1) for v in ms]
        return out[0] if isinstance(m, (int, np.integer)) else np.stack(out, axis=-1)

    def moment(self, m=(0, 1, 2)):
        """sum_t x^m over the draws: [C, *dims, len(m)] (a list m) or [C, *dims] (an int m)."""
        return self.metric(lambda x: self._power_sums(_check(x, 1), m, [(0, 1, x.shape[1])])[:, 0], axis=1)

    def center_moment(self, axis=-1):
        """(count, sum x, sum x^2) along `axis` -> (mean, std) along it."""
        def center(mom):
            mom = np.moveaxis(_host64(mom), axis, 0)
            mean = mom[1] / mom[0]
            return np.stack((mean, (mom[2] / mom[0] - mean ** 2) ** .5), axis)
        return self.metric(center, axis=())

    def cmoment(self):
        """(mean, std) over the draws, stacked last: [C, *dims, 2]."""
        return self.metric(lambda x: np.stack(chain_moments(x, self.backend), axis=-1), axis=1)

    def mse_cmoment(self, true_cmom, axis=None):
        """Squared errors of the chains' mean and std against `true_cmom` (entries [..., 2] = mean, std), in units of the true variance,
        per chain count: stack(mean_axis ((m - m0) / s0)^2 / C, mean_axis 2 ((s - s0) / s0)^2 / C)."""
        def mse_mom(est, true):
            n_chains = est.shape[0]
            est, true = np.moveaxis(est, -1, 0), np.moveaxis(_host64(true), -1, 0)
            sq_mean = ((est[0] - true[0]) / true[1]) ** 2 / n_chains
            sq_std = 2 * ((est[1] - true[1]) / true[1]) ** 2 / n_chains
            return np.stack((sq_mean.mean(axis), sq_std.mean(axis)))
        return self.cmoment().metric(mse_mom, true_cmom)

    def _times(self, op):
        return self._new({k: (v if k == N_EVALS else op(self[N_EVALS], v)) for k, v in self.items()})

    def eval_times_mse(self, truth, axis=None):
        return self.mse_cmoment(truth, axis=axis)._times(lambda n, x: n * x)

    def multi_ess(self, axis=None):
        return self.metric(lambda x: multi_ess(x, axis=axis, backend=self.backend))

    def multi_gr(self, axis=None):
        return self.metric(lambda x: multi_gr(x, axis=axis, backend=self.backend))

    def eval_per_ess(self, axis=None):
        return self.multi_ess(axis=axis)._times(lambda n, x: n / x)

    def quantile(self, p):
        """Quantiles of the pooled chains and draws of every entry: (*p.shape, *dims) (bdec.quantile)."""
        return self.metric(lambda x: quantile(x, p, backend=self.backend), axis=(0, 1))

    def credint(self, p=.95, type="small"):
        """Credible intervals of the pooled chains and draws of every entry: (*p.shape, *dims, 2) (bdec.credint)."""
        return self.metric(lambda x: credint(x, p, type=type, backend=self.backend), axis=(0, 1))

    def coverage(self, truth, p=.95, type="small"):
        """Per entry of `truth` (a dict of arrays of shape dims) the fraction of its dimensions with low <= truth <= high, the p-credible
        interval of `type` taken over the pooled chains and draws."""
        out = {}
        for k, t in truth.items():
            ci = credint(self[k], p, type=type, backend=self.backend)
            t = _host64(t)
            if t.shape != ci.shape[:-1]:
                raise ValueError(f"truth of {k!r} must have shape {ci.shape[:-1]}, got {t.shape}")
            out[k] = float(np.mean((ci[..., 0] <= t) & (t <= ci[..., 1])))
        return out

    def thin(self, thinning=None, moment=None):
        """The draws in n_split = max(rint(N / thinning), 1) blocks (as numpy.array_split makes them) -> one value per block along axis 1:
        the last draw, or with `moment` the power sums of the block (`moment` as in Chains.moment)."""
        n = next(iter(self.values())).shape[1]
        n_split = 1 if thinning is None else int(max(np.rint(n / thinning), 1))
        if n_split > n:
            raise ValueError(f"{n_split} blocks from {n} draws")
        q, rem = divmod(n, n_split)
        blocks = [b for b in ((0, rem, q + 1), (rem * (q + 1), n_split - rem, q)) if b[1] > 0]      # two lengths: two sub-ranges
        ends = np.concatenate([first + ln * np.arange(1, cnt + 1) for first, cnt, ln in blocks])
        out = self._new({})
        for k, v in self.items():
            if k == N_EVALS:
                out[k] = np.add.reduceat(_host64(v), np.concatenate([[0], ends[:-1]]), axis=1)
            elif moment is None:
                out[k] = _host64(_take(v, ends - 1, 1))
            else:
                out[k] = self._power_sums(_check(v, 1), moment, blocks)
        return out

    def summary(self, names=None, file=None):
        """Per scalar entry (per component of the entries in `names`): mean, std, median, 5 %, 95 %, n_eff and the split r_hat, as a dict
        name -> dict, and printed.  Quantiles are made on the host."""
        if names is None:
            names = [k for k, v in self.items() if k != N_EVALS and not isinstance(v, tuple) and v.ndim == 2]
        out = {}
        for k in np.atleast_1d(names):
            x = self[k]
            ess = effective_sample_size(x, backend=self.backend).reshape(-1)
            rhat = (split_gelman_rubin(x, backend=self.backend) if x.shape[1] >= 4 else np.full(x.shape[2:], np.nan)).reshape(-1)
            a = _host64(x).reshape(x.shape[0] * x.shape[1], -1)
            q = np.quantile(a, [.5, .05, .95], axis=0)
            for i, ids in enumerate(np.ndindex(*x.shape[2:])):
                label = k + ("[" + ",".join(map(str, ids)) + "]" if ids else "")
                out[label] = {"mean": float(a[:, i].mean()), "std": float(a[:, i].std()), "median": float(q[0, i]), "5.0%": float(q[1, i]),
                              "95.0%": float(q[2, i]), "n_eff": float(ess[i]), "r_hat": float(rhat[i])}
        cols = ["mean", "std", "median", "5.0%", "95.0%", "n_eff", "r_hat"]
        width = max([len(k) for k in out] + [4])
        print(" " * width + "".join(f"{c:>11}" for c in cols), file=file)
        for k, row in out.items():
            print(f"{k:>{width}}" + "".join(f"{row[c]:>11.4g}" for c in cols), file=file)
        return out
