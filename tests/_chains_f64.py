"""Float64 numpy restatement of the chain diagnostics that montecosmo/metrics.py:562-579 takes from numpyro.diagnostics
(effective_sample_size, gelman_rubin, split_gelman_rubin), for the tests of montecosmo_amd/chains.py and csrc/chains.hip.

numpyro is not installed where these tests run: the definitions below are restated from knowledge of its source, not checked against
it (the status jax_cosmo has in SURVEY section 8(c)).  The known answers of tests/test_chains_host.py pin this reading of them.

For x[c, t, ...] with C chains and N draws, every trailing index is one independent dimension:
    m_c = mean_t x,  v_c = sum_t (x - m_c)^2 / (N - 1),  W = mean_c v_c,  V = W (N - 1) / N  (+ var_c(m_c, ddof=1) if C > 1; else W = V)
    gelman_rubin = sqrt(V / W);  split_gelman_rubin = gelman_rubin of the 2 C half chains x[:, :h], x[:, -h:], h = N // 2
    gamma_c(k) = sum_{t < N - k} (x_t - m_c)(x_{t+k} - m_c) / N   (bias=False: / (N - k))
    rho_k = 1 - (W - mean_c gamma_c(k)) / V,  rho_0 = 1;  P_j = rho_2j + rho_2j+1, j < N_even / 2, N_even = N - N % 2
    tau = -1 + 2 (P_0 + sum_{j >= 1} cummin_j max(P_j, 0));  ess = C N / tau
    L = 2 (j_stop + 1), j_stop the first j >= 1 with P_j <= 0, else the last pair.
Written independently of chains.py's host path: the autocovariance here is a direct sum per lag (small N) or a zero-padded real FFT of
length 2 N (large N); nothing is imported from the package.
"""
import numpy as np

DIRECT_MAX_DRAWS = 300      # direct sums up to this N (exact order-free reference for the tight bounds at tiny N), the FFT above


def _check(x):
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim >= 2 and x.shape[1] >= 2
    return x


def autocov_direct(y):
    """sum_t y[c, t] y[c, t + k] for k = 0 .. N - 1, shape (C, N, ...)."""
    n = y.shape[1]
    out = np.empty_like(y)
    for k in range(n):
        out[:, k] = np.sum(y[:, :n - k] * y[:, k:], axis=1)
    return out


def autocov_fft(y):
    n = y.shape[1]
    f = np.fft.rfft(y, n=2 * n, axis=1)
    return np.fft.irfft(f.real ** 2 + f.imag ** 2, n=2 * n, axis=1)[:, :n]


def within_between(x):
    """(W, V) of the definitions."""
    x = _check(x)
    c, n = x.shape[:2]
    w = x.var(axis=1, ddof=1).mean(axis=0)
    v = w * (n - 1) / n
    if c > 1:
        v = v + x.mean(axis=1).var(axis=0, ddof=1)
    else:
        w = v
    return w, v


def gelman_rubin(x):
    w, v = within_between(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(v / w)


def split_halves(x):
    x = _check(x)
    h = x.shape[1] // 2
    return np.concatenate([x[:, :h], x[:, -h:]], axis=0)


def split_gelman_rubin(x):
    return gelman_rubin(split_halves(x))


def pair_sums(x, bias=True, method=None):
    """P[j, ...] for j < N_even / 2."""
    x = _check(x)
    c, n = x.shape[:2]
    y = x - x.mean(axis=1, keepdims=True)
    if method is None:
        method = "direct" if n <= DIRECT_MAX_DRAWS else "fft"
    s = (autocov_direct if method == "direct" else autocov_fft)(y)
    div = np.full(n, float(n)) if bias else (n - np.arange(n)).astype(np.float64)
    gamma = (s / div.reshape((1, n) + (1,) * (x.ndim - 2))).mean(axis=0)
    w, v = within_between(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = 1. - (w - gamma) / v
    rho[0] = 1.
    n_even = n - n % 2
    return rho[0:n_even:2] + rho[1:n_even:2]


def tau_and_lags(x, bias=True, method=None, return_pairs=False):
    """(tau, L) per dimension; with return_pairs also P."""
    p = pair_sums(x, bias, method)
    npair = p.shape[0]
    with np.errstate(invalid="ignore"):
        mono = np.minimum.accumulate(np.maximum(p[1:], 0.), axis=0)      # NaN propagates through both
        tau = -1. + 2. * (p[0] + mono.sum(axis=0))
        stop = p[1:] <= 0.
    first = np.where(stop.any(axis=0), stop.argmax(axis=0) + 1, npair - 1)
    lags = np.minimum(2 * (first + 1), 2 * npair).astype(np.int64)
    return (tau, lags, p) if return_pairs else (tau, lags)


def effective_sample_size(x, bias=True, method=None):
    x = _check(x)
    tau, _ = tau_and_lags(x, bias, method)
    with np.errstate(divide="ignore", invalid="ignore"):
        return x.shape[0] * x.shape[1] / tau


def harmean(a, axis=None):
    return 1. / np.mean(1. / np.asarray(a, dtype=np.float64), axis=axis)


def geomean(a, axis=None):
    return np.exp(np.mean(np.log(np.asarray(a, dtype=np.float64)), axis=axis))


def multi_ess(x, axis=None, method=None):
    return harmean(effective_sample_size(x, method=method), axis)


def multi_gr(x, axis=None):
    return np.sqrt(np.mean(gelman_rubin(x) ** 2, axis=axis))


def ar1(rng, phi, shape, dtype=np.float64):
    """Stationary AR(1) chains x_t = phi x_{t-1} + sqrt(1 - phi^2) e_t of shape (C, N, ...); phi a number or an array over the dims."""
    e = rng.standard_normal(shape)
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), shape[2:])
    x = np.empty(shape)
    x[:, 0] = e[:, 0]
    s = np.sqrt(1. - phi ** 2)
    for t in range(1, shape[1]):
        x[:, t] = phi * x[:, t - 1] + s * e[:, t]
    return x.astype(dtype)
