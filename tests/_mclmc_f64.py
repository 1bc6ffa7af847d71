"""numpy float64 restatement of the isokinetic integrator behind the MCLMC / MAMS samplers, written from its formulas: the velocity
update B, the drift A, one McLachlan step, the warm-up's moments update and `collapse_configs`.  The sums are taken in extended
precision, so that a float64 sum taken in another order can be held to it."""
import numpy as np

LAMBDA = 0.1931833275037836


def _sum(x):
    return float(np.sum(np.asarray(x, dtype=np.float64).astype(np.longdouble)))


def sums(u, g, s=None):
    """sum gt^2, sum u gt, sum u^2 with gt = s g, every operand taken to float64 first."""
    u, g = np.asarray(u, np.float64), np.asarray(g, np.float64)
    gt = g if s is None else np.asarray(s, np.float64) * g
    return _sum(gt * gt), _sum(u * gt), _sum(u * u)


def kick_coefficients(gg, ug, uu, d, eps):
    """(ca, cb, dK) with u' = ca gt + cb u."""
    n = np.sqrt(uu)
    if not gg > 0.:
        return 0., 1. / n, 0.
    gam = np.sqrt(gg)
    c = ug / (gam * n)
    delta = eps * gam / (d - 1)
    z = np.exp(-delta)
    D = max((1. + c) + (1. - c) * z * z, 1e-300)
    return (1. - z) * (1. + z + c * (1. - z)) / (gam * D), 2. * z / (n * D), (d - 1) * (delta - np.log(2.) + np.log(D))


def kick(u, g, eps, s=None):
    """B(eps): returns (u', dK, (sum gt^2, sum u gt, sum u^2))."""
    u, g = np.asarray(u, np.float64), np.asarray(g, np.float64)
    gt = g if s is None else np.asarray(s, np.float64) * g
    st = sums(u, g, s)
    ca, cb, dK = kick_coefficients(*st, u.size, eps)
    return ca * gt + cb * u, dK, st


def drift(q, u, eps, s=None):
    """A(eps): q + eps s u."""
    q, u = np.asarray(q, np.float64), np.asarray(u, np.float64)
    return q + eps * (u if s is None else np.asarray(s, np.float64) * u)


def kick_drift(u, q, g, eps_kick, eps_drift, s=None, dtype=np.float64):
    """What one call of the kernel does: u' rounded to `dtype`, then q' = q + eps_drift s u' from the ROUNDED u', rounded."""
    un, dK, st = kick(u, g, eps_kick, s)
    un = un.astype(dtype)
    qn = None if q is None else drift(q, un, eps_drift, s).astype(dtype)
    return un, qn, dK, st


def mclachlan_step(fn, q, u, lp, g, eps, s=None):
    """B(lam eps) A(eps/2) B((1 - 2 lam) eps) A(eps/2) B(lam eps); fn(q) -> (log density, gradient).  Returns (q, u, lp, g, dE)."""
    u, k1, _ = kick(u, g, LAMBDA * eps, s)
    q = drift(q, u, 0.5 * eps, s)
    _, g1 = fn(q)
    u, k2, _ = kick(u, g1, (1. - 2. * LAMBDA) * eps, s)
    q = drift(q, u, 0.5 * eps, s)
    lp2, g2 = fn(q)
    u, k3, _ = kick(u, g2, LAMBDA * eps, s)
    return q, u, lp2, g2, (k1 + k2 + k3) - (lp2 - lp)


def moments(q, gamma, w, xavg, x2avg):
    q = np.asarray(q, np.float64)
    return gamma * xavg + w * q, gamma * x2avg + w * (q * q)


def collapse_configs(configs, eval_per_ess=1e3):
    eps = float(np.median([c["step_size"] for c in configs]))
    ims = [c["inverse_mass"] for c in configs if c.get("inverse_mass") is not None]
    return {"L": 0.4 * eval_per_ess / 2. * eps, "step_size": eps,
            "inverse_mass": np.median(np.stack([np.asarray(m, np.float64) for m in ims]), axis=0) if ims else None}
