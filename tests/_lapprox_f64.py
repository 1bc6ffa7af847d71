"""numpy float64 restatement of the MAP and Laplace passes, written from their formulas: one Adam epoch and the `optimize` loop, the
splitmix64 Rademacher hash, Hutchinson's diagonal with the same probes, and the Schur sum."""
import math

import numpy as np

U64 = np.uint64


def splitmix64(x):
    x = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def rademacher(seed, probe, d, start=0, stop=None):
    """r_i = +1 if the top bit of splitmix64(i ^ key) is 0, else -1, key = splitmix64(seed ^ splitmix64(probe)); 0 outside start:stop."""
    stop = d if stop is None else stop
    key = splitmix64(U64(seed) ^ splitmix64(U64(probe)))
    r = np.zeros(d)
    h = splitmix64(np.arange(start, stop, dtype=U64) ^ key)
    r[start:stop] = np.where(h >> U64(63), -1.0, 1.0)
    return r


def adam_step(q, m, v, g, i, lr0=0.1, b1=0.9, b2=0.999, eps=1e-8):
    """Epoch i of Adam for the gradient g of the LOG density; float64 in, float64 (q', m', v') out, nothing rounded to float32."""
    q, m, v, gu = (np.asarray(a, np.float64) for a in (q, m, v, -np.asarray(g, np.float64)))
    lr, c1, c2 = lr0 / math.sqrt(1.0 + i), 1.0 / (1.0 - b1 ** (i + 1)), 1.0 / (1.0 - b2 ** (i + 1))
    m = (1.0 - b1) * gu + b1 * m
    v = (1.0 - b2) * (gu * gu) + b2 * v
    return q - (lr * (m * c1)) / (np.sqrt(v * c2) + eps), m, v


def optimize(fn, start, lr0=0.1, n_epochs=100, **kw):
    """The loop of `samplers.optimize` on numpy float64; fn(q) -> (lp, g).  Returns (q, pots, trajectory of epoch starts)."""
    q = np.array(start, np.float64)
    m, v, pots, traj = np.zeros_like(q), np.zeros_like(q), [], []
    for i in range(n_epochs):
        lp, g = fn(q)
        pots.append(-lp)
        traj.append(q.copy())
        q, m, v = adam_step(q, m, v, g, i, lr0, **kw)
    return q, pots, traj


def hutchinson_accumulate(diag, gp, gm, r, coef):
    """diag + coef (r (g+ - g-)), each operation rounded on its own."""
    return diag + coef * (r * (np.asarray(gp, np.float64) - np.asarray(gm, np.float64)))


def hess_diag_hutchinson(grad_U, q, n_probes, seed, fd_step, start=0, stop=None):
    """(1 / n) sum_p r_p (grad U(q + eps r_p) - grad U(q - eps r_p)) / (2 eps), in the order the product adds the probes."""
    q = np.asarray(q, np.float64)
    diag = np.zeros(q.size)
    for p in range(n_probes):
        r = rademacher(seed, p, q.size, start, stop)
        diag = hutchinson_accumulate(diag, -grad_U(q + fd_step * r), -grad_U(q - fd_step * r), r, -1.0 / (2.0 * fd_step * n_probes))
    return diag


def schur_sum(B, D, eps_diag):
    """B (D + eps_diag)^-1 B^T with the sums in extended precision."""
    B, w = np.asarray(B, np.float64).astype(np.longdouble), 1.0 / (np.asarray(D, np.float64) + eps_diag)
    return np.asarray((B * w.astype(np.longdouble)) @ B.T, np.float64)
