"""Laplace approximation of the posterior around a mode (the names of montecosmo/lapprox.py): the diagonal of the Hessian of the
potential U = -log p, and the marginal covariance of the first few (scalar) parameters through the Schur complement.

The reference takes Hessian-vector products from jax's autodiff.  Here the gradient is hand-written, so they are central differences of
it:  H r ~ (grad U(q + eps r) - grad U(q - eps r)) / (2 eps),  two gradient evaluations each.  Every function takes the flat contract
`logdensity_and_grad(q) -> (lp, g)` of samplers.py (`samplers.FlatLogDensity`, or any closure on a flat tensor), g the gradient of the
LOG density, and works in two ways, chosen as `samplers.make_integrator` chooses: backend 'hip' on flat contiguous float32 device
tensors through the passes of csrc/lapprox.hip, 'torch' on anything else (CPU float64 included) through torch ops with the same formulas,
'auto' takes 'hip' where it applies.

The Rademacher probes are never stored.  Probe p of a seed is a counter-based hash, regenerated wherever it is needed.  With 64-bit
wrap-around arithmetic and

    splitmix64(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;
                    return x ^ (x >> 31)
    key = splitmix64(seed ^ splitmix64(p))
    r_i = +1 if the top bit of splitmix64(i ^ key) is 0, else -1        (start <= i < stop; r_i = 0 elsewhere)

(`rademacher` below in numpy, include/mcpm.h for the kernels).

`FD_STEP`, the default finite-difference step in the units of q (the model's sample space is standardised: one unit is about one
prior or fiducial standard deviation), is the one tuning number here; DESIGN.md records the sweep it comes from.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .samplers import hip_backend_applies

__all__ = ["hess_diag_hutchinson", "hess_diag_exact", "hess_diag_in_chunks", "cov_x_from_pot_x_y", "rademacher", "FD_STEP"]

FD_STEP = 0.01      # the middle of the plateau 0.0056 .. 0.018 of the sweep on one MI355X (profiles/map_laplace.txt; DESIGN.md, MAP and Laplace)

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    """splitmix64 of a uint64 array (or scalar), element-wise, modulo 2^64."""
    with np.errstate(over="ignore"):
        x = (np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return x ^ (x >> np.uint64(31))


def rademacher(seed, probe, d, start=0, stop=None):
    """Probe `probe` of `seed` as a float64 numpy vector of length d: +-1 on start:stop, 0 elsewhere (the hash of the module docstring)."""
    stop = d if stop is None else stop
    key = _splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ _splitmix64(np.uint64(int(probe))))
    r = np.zeros(d)
    top = _splitmix64(np.arange(start, stop, dtype=np.uint64) ^ key) >> np.uint64(63)
    r[start:stop] = 1.0 - 2.0 * top.astype(np.float64)
    return r


def _backend(q, backend):
    if backend == "auto":
        backend = "hip" if hip_backend_applies(q) else "torch"
    if backend == "hip":
        if not hip_backend_applies(q):
            raise ValueError("backend='hip' serves flat contiguous float32 device tensors")
        from . import nbody
        return nbody.get_plan((8, 8, 8))      # shape-free passes: the plan lends its stream and reduction scratch
    if backend == "torch":
        return None
    raise ValueError(f"backend must be 'auto', 'hip' or 'torch', not {backend!r}")


def _grad(fn, q, what):
    lp, g = fn(q)
    if not math.isfinite(float(lp)):
        raise FloatingPointError(f"log density is {float(lp)} at {what}: the finite-difference step left the support, reduce fd_step")
    return g if g.is_contiguous() else g.contiguous()


def hess_diag_hutchinson(logdensity_and_grad, q, n_probes=64, seed=42, fd_step=None, start=0, stop=None, backend="auto"):
    """Hutchinson's estimate of the diagonal of the Hessian H of U = -log p at q, as a float64 tensor of length d on q's device:

        diag ~ (1 / n_probes) sum_p r_p * (H r_p),      H r ~ (grad U(q + eps r) - grad U(q - eps r)) / (2 eps),  eps = fd_step,

    with r_p Rademacher on the entries start:stop and zero elsewhere (the hash of the module docstring, probes p = 0 .. n_probes - 1):
    the entries outside start:stop are held fixed and their estimate is left exactly 0, so the field can be probed with the scalars
    fixed, as `cov_x_from_pot_x_y` needs.  2 n_probes gradient evaluations.  The error of an entry is the off-diagonal mass of its
    row, |sum_{j != i} H_ij r_i r_j| / sqrt(n_probes); on a diagonal H every probe is exact."""
    d = q.numel()
    stop = d if stop is None else int(stop)
    start = int(start)
    if not 0 <= start <= stop <= d:
        raise ValueError(f"need 0 <= start <= stop <= {d}, got {start}, {stop}")
    eps = float(FD_STEP if fd_step is None else fd_step)
    coef = -1.0 / (2.0 * eps * n_probes)      # g is the gradient of the LOG density: the sign turns it into U's
    plan = _backend(q, backend)
    diag = torch.zeros(d, dtype=torch.float64, device=q.device)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if plan is not None:
        qp, qm = torch.empty_like(q), torch.empty_like(q)
    for p in range(int(n_probes)):
        if plan is not None:
            plan.call("mcpm_probe_shift_f32", q, d, start, stop, seed, p, eps, qp, qm)
            gp, gm = _grad(logdensity_and_grad, qp, "q + eps r"), _grad(logdensity_and_grad, qm, "q - eps r")
            plan.call("mcpm_hutchinson_accum_f64", gp, gm, d, start, stop, seed, p, coef, diag)
        else:
            r = torch.from_numpy(rademacher(seed, p, d, start, stop)).to(q.device)
            er = (eps * r).to(q.dtype)
            gp, gm = _grad(logdensity_and_grad, q + er, "q + eps r"), _grad(logdensity_and_grad, q - er, "q - eps r")
            diag += coef * (r * (gp.double() - gm.double()))
    return diag


def hess_diag_exact(logdensity_and_grad, q, indices=None, fd_step=None):
    """The diagonal of the Hessian of U = -log p at q on `indices` (default: every entry) by unit-vector central differences,
    H_kk ~ (dU/dq_k(q + eps e_k) - dU/dq_k(q - eps e_k)) / (2 eps): two gradient evaluations per index, for small problems and tests.
    A float64 tensor with one value per index, on q's device."""
    eps = float(FD_STEP if fd_step is None else fd_step)
    idx = list(range(q.numel())) if indices is None else [int(k) for k in indices]
    out = torch.zeros(len(idx), dtype=torch.float64, device=q.device)
    x = q.clone()
    for j, k in enumerate(idx):
        x[k] = q[k] + eps
        gp = _grad(logdensity_and_grad, x, f"q + eps e_{k}")[k].double()
        x[k] = q[k] - eps
        gm = _grad(logdensity_and_grad, x, f"q - eps e_{k}")[k].double()
        x[k] = q[k]
        out[j] = -(gp - gm) / (2.0 * eps)
    return out


def hess_diag_in_chunks(logdensity_and_grad, q, chunk_size=64, indices=None, fd_step=None):
    """`hess_diag_exact` under the reference's other name; `chunk_size` (its vmap batch) is accepted and ignored."""
    return hess_diag_exact(logdensity_and_grad, q, indices=indices, fd_step=fd_step)


def cov_x_from_pot_x_y(logdensity_and_grad, q, n_x, method="hutchinson", chunk_size=None, eps_diag=1e-9, seed=42, fd_step=None,
                       backend="auto"):
    """Marginal covariance of x = q[:n_x] (FlatLogDensity puts the scalars first) under the Laplace approximation at q = [x, y].
    With the Hessian of U = -log p in blocks, H = [A B; B^T D], Cov_x = (A - B D^-1 B^T)^-1, and D (the field's block) is taken DIAGONAL,
    so that neither D nor the full Hessian is ever formed.  Returns (cov_x, schur) as numpy float64 (n_x, n_x).

    Column i of H is a central difference of the gradient along x_i (2 n_x gradient evaluations): its first n_x entries are A[:, i], the
    rest row i of B, kept on the device as (n_x, n_y) in q's dtype (the difference is formed in float64 and rounded once).  diag D is
    `hess_diag_hutchinson` over y with chunk_size probes (default 64; the reference's default of n_y probes costs more than the exact
    diagonal), or `hess_diag_exact` with method='exact'.  schur = A - B (D + eps_diag)^-1 B^T is symmetrised and inverted in float64.

    As in the reference, D is NOT clamped: the result means something near a mode, where the whitened prior keeps D positive; away from
    one an entry of D near -eps_diag dominates the sum.  backend='hip' forms the m x m sums in mcpm_schur_f64 (n_x <= 16)."""
    d, n_x = q.numel(), int(n_x)
    n_y = d - n_x
    if not 1 <= n_x <= d:
        raise ValueError(f"need 1 <= n_x <= {d}")
    if method not in ("hutchinson", "exact"):
        raise ValueError(f"method must be 'hutchinson' or 'exact', not {method!r}")
    eps = float(FD_STEP if fd_step is None else fd_step)
    plan = _backend(q, backend)
    A = np.zeros((n_x, n_x))
    B = torch.empty((n_x, n_y), dtype=q.dtype, device=q.device)
    x = q.clone()
    for i in range(n_x):
        x[i] = q[i] + eps
        gp = _grad(logdensity_and_grad, x, f"q + eps e_{i}")
        x[i] = q[i] - eps
        gm = _grad(logdensity_and_grad, x, f"q - eps e_{i}")
        x[i] = q[i]
        col = -(gp.double() - gm.double()) / (2.0 * eps)
        A[:, i] = col[:n_x].cpu().numpy()
        B[i] = col[n_x:]
    if n_y == 0:
        bdb = np.zeros((n_x, n_x))
    else:
        if method == "hutchinson":
            D = hess_diag_hutchinson(logdensity_and_grad, q, n_probes=64 if chunk_size is None else chunk_size, seed=seed, fd_step=eps,
                                     start=n_x, stop=d, backend=backend)[n_x:]
        else:
            D = hess_diag_exact(logdensity_and_grad, q, indices=range(n_x, d), fd_step=eps)
        if plan is not None:
            out = torch.empty(n_x * n_x, dtype=torch.float64, device=q.device)
            plan.call("mcpm_schur_f64", B, n_x, n_y, n_y, D.contiguous(), float(eps_diag), out)
            bdb = out.reshape(n_x, n_x).cpu().numpy()
        else:
            Bd = B.double()
            bdb = ((Bd / (D + eps_diag)) @ Bd.T).cpu().numpy()
    schur = A - bdb
    schur = (schur + schur.T) / 2
    return np.linalg.inv(schur), schur
