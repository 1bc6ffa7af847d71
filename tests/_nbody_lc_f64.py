"""N-body evolution on the light cone in float64 numpy (checker only; it never imports the library), composed from oracle.pm_oracle:
`nbody_bf(..., return_traj=True)`, `euler_times` (inside it), `dkd_vjp`, `lpt_vjp`.

Definition.  A run of K steps from a0 to a_end has g0 = a2g(a0), dg = (a2g(a_end) - g0) / K and the Euler step states
(x_i, v_i), i = 0 .. K.  Particle p, whose Lagrangian lattice point has the scale factor a_p, takes the state at g_p = a2g(a_p):
    s = (g_p - g0) / dg,   i = clamp(floor(s), 0, K - 1),   theta = clamp(s - i, 0, 1),
    state_p = (1 - theta) state_i[p] + theta state_{i+1}[p]
-- diffrax's dense output, per particle.  Earlier than a0: the LPT start state; later than a_end: the final state.

The reverse sweep injects the loss cotangents (Xb, Vb) of the light-cone state into state j with the weight w_j = 1 - theta (i_p = j),
theta (i_p = j - 1), 0 (otherwise): state K opens the sweep, state j follows step j's adjoint.  g_bar_p = (Xb . (x_{i+1} - x_i) +
Vb . (v_{i+1} - v_i)) / dg where theta was not clamped; through theta, g0 receives -sum g_bar_p and dg receives -sum g_bar_p (g_p - g0) / dg.

A model-level `evolve` / `log_density` for evolution='nbody', a_obs=None is built from the pieces tests/_model_f64.py uses."""
import numpy as np

import _ap_f64 as apo
import _eulerian_f64 as ef
import _model_f64 as M
import _png_f64 as pf
from oracle import pm_oracle as o, bias_oracle as bo


def locate(g_p, g0, dg, K):
    """(i, theta, inside) of the definition; `inside`: theta was not clamped."""
    s = (np.asarray(g_p, dtype=np.float64).reshape(-1) - g0) / dg
    i = np.clip(np.floor(s), 0, K - 1).astype(int)
    th = s - i
    return i, np.clip(th, 0., 1.), (th >= 0.) & (th <= 1.)


def select(traj, g_p, g0, dg):
    """Light-cone (pos, vel) from the K + 1 step states `traj` = [(pos_i, vel_i)]."""
    K = len(traj) - 1
    i, th, _ = locate(g_p, g0, dg, K)
    X, V = np.stack([t[0] for t in traj]), np.stack([t[1] for t in traj])
    n = np.arange(len(i))
    th = th[:, None]
    return (1 - th) * X[i, n] + th * X[i + 1, n], (1 - th) * V[i, n] + th * V[i + 1, n]


def weights(g_p, g0, dg, K):
    """(K + 1, N): the weight of state j for particle p."""
    i, th, _ = locate(g_p, g0, dg, K)
    w = np.zeros((K + 1, len(i)))
    n = np.arange(len(i))
    w[i, n] += 1 - th
    w[i + 1, n] += th
    return w


def run(cosmo, init_mesh, pos, a0, a_end, n_steps, paint_order=2, lpt_order=2, alpha_fn=o.alpha_bf):
    """The fixed-time run whose step states the light cone interpolates: (traj, g0, dg)."""
    _, traj, ts, dg = o.nbody_bf(cosmo, init_mesh, pos, a0, a_end, n_steps, paint_order, lpt_order, alpha_fn=alpha_fn, return_traj=True)
    return traj, ts[0], dg


def nbody_lc(cosmo, init_mesh, pos, a0, a_p, a_end, n_steps, paint_order=2, lpt_order=2, alpha_fn=o.alpha_bf, g_p=None):
    """(pos, vel) on the light cone; a_p: (N,) or (N,1) scale factors (or their growth factors `g_p` directly)."""
    traj, g0, dg = run(cosmo, init_mesh, pos, a0, a_end, n_steps, paint_order, lpt_order, alpha_fn)
    g_p = o.a2g(cosmo, np.asarray(a_p, dtype=np.float64).reshape(-1)) if g_p is None else g_p
    return select(traj, g_p, g0, dg)


def nbody_lc_vjp(cosmo, init_mesh, pos, pos_bar, vel_bar, a0, a_p, a_end, n_steps, paint_order=2, lpt_order=2, alpha_fn=o.alpha_bf, g_p=None):
    """Reverse sweep with per-state injection: (init_mesh_bar, scalar_bars, g_bar_p).  scalar_bars as o.nbody_bf_vjp's ('alpha', 'beta',
    'dg', 'g', 'g2', 'dg2dg'), with the theta terms of g0 and dg added into 'g' and 'dg' and also given alone as 'g0_theta', 'dg_theta'."""
    _, traj, ts, dg = o.nbody_bf(cosmo, init_mesh, pos, a0, a_end, n_steps, paint_order, lpt_order, alpha_fn=alpha_fn, return_traj=True)
    K, g0 = n_steps, ts[0]
    g_p = o.a2g(cosmo, np.asarray(a_p, dtype=np.float64).reshape(-1)) if g_p is None else np.asarray(g_p, dtype=np.float64).reshape(-1)
    Xb, Vb = np.asarray(pos_bar, dtype=np.float64), np.asarray(vel_bar, dtype=np.float64)
    w = weights(g_p, g0, dg, K)
    mesh_shape = o.ch2rshape(init_mesh.shape)
    xb, vb = w[K][:, None] * Xb, w[K][:, None] * Vb
    abar, bbar, dgbar = np.zeros(K), np.zeros(K), 0.
    for i in reversed(range(K)):
        x, v = traj[i]
        r = (ts[i + 1] - ts[i]) / dg
        alpha = float(alpha_fn(cosmo, ts[i], dg))
        xb2, vb2, ab, bb, db = o.dkd_vjp(x, v, r * xb, r * vb, dg, alpha, ts[i] + dg / 2, mesh_shape, paint_order)
        xb = (1 - r) * xb + xb2 + w[i][:, None] * Xb
        vb = (1 - r) * vb + vb2 + w[i][:, None] * Vb
        abar[i], bbar[i] = ab, bb
        dgbar += db
    mesh_bar, _, sbar = o.lpt_vjp(cosmo, init_mesh, pos, a0, xb, vb, lpt_order=lpt_order, read_order=1)
    i, th, inside = locate(g_p, g0, dg, K)
    n = np.arange(len(i))
    X, V = np.stack([t[0] for t in traj]), np.stack([t[1] for t in traj])
    g_bar_p = inside * ((Xb * (X[i + 1, n] - X[i, n])).sum(-1) + (Vb * (V[i + 1, n] - V[i, n])).sum(-1)) / dg
    g0_th, dg_th = -float(g_bar_p.sum()), -float((g_bar_p * (g_p - g0) / dg).sum())
    sbar.update(alpha=abar, beta=bbar, dg=dgbar + dg_th, g0_theta=g0_th, dg_theta=dg_th)
    sbar["g"] = sbar["g"] + g0_th
    return mesh_bar, sbar, g_bar_p


# ---- the forward model with evolution='nbody' on the light cone ------------------------------------------------------------------
def lattice_a(cfg, cosmo):
    """(a_p (N,1) of the Lagrangian lattice, a_end = chi2a(cosmo, r_min) of its nearest point)."""
    R = bo.rotvec_matrix(cfg["box_rotvec"])
    pos0 = o.regular_pos(cfg["evol_shape"], cfg["ptcl_shape"])
    p = bo.cell2phys_pos(pos0, cfg["box_center"], R, cfg["box_size"], cfg["evol_shape"])
    if cfg["curved_sky"]:
        r = np.linalg.norm(p, axis=-1)
    else:
        los = o.safe_div(np.asarray(cfg["box_center"], dtype=float), np.linalg.norm(cfg["box_center"]))
        r = np.abs((p * los).sum(-1))
    return o.chi2a(cosmo, r)[:, None], float(o.chi2a(cosmo, r.min()))


def evolve(cfg, cosmo, bias, white, *, png=None, png_type=None, bias_type="lagrangian", ap_auto=None, ap=None, cosmo_fid=None):
    """tests/_model_f64.py::evolve with the N-body branch on the light cone (cfg['evolution'] = 'nbody', cfg['a_obs'] = None): every
    particle at the scale factor of its Lagrangian lattice point, the run ending at the nearest one's; the observation pass keeps taking
    a at the evolved position."""
    assert cfg["evolution"] == "nbody" and cfg["a_obs"] is None
    from _lik_phi_f64 import evol_mesh
    aux = dict(white=white, evol_mesh=evol_mesh(cfg, cosmo, white), pos=None, weights=None, phi=None)
    R = bo.rotvec_matrix(cfg["box_rotvec"])
    box, ctr, es = cfg["box_size"], cfg["box_center"], cfg["evol_shape"]
    lin = aux["evol_mesh"]
    pos0 = o.regular_pos(es, cfg["ptcl_shape"])
    a, a_end = lattice_a(cfg, cosmo)
    pngp = phi_pos = None
    if png_type is None:
        w, dvel = bo.lagrangian_bias(o.a2g(cosmo, a), pos0, box, lin, bias, read_order=1)
    else:
        pngp = pf.fNL_bias({k: (png or {}).get(k, 0.) for k in pf.PNG_KEYS}, bias, 1., png_type)
        table = pf.trans_table(cosmo)
        w, dvel, aux["phi"] = pf.lagrangian_bias(table, o.a2g(cosmo, a), pos0, box, lin, bias, pngp, read_order=1)
        phi_pos = o.read(pos0, aux["phi"], 1)
        lin = pf.add_png(table, pngp["fNL"], lin, box)
        lin = o.chreshape(o.chreshape(lin, o.r2chshape(cfg["init_shape"])), o.r2chshape(es))
    cosmo._workspace = {}
    pos, vel = nbody_lc(cosmo, lin, pos0, cfg["nbody_a_start"], a, a_end, cfg["nbody_n_steps"], cfg["paint_order"], cfg["lpt_order"])
    los, p = apo.observe_phys(cosmo, pos, vel, ctr, R, box, es, None, cfg["curved_sky"], dvel)
    p = apo.apply_ap(p, los, cosmo, cfg["curved_sky"], ap_auto, ap, cosmo_fid)
    pos_c = bo.phys2cell_pos(p, ctr, R, box, cfg["init_shape"])
    aux.update(pos=pos_c, weights=w)
    if bias_type == "eulerian":
        return ef.painted_bias(cfg, pos_c, phi_pos, bias, pngp), aux
    return apo.paint(cfg, pos_c, w), aux


def log_density(*args, **kwargs):
    """tests/_model_f64.py::log_density with `evolve` above in the place of its own (which, like the reference, has no N-body light cone)."""
    keep, M.evolve = M.evolve, evolve
    try:
        return M.log_density(*args, **kwargs)
    finally:
        M.evolve = keep
