"""The whole forward model and its log density in float64 numpy, composed from the per-feature restatements (checker only; it never imports
the library): Lagrangian / Eulerian bias (oracle/bias_oracle.py, tests/_eulerian_f64.py), local PNG (tests/_png_f64.py), Alcock-Paczynski
(tests/_ap_f64.py), the Kaiser model on any sky (tests/_kaiser_f64.py), the likelihood families with s_ep phi and a temperature
(tests/_lik_phi_f64.py, tests/_lik_f64.py), survey selection / mask / shells, sampled ngbars and the three preconditionings
(oracle/bias_oracle.py).  Every feature is an argument, so any mix the constructors of montecosmo_amd accept has a reference here;
tests/test_model_f64_host.py holds this composition to each per-feature restatement where that one is defined."""
import numpy as np

import _ap_f64 as apo
import _eulerian_f64 as ef
import _kaiser_f64 as kf
import _lik_f64 as L
import _lik_phi_f64 as P
import _png_f64 as pf
from oracle import pm_oracle as o, bias_oracle as bo

AP_KEYS = ("alpha_iso", "alpha_ap")
PHI_LIKS = ("quad_gauss", "shash", "two_quad_gauss")
REAL_LIKS = PHI_LIKS + ("poisson",)


def evolve(cfg, cosmo, bias, white, *, png=None, png_type=None, bias_type="lagrangian", ap_auto=None, ap=None, cosmo_fid=None):
    """FieldLevelForward.evolve for every option: (gxy mesh, aux).  aux: 'white', 'evol_mesh' (the Gaussian evolution mesh), 'pos' (observed
    positions in cells of init_shape), 'weights' (Lagrangian weights), 'phi' (the Gaussian potential on the evolution mesh; None without
    png_type or for the Kaiser model, which defines none)."""
    aux = dict(white=white, evol_mesh=P.evol_mesh(cfg, cosmo, white), pos=None, weights=None, phi=None)
    if cfg["evolution"] == "kaiser":      # no Alcock-Paczynski, and bias_type is ignored (the constructors' own rules)
        assert ap_auto is None
        return kf.evolve(cfg, cosmo, bias, white, png, png_type)[0], aux
    R = bo.rotvec_matrix(cfg["box_rotvec"])
    box, ctr, es = cfg["box_size"], cfg["box_center"], cfg["evol_shape"]
    lin = aux["evol_mesh"]
    pos0 = o.regular_pos(es, cfg["ptcl_shape"])
    _, a = bo.los_scalefactor_pos(pos0, ctr, R, box, es, cosmo, cfg["a_obs"], cfg["curved_sky"])
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
    if cfg["evolution"] == "lpt":
        dpos, vel = o.lpt(cosmo, lin, pos0, a, lpt_order=cfg["lpt_order"], read_order=1)
        pos = pos0 + dpos
    else:
        p, v = o.nbody_bf(cosmo, lin, pos0, a0=cfg["nbody_a_start"], a1=a, n_steps=cfg["nbody_n_steps"], paint_order=cfg["paint_order"],
                          lpt_order=cfg["lpt_order"])
        pos, vel = p[-1], v[-1]
    los, p = apo.observe_phys(cosmo, pos, vel, ctr, R, box, es, cfg["a_obs"], cfg["curved_sky"], dvel)
    p = apo.apply_ap(p, los, cosmo, cfg["curved_sky"], ap_auto, ap, cosmo_fid)
    pos_c = bo.phys2cell_pos(p, ctr, R, box, cfg["init_shape"])
    aux.update(pos=pos_c, weights=w)
    if bias_type == "eulerian":
        return ef.painted_bias(cfg, pos_c, phi_pos, bias, pngp), aux
    return apo.paint(cfg, pos_c, w), aux


def los_fid(cfg):
    """The box centre's direction in cell axes: the line of sight of 'fourier_gauss' (model.py:607-608)."""
    c = np.asarray(cfg["box_center"], dtype=np.float64)
    return bo.rotvec_matrix(cfg["box_rotvec"]).T @ o.safe_div(c, np.linalg.norm(c))


def log_density(cfg, latents, fixed, sample, count_obs, make_cosmo, *, lik_type="quad_gauss", temp=1., png_type=None,
                bias_type="lagrangian", ap_auto=None, cosmo_fid=None, info=None):
    """log p(sample, count_obs): the oracle's priors and preconditioning, `evolve` above, the oracle's mean counts (cfg may carry
    'selec_mesh', 'mask_mesh', 'redges', 'n_rbins', 'precond') and the likelihood `lik_type` at temperature `temp`.  The PNG parameters,
    alpha_iso / alpha_ap and s_ep are latents or fixed (missing: 0, 1 and 0); a stochastic parameter the family does not read may be absent.
    `make_cosmo(base)` returns the oracle's cosmology.  `info` (a dict) receives 'base', 'gxy', 'aux', 'count', 'selec', 'mask', 'phi',
    's_ep_phi' and, for 'quad_gauss', 'D' = b^2 + 4 a (obs - loc + a) over the observed cells (the support is D > 0)."""
    fx = dict(fixed)
    for k, v in (("s_e", 1.0), ("s_ed", 0.0), ("s_e2", 0.0)):
        if k not in fx and k not in latents:
            fx[k] = v
    lp, base, white = bo.prior_and_white(cfg, latents, fx, sample, make_cosmo)
    cosmo = make_cosmo(base)
    png = None if png_type is None else {k: base.get(k, 0.) for k in pf.PNG_KEYS}
    ap = {k: base.get(k, 1.) for k in AP_KEYS}
    gxy, aux = evolve(cfg, cosmo, {k: base[k] for k in bo.BIAS_KEYS}, white, png=png, png_type=png_type, bias_type=bias_type,
                      ap_auto=ap_auto, ap=ap, cosmo_fid=cosmo_fid)
    cosmo._workspace = {}
    final = tuple(cfg["final_shape"])
    cm, selec, mask = bo.mean_counts(cfg, base, gxy)
    selec = selec * np.ones(final)
    phi = np.zeros(final) if aux["phi"] is None else P.down(aux["phi"], final)
    s_ep = float(base.get("s_ep", 0.))
    obs = np.asarray(count_obs, dtype=np.float64)
    st = [base.get(k, 0.) for k in ("s_e", "s_ed", "s_e2")]
    if info is not None:
        info.update(base=base, gxy=gxy, aux=aux, count=cm, selec=selec, mask=mask, phi=phi, s_ep_phi=s_ep * phi[mask])
        if lik_type == "quad_gauss":
            S = P.scales(cm[mask], selec[mask], phi[mask], *st, s_ep, temp)
            info["D"] = S["b"] ** 2 + 4 * S["a"] * (obs[mask] - cm[mask] + S["a"])
    if lik_type == "fourier_gauss":      # the scale at (selec, temp) is the scale of the selection selec * temp
        assert cfg.get("mask_mesh") is None and cfg.get("selec_mesh") is None
        t = L.fourier_terms(o._rfftn(cm), o.cgh2rg(o._rfftn(obs)), cfg["box_size"], los_fid(cfg), float(selec.flat[0]) * temp, base["s_e"],
                            base["s_k2e"], base["s_kmu2e"], adjoint=False)
        return float(lp + t["sums"][0])
    if lik_type not in REAL_LIKS:
        raise ValueError(lik_type)
    return float(lp + np.sum(P.family_log_prob(lik_type, obs[mask], cm[mask], selec[mask], phi[mask], *st, s_ep, temp)))
