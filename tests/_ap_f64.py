"""float64 numpy restatement of the Alcock-Paczynski step of montecosmo (checker only; no device code):
scale_pos / parperp2isoap / isoap2parperp (bricks.py:708-732), ap_auto (bricks.py:795-814), ap_param (bricks.py:848-857), and their
place in the chain of model.py:780-799 (`observe_pos_ap`) and in `evolve` (`evolve_ap`), composed with the pieces of
oracle/bias_oracle.py (imported read-only)."""
import numpy as np

from oracle import pm_oracle as o, bias_oracle as bo


def scale_pos(pos, los, scale_par, scale_perp):
    """bricks.py:708-716"""
    pos_par = (pos * los).sum(-1, keepdims=True) * los
    pos_perp = pos - pos_par
    pos_par = pos_par * scale_par
    pos_perp = pos_perp * scale_perp
    return pos_par + pos_perp


def parperp2isoap(alpha_par, alpha_perp):
    """bricks.py:718-724"""
    alpha_iso = (alpha_par * alpha_perp ** 2) ** (1 / 3)
    alpha_ap = alpha_par / alpha_perp
    return alpha_iso, alpha_ap


def isoap2parperp(alpha_iso, alpha_ap):
    """bricks.py:726-732"""
    alpha_par = alpha_iso * alpha_ap ** (2 / 3)
    alpha_perp = alpha_iso * alpha_ap ** (-1 / 3)
    return alpha_par, alpha_perp


def ap_rpos(pos, los, curved_sky=True):
    """The distance ap_auto looks up (bricks.py:808, :811)."""
    if curved_sky:
        return np.linalg.norm(pos, axis=-1, keepdims=True)
    return np.abs((pos * los).sum(-1, keepdims=True))


def ap_auto(pos, los, cosmo, cosmo_fid, curved_sky=True, chi2a=None, a2chi_fid=None):
    """bricks.py:795-814.  `chi2a`, `a2chi_fid`: replacements of the two look-ups (a test that moves the table nodes)."""
    chi2a = (lambda r: o.chi2a(cosmo, r)) if chi2a is None else chi2a
    a2chi_fid = (lambda a: o.a2chi(cosmo_fid, a)) if a2chi_fid is None else a2chi_fid

    def alpha_fn(rpos):                                   # bricks.py:799-801
        rpos_new = a2chi_fid(chi2a(rpos))
        return o.safe_div(rpos_new, rpos)
    rpos = ap_rpos(pos, los, curved_sky)                  # curved remains curved, flat remains flat (bricks.py:807-812)
    return pos * alpha_fn(rpos)


def ap_param(pos, los, alphas, curved_sky=True):
    """bricks.py:848-857"""
    if curved_sky:
        return pos * alphas["alpha_iso"]
    alpha_par, alpha_perp = isoap2parperp(alphas["alpha_iso"], alphas["alpha_ap"])
    return scale_pos(pos, los, alpha_par, alpha_perp)


def apply_ap(p, los, cosmo, curved_sky, ap_auto_, ap=None, cosmo_fid=None, **kw):
    """model.py:787-794 on physical positions `p`."""
    if ap_auto_ is None:
        return p
    if ap_auto_:
        return ap_auto(p, los, cosmo, cosmo_fid, curved_sky, **kw)
    ap = ap or {}
    return ap_param(p, los, {"alpha_iso": ap.get("alpha_iso", 1.), "alpha_ap": ap.get("alpha_ap", 1.)}, curved_sky)


def observe_phys(cosmo, pos, vel, box_center, R, box_size, evol_shape, a_obs=None, curved_sky=True, dvel=0.):
    """model.py:780-786: (line of sight, physical redshift-space positions before Alcock-Paczynski)."""
    los, a = bo.los_scalefactor_pos(pos, box_center, R, box_size, evol_shape, cosmo, a_obs, curved_sky)
    p = bo.cell2phys_pos(pos, box_center, R, box_size, evol_shape)
    return los, p + bo.rsd(cosmo, vel, los, a, R, box_size, evol_shape, dvel)


def observe_pos_ap(cosmo, pos, vel, box_center, R, box_size, evol_shape, paint_shape, a_obs=None, curved_sky=True, dvel=0.,
                   ap_auto_=None, ap=None, cosmo_fid=None, **kw):
    """model.py:780-799: bias_oracle.observe_pos with the Alcock-Paczynski step between rsd and phys2cell_pos."""
    los, p = observe_phys(cosmo, pos, vel, box_center, R, box_size, evol_shape, a_obs, curved_sky, dvel)
    p = apply_ap(p, los, cosmo, curved_sky, ap_auto_, ap, cosmo_fid, **kw)
    return bo.phys2cell_pos(p, box_center, R, box_size, paint_shape)


def paint(cfg, pos_c, weights):
    """model.py:802-809: the weighted nufft of positions in cells of init_shape, with the Jacobian prod(init_shape / ptcl_shape), on paint_shape."""
    gxy = o.nufft(pos_c, cfg["init_shape"], tuple(cfg["paint_shape"]), weights=weights, paint_order=cfg["paint_order"],
                  interlace_order=cfg["interlace_order"], paint_deconv=cfg["paint_deconv"])
    gxy = gxy * np.divide(cfg["init_shape"], cfg["ptcl_shape"]).prod()
    gxy = o.chreshape(gxy, o.r2chshape(cfg["paint_shape"]))
    return o._irfftn(gxy, s=tuple(cfg["paint_shape"]), axes=(0, 1, 2))


def evolve_ap(cfg, cosmo, bias, white_mesh, ap_auto_=None, ap=None, cosmo_fid=None):
    """model.py:686-838 with ap_auto set, composed from bias_oracle.evolve's intermediates: its `pos` are the redshift-space
    positions in cells of init_shape (model.py:786, :799), so they go back to physical units, through the Alcock-Paczynski step with the
    line of sight of model.py:780 and on to the same nufft (model.py:802-809)."""
    ref, aux = bo.evolve(cfg, cosmo, bias, white_mesh)
    if ap_auto_ is None:
        return ref
    R = bo.rotvec_matrix(cfg["box_rotvec"])
    box, ctr = cfg["box_size"], cfg["box_center"]
    # the line of sight belongs to the positions BEFORE rsd; ap_auto / ap_param read it only on the flat sky, where it is constant
    los = o.safe_div(np.asarray(ctr, dtype=float), np.linalg.norm(ctr))
    p = bo.cell2phys_pos(aux["pos"], ctr, R, box, cfg["init_shape"])
    p = apply_ap(p, los, cosmo, cfg["curved_sky"], ap_auto_, ap, cosmo_fid)
    pos_c = bo.phys2cell_pos(p, ctr, R, box, cfg["init_shape"])
    return paint(cfg, pos_c, aux["weights"])


def log_density_ap(cfg, latents, fixed, sample, count_obs, make_cosmo, ap_auto_, cosmo_fid=None):
    """Single-feature restatement; the composed form is tests/_model_f64.py (whose host test keeps this one as an independent witness).
    bias_oracle.log_density (no selection, no mask, one radial bin) with the Alcock-Paczynski step inside evolve: the prior and
    white-field terms are its own, and its likelihood term (model.py:852-866, :893-908) is re-evaluated on `evolve_ap`'s mesh.
    alpha_iso / alpha_ap: latents (truncated normal, model.py:189-204) or fixed; a missing one is 1."""
    aux = {}
    lp = bo.log_density(cfg, latents, fixed, sample, count_obs, make_cosmo, aux=aux)
    base = aux["base"]
    final = tuple(cfg["final_shape"])

    def like(gxy):
        down = o._irfftn(o.chreshape(o._rfftn(gxy), o.r2chshape(final)), s=final, axes=(0, 1, 2))
        rcounts = np.atleast_1d(np.asarray(base["ngbars"], float)) * cfg["cell_length"] ** 3
        cm = bo.set_radial_count(down, bo.radius_mesh(cfg, final), bo.radial_edges(cfg, len(rcounts)), rcounts)
        selec = np.mean(rcounts)
        delta = cm / selec - 1
        scale1 = (np.abs(base["s_e"] + base["s_ed"] * delta) + 1e-9) * selec ** .5
        scale2 = base["s_e2"] * selec ** .5 * np.ones(final)
        return np.sum(bo.quad_gaussian_log_prob(np.asarray(count_obs), cm, scale1 * np.ones(final), scale2))
    ap = {k: base.get(k, 1.) for k in ("alpha_iso", "alpha_ap")}
    gxy = evolve_ap(cfg, make_cosmo(base), {k: base[k] for k in bo.BIAS_KEYS}, aux["white"], ap_auto_, ap, cosmo_fid)
    return float(lp - like(aux["gxy"]) + like(gxy))
