"""Float64 numpy restatement of the reference's chain start, the checker of tests/test_kaiser_post_host.py and
tests/test_gpu_kaiser_post.py: `count2delta` (montecosmo/bricks.py:927-937; model.py:1271-1285), `kaiser_posterior` (bricks.py:234-247),
`lin2white` (bricks.py:159-164), `trunc2std` (utils.py:229-264), the inverse reparametrisation (bricks.py:255-287, :310-318 with inv=True)
and `FieldLevelModel.kaiser_post` (model.py:1444-1477) that chains them.  The Fourier-layout helpers (rg2cgh, cgh2rg, chreshape), the
growth functions and the fiducial scale factor are the oracle's."""
import numpy as np
from scipy.special import logsumexp, ndtr, ndtri

from oracle import background as obg, bias_oracle as bo, pm_oracle as o

TAIL_TEMP = 1 / 6.2842226 / 2      # utils.py:247, :252
TAIL_LIM = 12                      # utils.py:261


# --------------------------------------------------------------------------- pieces
def count2delta(mesh, selec_mesh):
    """bricks.py:936-937."""
    mesh, selec_mesh = np.asarray(mesh, dtype=np.float64), np.asarray(selec_mesh, dtype=np.float64)
    alpha_selec = selec_mesh * mesh.mean() / selec_mesh.mean()
    return (mesh - alpha_selec) / (alpha_selec ** 2).mean() ** .5


def kaiser_posterior(delta_obs, cosmo, a, box_size, var_noise, b1E, los, sigma8, kpow):
    """bricks.py:239-247 with a tabulated power (normalised to sigma8 = 1)."""
    mesh_shape = o.ch2rshape(delta_obs.shape)
    pmesh = bo.lin_power_mesh(sigma8, mesh_shape, box_size, kpow)
    pmesh = pmesh * np.divide(mesh_shape, box_size).prod()      # power in cell units
    boost = bo.kaiser_boost(cosmo, a, mesh_shape, box_size, b1E, los)
    stds = (pmesh / (1 + boost ** 2 / var_noise * pmesh)) ** .5
    means = stds ** 2 * boost / var_noise * delta_obs
    return means, stds


def lin2white(sigma8, lin_mesh, init_shape, box_size, kpow):
    """bricks.py:163-164: safe_div by the square root of the PHYSICAL power."""
    pmesh = bo.lin_power_mesh(sigma8, init_shape, box_size, kpow)
    return o.safe_div(lin_mesh, pmesh ** .5)


def trunc2std(y, loc=0., scale=1., low=-np.inf, high=np.inf):
    """utils.py:231-264, one number at a time."""
    y, low, high = (y - loc) / scale, (low - loc) / scale, (high - loc) / scale
    if y < -TAIL_LIM and low < -TAIL_LIM:      # invlowtail
        return float(TAIL_TEMP * logsumexp(np.array([y, low]) / TAIL_TEMP, b=np.array([1., -1.])))
    if TAIL_LIM < y and TAIL_LIM < high:       # invhightail
        return float(-TAIL_TEMP * logsumexp(-np.array([y, high]) / TAIL_TEMP, b=np.array([1., -1.])))
    if y < 0.:                                 # invlowbody
        cdf_low, cdf_high = ndtr(low), ndtr(high)
        return float(ndtri((ndtr(y) - cdf_low) / (cdf_high - cdf_low)))
    cdf_nlow, cdf_nhigh = ndtr(-low), ndtr(-high)      # invhighbody
    return float(-ndtri((cdf_nhigh - ndtr(-y)) / (cdf_nhigh - cdf_nlow)))


def _conf(c):
    """A latent's config with the defaults of model.py:1081-1084 (uniform: loc_fid, scale_fid from the bounds)."""
    c = {k: v for k, v in c.items() if v is not None}
    low, high = c.get("low", -np.inf), c.get("high", np.inf)
    if "loc" not in c or "scale" not in c:
        c.setdefault("loc_fid", (low + high) / 2)
        c.setdefault("scale_fid", (high - low) / 12 ** .5)
    return dict(c, low=low, high=high)


def base2sample(y, c):
    """bricks.py:277-283 for one latent: trunc2std when a bound is finite, else the affine inverse; arrays element by element."""
    c = _conf(c)
    y = np.asarray(y, dtype=np.float64)
    lf, sf, lo, hi = (np.broadcast_to(np.asarray(c[k], dtype=np.float64), y.shape) for k in ("loc_fid", "scale_fid", "low", "high"))
    if np.any(lo != -np.inf) or np.any(hi != np.inf):
        out = np.array([trunc2std(*v) for v in zip(y.reshape(-1), lf.reshape(-1), sf.reshape(-1), lo.reshape(-1), hi.reshape(-1))])
        return out.reshape(y.shape) if y.ndim else float(out[0])
    out = (y - lf) / sf
    return out if y.ndim else float(out)


def fiducial(latents, fixed):
    """model.py:1214-1223: loc_fid of the latents, else the fixed value."""
    fid = dict(fixed)
    fid.update({k: _conf(v)["loc_fid"] for k, v in latents.items()})
    return fid


def selec_fid(cfg):
    sel = cfg.get("selec_mesh")
    return 1.0 if sel is None else float((np.asarray(sel, dtype=np.float64) ** 2).mean() ** .5 / np.asarray(sel, dtype=np.float64).mean())


def observed_delta(cfg, count_obs):
    """model.py:1271-1285 on the final mesh: masked counts, the selection brought to the final mesh and masked when its shape differs."""
    final = tuple(cfg["final_shape"])
    mask = np.ones(final, bool) if cfg.get("mask_mesh") is None else np.asarray(cfg["mask_mesh"], bool)
    mesh = np.where(mask, np.asarray(count_obs, dtype=np.float64), 0.)
    sel = cfg.get("selec_mesh")
    if sel is None:
        selec = np.float64(1.)
    elif tuple(np.shape(sel)) != final:
        selec = o._irfftn(o.chreshape(o._rfftn(np.asarray(sel, dtype=np.float64)), o.r2chshape(final)), s=final, axes=(0, 1, 2))
        selec = np.where(mask, selec, 0.)
    else:
        selec = np.asarray(sel, dtype=np.float64)
    return count2delta(mesh, selec)


def los_fid(cfg):
    c = np.asarray(cfg["box_center"], dtype=np.float64)
    return bo.rotvec_matrix(cfg["box_rotvec"]).T @ o.safe_div(c, np.linalg.norm(c))


def kpow_of(cfg, cosmo):
    if cfg["lin_kpow"] is not None:
        return cfg["lin_kpow"]
    from oracle import power_oracle
    return power_oracle.lin_power_table(cosmo)


# --------------------------------------------------------------------------- the chain
def posterior_moments(cfg, latents, fixed, count_obs, make_cosmo):
    """(means, stds, fid, cosmo_fid): model.py:1451-1460."""
    init = tuple(cfg["init_shape"])
    fid = fiducial(latents, fixed)
    cosmo_fid = make_cosmo(fid)
    delta_obs = o.chreshape(o._rfftn(observed_delta(cfg, count_obs)), o.r2chshape(init))
    count_fid = float(np.mean(fid["ngbars"])) * cfg["cell_length"] ** 3
    var_fid = fid["s_e"] / (count_fid * selec_fid(cfg))
    a_fid = bo.fiducial_scale_factor(cfg, cosmo_fid)
    means, stds = kaiser_posterior(delta_obs, cosmo_fid, a_fid, cfg["box_size"], var_fid, 1. + fid["b1"], los_fid(cfg), fid["sigma8"],
                                   kpow_of(cfg, cosmo_fid))
    return means, stds, fid, cosmo_fid


def white2sample(cfg, latents, fixed, white, make_cosmo):
    """bricks.py:310-318: safe_div by the transfer, then cgh2rg ('fourier', 'kaiser') or irfftn ('real')."""
    fid = fiducial(latents, fixed)
    _, transfer = bo.precond_scale_and_transfer(cfg, fid, make_cosmo(fid) if cfg["precond"] == "kaiser" else None)
    mesh = o.safe_div(white, transfer * np.ones(white.shape))
    if cfg["precond"] == "real":
        return o._irfftn(mesh, s=tuple(cfg["init_shape"]), axes=(0, 1, 2))
    return o.cgh2rg(mesh)


def kaiser_post(cfg, latents, fixed, count_obs, noise, make_cosmo, temp=1., scale_field=1., base=False):
    """model.py:1444-1477 with the unit normal real mesh `noise` (init_shape) given.  Returns the start values of every sampled latent: the
    fiducial scalars and 'white_mesh' (base=True), or their sample-space values and 'white_mesh_'."""
    init = tuple(cfg["init_shape"])
    means, stds, fid, cosmo_fid = posterior_moments(cfg, latents, fixed, count_obs, make_cosmo)
    post = temp ** .5 * stds * o.rg2cgh(np.asarray(noise, dtype=np.float64)) + means
    post = lin2white(fid["sigma8"], post, init, cfg["box_size"], kpow_of(cfg, cosmo_fid)) * scale_field
    start = {k: fid[k] for k in latents}
    if base:
        return dict(start, white_mesh=post)
    out = {k + "_": base2sample(v, latents[k]) for k, v in start.items()}
    out["white_mesh_"] = white2sample(cfg, latents, fixed, post, make_cosmo)
    return out


# --------------------------------------------------------------------------- self check
def self_check():
    """Known answers of the pieces, independent of any device code."""
    rng = np.random.default_rng(0)
    # count2delta: a scalar selection gives (mesh - mean) / mean; a mesh selection the closed form of bricks.py:931-934
    mesh = rng.uniform(1., 9., (6, 4, 8))
    assert np.allclose(count2delta(mesh, 1.), (mesh - mesh.mean()) / mesh.mean(), rtol=1e-14, atol=0)
    sel = rng.uniform(.2, 1., mesh.shape)
    closed = (mesh / mesh.mean() - sel / sel.mean()) / ((sel / sel.mean()) ** 2).mean() ** .5
    assert np.allclose(count2delta(mesh, sel), closed, rtol=1e-13, atol=1e-15)
    # trunc2std inverts the oracle's std2trunc on the body and on both tails
    for x, lo, hi in [(0.3, -5., 3.), (-2., -1., np.inf), (1.5, -np.inf, 2.), (-13., -20., 5.), (14., -3., 30.)]:
        y = bo.std2trunc(x, 0.3, 0.01, 0.3 + 0.01 * lo, 0.3 + 0.01 * hi)
        assert abs(trunc2std(y, 0.3, 0.01, 0.3 + 0.01 * lo, 0.3 + 0.01 * hi) - x) < 1e-9 * max(1., abs(x)), (x, lo, hi)
    # kaiser_posterior: Wiener filter limits; lin2white inverts white2lin where P > 0 and gives 0 elsewhere
    ks = np.logspace(-2, 0, 64)
    kpow = (ks, 1e4 * ks / (1 + (ks / 0.05) ** 2.5))
    shape, box = (8, 6, 4), np.array([400., 300., 200.])
    cosmo = obg.Planck18()
    d = o._rfftn(rng.standard_normal(shape))
    means, stds = kaiser_posterior(d, cosmo, 0.7, box, 1e-12, 2., np.array([0., 0., 1.]), 0.8, kpow)
    boost = bo.kaiser_boost(cosmo, 0.7, shape, box, 2., np.array([0., 0., 1.]))
    p = bo.lin_power_mesh(0.8, shape, box, kpow)
    assert np.allclose(means[p > 0], (d / boost)[p > 0], rtol=1e-6)      # no noise: the observed field divided by the boost
    assert np.all(stds[p == 0] == 0) and np.all(means[p == 0] == 0)
    _, stds_prior = kaiser_posterior(d, cosmo, 0.7, box, 1e30, 2., np.array([0., 0., 1.]), 0.8, kpow)
    assert np.allclose(stds_prior ** 2, p * np.divide(shape, box).prod(), rtol=1e-12)      # all noise: the prior
    w = o.rg2cgh(rng.standard_normal(shape))
    back = lin2white(0.8, bo.white2lin(0.8, w, shape, box, kpow), shape, box, kpow)
    assert np.allclose(back[p > 0], w[p > 0], rtol=1e-13) and np.all(back[p == 0] == 0) and (p == 0).any()
    return True


if __name__ == "__main__":
    print("self_check", self_check())
