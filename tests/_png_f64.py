"""Float64 numpy restatement of the primordial non-Gaussianity pieces of montecosmo/bricks.py, the checker of
tests/test_png_host.py and tests/test_gpu_png.py: `trans_phi2delta_interp` (bricks.py:108-127), `add_png` (bricks.py:129-141)
and the reparametrisation `b_phi` / `b_phi_delta` / `fNL_bias` (bricks.py:466-508).  Wavevectors, safe division, the growth
tables and the Eisenstein & Hu power table come from the oracle (read-only).  `dtype=np.float32` runs the same arithmetic in
single precision on the CPU (scipy.fft keeps float32): the measure of what float32 can deliver for a quantity with the 1/k^2 red spectrum of phi."""
import numpy as np
import scipy.fft

from oracle import background, pm_oracle as o, power_oracle as po

PNG_KEYS = ("fNL", "fNL_bp", "fNL_bpd", "fNL_bpd2", "fNL_bps2", "fNL_bn2p")


def trans_table(cosmo, a=1., kpow=None):
    """(ks, trans) of bricks.py:117-125.  kpow: (ks, pows normalised to sigma8 = 1) or None for Eisenstein & Hu; the power
    enters through a ratio, so its amplitude (sigma8^2, bricks.py:77) drops out and is not applied."""
    ks, pows = po.lin_power_table(cosmo) if kpow is None else kpow
    ks, pows = np.asarray(ks, dtype=np.float64), np.asarray(pows, dtype=np.float64)
    pow_large = ks ** cosmo.n_s
    lin_trans = np.sqrt(pows / pow_large / (pows[0] / pow_large[0]))
    a_md = 1. / (1. + 10.)
    growth_md = o.a2g(cosmo, a_md) / a_md
    return ks, 2. * background.rh ** 2 * ks ** 2 * lin_trans * (o.a2g(cosmo, a) / growth_md) / (3. * cosmo.Omega_m)


def kmesh(shape, box_size):
    kx, ky, kz = o.rfftk(tuple(int(s) for s in shape), np.asarray(box_size, dtype=np.float64))
    return np.sqrt((kx ** 2 + ky ** 2) + kz ** 2)


def trans_mesh(table, shape, box_size):
    """bricks.py:126: jnp.interp(|k|, ks, trans, left=0, right=0) on the half-spectrum mesh."""
    ks, trans = table
    return np.interp(kmesh(shape, box_size), ks, trans, left=0., right=0.)


def add_png(table, fNL, lin_mesh, box_size, dtype=np.float64, return_phi=False):
    """bricks.py:133-141 with the transfer table given explicitly (so that a test can move its entries)."""
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    lin_mesh = np.asarray(lin_mesh).astype(cdt)
    shape = o.ch2rshape(lin_mesh.shape)
    t = trans_mesh(table, shape, box_size).astype(dtype)
    phi0 = scipy.fft.irfftn(o.safe_div(lin_mesh, t).astype(cdt), s=shape).astype(dtype)
    phi2 = phi0 ** 2
    phi = phi0 + dtype(fNL) * (phi2 - phi2.mean(dtype=dtype))
    out = (t * scipy.fft.rfftn(phi).astype(cdt)).astype(cdt)
    return (out, phi0) if return_phi else out


def bpd_L2E(bpd, bp):
    return bpd + bp / 2          # bricks.py:466-467


def bpd_E2L(bpd, bp):
    return bpd - bp / 2          # bricks.py:469-470


def b_phi(b1, p=1., delta_c=1.686):
    return 2 * delta_c * (b1 + 1 - p)          # bricks.py:481


def b_phi_delta(b1, b2, delta_c=1.686):
    return 2 * (delta_c * b2 - b1)          # bricks.py:491


def fNL_bias(png, bias, p=1., png_type=None):
    """bricks.py:493-508 on a copy."""
    png = dict(png)
    if png_type == "fNL":
        png["fNL_bp"] = png["fNL"] * b_phi(bias["b1"], p)
        png["fNL_bpd"] = png["fNL"] * b_phi_delta(bias["b1"], bias["b2"])
    elif png_type == "bias":
        png["fNL_bp"] = png["fNL"] * png["fNL_bp"]
        png["fNL_bpd"] = png["fNL"] * png["fNL_bpd"]
    return png


# ---- PNG block of lagrangian_bias (bricks.py:413-441), the Kaiser boost term (bricks.py:181-183) and a PNG-enabled evolve
# (model.py:686-838), composed with the oracle's Gaussian pieces (imported read-only)
def png_fields(table, lin_mesh, box_size):
    """phi = irfftn(safe_div(lin, t)) and irfftn(-k^2 safe_div(lin, t)) (bricks.py:415, :439)."""
    shape = o.ch2rshape(np.shape(lin_mesh))
    u = o.safe_div(np.asarray(lin_mesh, dtype=np.complex128), trans_mesh(table, shape, box_size))
    return o._irfftn(u, s=shape, axes=(0, 1, 2)), o._irfftn(-kmesh(shape, box_size) ** 2 * u, s=shape, axes=(0, 1, 2))


def png_terms(table, growths, pos, box_size, lin_mesh, read_order=2):
    """The five per-particle factors of fNL_bp, fNL_bpd, fNL_bpd2, fNL_bps2, fNL_bn2p (bricks.py:418-441) and phi."""
    from oracle import bias_oracle as bo
    fld, _ = bo.bias_fields(np.asarray(lin_mesh, dtype=np.complex128), box_size)
    gs = np.asarray(growths, dtype=float).squeeze()
    d = o.read(pos, fld["delta"], read_order) * gs
    sigma2 = (d ** 2).mean()
    d2 = d ** 2 - sigma2                                                 # bricks.py:365-368
    s2 = o.read(pos, fld["shear2"], read_order) * gs ** 2 - 2 / 3 * sigma2      # bricks.py:387-389
    phi, lap = png_fields(table, lin_mesh, box_size)
    p = o.read(pos, phi, read_order)
    spd = (p * d).mean()
    return [p, p * d - spd, p * d2 - 2 * spd * d, p * s2, o.read(pos, lap, read_order)], phi


PNG5 = PNG_KEYS[1:]


def lagrangian_bias(table, growths, pos, box_size, lin_mesh, bias, png, read_order=2):
    """bricks.py:327-443 with png_type set: the oracle's Gaussian weights plus the five PNG terms.  Returns (w, dvel, phi)."""
    from oracle import bias_oracle as bo
    w, dvel = bo.lagrangian_bias(growths, pos, box_size, lin_mesh, bias, read_order)
    terms, phi = png_terms(table, growths, pos, box_size, lin_mesh, read_order)
    return w + sum(png.get(k, 0.) * t for k, t in zip(PNG5, terms)), dvel, phi


def evolve(cfg, cosmo, bias, white_mesh, png, png_type):
    """model.py:686-838 with png_type set: fNL_bias -> bias weights on the Gaussian mesh -> add_png -> chreshape to init_shape and
    back -> lpt / nbody -> observe -> paint (the oracle's composition, oracle/bias_oracle.py::evolve, with the PNG steps put in).
    The transfer table of the lpt / nbody path is Eisenstein & Hu (model.py:751, :757 pass no kpow), Kaiser's follows lin_kpow."""
    from oracle import bias_oracle as bo
    png = fNL_bias({k: png.get(k, 0.) for k in PNG_KEYS}, bias, 1., png_type)
    R = bo.rotvec_matrix(cfg["box_rotvec"])
    box, ctr = cfg["box_size"], cfg["box_center"]
    kpow = cfg["lin_kpow"] if cfg["lin_kpow"] is not None else po.lin_power_table(cosmo)
    init_mesh = bo.white2lin(cosmo.sigma8, white_mesh, cfg["init_shape"], box, kpow)
    init_mesh = o.chreshape(init_mesh, o.r2chshape(cfg["evol_shape"]))
    es = tuple(cfg["evol_shape"])
    if cfg["evolution"] == "kaiser":
        c = np.asarray(ctr, float)
        los = R.T @ o.safe_div(c, np.linalg.norm(c))
        boost = bo.kaiser_boost(cosmo, cfg["a_obs"], es, box, 1. + bias["b1"], los)
        boost = boost + o.safe_div(png["fNL_bp"], trans_mesh(trans_table(cosmo, kpow=cfg["lin_kpow"]), es, box))      # bricks.py:181-183
        cosmo._workspace = {}
        return 1. + o._irfftn(init_mesh * boost, s=es, axes=(0, 1, 2))
    table = trans_table(cosmo)
    pos = o.regular_pos(cfg["evol_shape"], cfg["ptcl_shape"])
    _, a = bo.los_scalefactor_pos(pos, ctr, R, box, cfg["evol_shape"], cosmo, cfg["a_obs"], cfg["curved_sky"])
    w, dvel, _ = lagrangian_bias(table, o.a2g(cosmo, a), pos, box, init_mesh, bias, png, read_order=1)
    init_mesh = add_png(table, png["fNL"], init_mesh, box)
    init_mesh = o.chreshape(o.chreshape(init_mesh, o.r2chshape(cfg["init_shape"])), o.r2chshape(cfg["evol_shape"]))      # model.py:758
    cosmo._workspace = {}
    if cfg["evolution"] == "lpt":
        dpos, vel = o.lpt(cosmo, init_mesh, pos, a, lpt_order=cfg["lpt_order"], read_order=1)
        pos = pos + dpos
    else:
        p, v = o.nbody_bf(cosmo, init_mesh, pos, a0=cfg["nbody_a_start"], a1=a, n_steps=cfg["nbody_n_steps"],
                          paint_order=cfg["paint_order"], lpt_order=cfg["lpt_order"])
        pos, vel = p[-1], v[-1]
    pos_c = bo.observe_pos(cosmo, pos, vel, ctr, R, box, cfg["evol_shape"], cfg["init_shape"], cfg["a_obs"], cfg["curved_sky"], dvel)
    gxy = o.nufft(pos_c, cfg["init_shape"], tuple(cfg["paint_shape"]), weights=w, paint_order=cfg["paint_order"],
                  interlace_order=cfg["interlace_order"], paint_deconv=cfg["paint_deconv"])
    gxy = o.chreshape(gxy * np.divide(cfg["init_shape"], cfg["ptcl_shape"]).prod(), o.r2chshape(cfg["paint_shape"]))
    return o._irfftn(gxy, s=tuple(cfg["paint_shape"]), axes=(0, 1, 2))
