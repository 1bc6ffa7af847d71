"""Float64 numpy restatement of the Eulerian bias expansion (csrc/eulerian.hip, bricks.eulerian_bias; montecosmo/bricks.py:513-586) with a
hand-written VJP, and of `evolve` for bias_type 'eulerian' (model.py:753-754, :815-831) composed from the oracle's and tests/_png_f64.py's
pieces.  The checker of tests/test_eulerian_host.py and tests/test_gpu_eulerian.py; it never imports the library.  `dtype=np.float32` runs
the same mesh arithmetic in single precision on the CPU (float32 wavevectors, multipliers and real meshes, complex64 products, every
transform and every sum over cells in float64, as in tests/_bias_f64.py): the measure of what float32 can deliver.

With d = irfftn(X, zero mode dropped), h_ij = irfftn(k_i k_j / k^2 X), a = h00 - d/3, b = h11 - d/3, c = -(a + b), sig = <d^2>, mu = <phi d>:
  s2 = a^2 + b^2 + c^2 + 2 (h01^2 + h02^2 + h12^2)
  w  = 1 + b1E d + b2E (d^2 - sig) / 2 + bs2 (s2 - 2/3 sig) + bn2 irfftn(-k^2 X)  [+ bp phi + bpdE (phi d - mu), phi = irfftn(P)]
coef = (b1E, b2E, bs2, bn2, bp, bpdE).  Where the reference's unfinished branch is not followed literally (stated with their reference lines
in bricks.eulerian_bias): the weights mesh alone is the output; both paints carry prod(init_shape / ptcl_shape); bpdE = bpd + bp / 2;
b1E = 1 + b1, b2E = b2 + 8/21 b1 with the Lagrangian b1."""
import numpy as np

import _bias_f64 as bf

F64 = np.float64
HESS = ((0, 0), (1, 1), (0, 1), (0, 2), (1, 2))


def l2e(bias, png=None):
    """Lagrangian bias dict (and the products of fNL_bias) -> coef (b1E, b2E, bs2, bn2, bp, bpdE)."""
    b1, b2 = bias.get("b1", 0.), bias.get("b2", 0.)
    bp, bpd = (png.get("fNL_bp", 0.), png.get("fNL_bpd", 0.)) if png is not None else (0., 0.)
    return (1 + b1, b2 + 8 / 21 * b1, bias.get("bs2", 0.), bias.get("bn2", 0.), bp, bpd + bp / 2)


def _multipliers(shape, box, dtype):
    k = bf.kvec(shape, box, dtype)
    k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2]
    ik2 = np.where(k2 == 0, dtype(0), dtype(1) / np.where(k2 == 0, dtype(1), k2))
    return [np.ones_like(k2)] + [k[i] * k[j] * ik2 for i, j in HESS] + [-k2]


def fields(X, P, box, dtype=F64):
    """-> [d, h00, h11, h01, h02, h12, lap d] and phi (None without P), real meshes of `dtype`."""
    X = bf._c(X, dtype).copy()
    X[0, 0, 0] = 0
    shape = (X.shape[0], X.shape[1], 2 * (X.shape[2] - 1))
    M, sc = int(np.prod(shape)), dtype(1) / dtype(np.prod(shape))      # the 1 / M of the device's unnormalised C2R, a number of `dtype`
    real = lambda v: (M * bf._irfftn(bf._c(v, dtype), shape)).astype(dtype)
    f = [real((sc * m) * X) for m in _multipliers(shape, box, dtype)]
    return f, (None if P is None else real(sc * bf._c(P, dtype)))


def _shear(f, dtype):
    t = f[0] * dtype(1 / 3)
    a, b = f[1] - t, f[2] - t
    c = -(a + b)
    return a, b, c, a * a + b * b + c * c + dtype(2) * (f[3] * f[3] + f[4] * f[4] + f[5] * f[5])


def _terms(f, phi, dtype):
    """The six factors of coef, and the two moments (float64 means)."""
    d = f[0]
    sigma2 = float((d.astype(F64) ** 2).mean())
    spd = 0. if phi is None else float((phi.astype(F64) * d.astype(F64)).mean())
    sig, mu = dtype(sigma2), dtype(spd)
    s2 = _shear(f, dtype)[3] - dtype(2 / 3) * sig
    t = [d, (d * d - sig) * dtype(0.5), s2, f[6]]
    t += [np.zeros_like(d), np.zeros_like(d)] if phi is None else [phi, phi * d - mu]
    return t, (sigma2, spd)


def eulerian_bias(X, P, box, coef, dtype=F64):
    """Half-spectra X (matter), P (phi, or None) -> w (float64 array of `dtype` values), (<d^2>, <phi d>)."""
    f, phi = fields(X, P, box, dtype)
    t, mom = _terms(f, phi, dtype)
    B = [dtype(c) for c in coef]
    w = dtype(1) + B[0] * t[0]
    for k in (1, 2, 3) + (() if phi is None else (4, 5)):
        w = w + B[k] * t[k]
    return w.astype(F64), mom


def eulerian_terms(X, P, box, dtype=F64):
    """The six per-cell factors of coef (w is linear in coef: its cotangents are the sums of w_bar times these)."""
    f, phi = fields(X, P, box, dtype)
    return [np.asarray(x, dtype=F64) for x in _terms(f, phi, dtype)[0]]


def eulerian_bias_vjp(X, P, box, coef, wb, dtype=F64):
    """Cotangent wb of w -> X_bar, P_bar (None without P; real-pair convention, the zero mode of X_bar 0), coef_bar (6, float64)."""
    f, phi = fields(X, P, box, dtype)
    shape = f[0].shape
    M = f[0].size
    wb = np.asarray(wb, dtype=dtype)
    t, _ = _terms(f, phi, dtype)
    b1, b2, bs2, bn2, bp, bpd = (dtype(c) for c in coef)
    cbar = np.array([float((wb.astype(F64) * x.astype(F64)).sum()) for x in t])
    d = f[0]
    a, b, c, _ = _shear(f, dtype)
    sigbar = dtype(float((wb.astype(F64) * F64(-0.5 * b2 - 2 / 3 * bs2)).sum()))
    w2 = wb * bs2
    ab, bb = w2 * (dtype(2) * a - dtype(2) * c), w2 * (dtype(2) * b - dtype(2) * c)
    db = wb * (b1 + b2 * d) + sigbar * dtype(2) * d / dtype(M) - (ab + bb) * dtype(1 / 3)
    pb = None
    if phi is not None:
        mubar = dtype(float((-wb.astype(F64) * F64(bpd)).sum()))
        db = db + wb * bpd * phi + mubar * phi / dtype(M)
        pb = wb * (bp + bpd * d) + mubar * d / dtype(M)
    fb = [db, ab, bb, w2 * dtype(4) * f[3], w2 * dtype(4) * f[4], w2 * dtype(4) * f[5], wb * bn2]
    # adjoint of y = M irfftn(sc m X): sc zw m rfftn(y_bar), zw = 2 on the planes 0 < kz < nz / 2 that stand for their mirror images too
    zw = np.full(shape[2] // 2 + 1, 2.)
    zw[[0, -1]] = 1.
    sc = dtype(1) / dtype(M)
    back = lambda y: np.fft.rfftn(np.asarray(y, dtype=F64)) * zw
    Xb = sum((sc * m) * back(y) for m, y in zip(_multipliers(shape, box, dtype), fb))
    Xb[0, 0, 0] = 0
    return Xb, (None if pb is None else sc * back(pb)), cbar


def evolve(cfg, cosmo, bias, white_mesh, png=None, png_type=None):
    """model.py:686-838 for bias_type 'eulerian', evolution 'lpt' or 'nbody': the oracle's chain up to the observed positions (the
    Lagrangian weights are formed and dropped; dvel and phi are kept), then unweighted / phi-weighted paints and `eulerian_bias`."""
    from oracle import pm_oracle as o, bias_oracle as bo, power_oracle as po
    import _png_f64 as pf
    R = bo.rotvec_matrix(cfg["box_rotvec"])
    box, ctr = cfg["box_size"], cfg["box_center"]
    kpow = cfg["lin_kpow"] if cfg["lin_kpow"] is not None else po.lin_power_table(cosmo)
    init_mesh = bo.white2lin(cosmo.sigma8, white_mesh, cfg["init_shape"], box, kpow)
    init_mesh = o.chreshape(init_mesh, o.r2chshape(cfg["evol_shape"]))
    pos0 = o.regular_pos(cfg["evol_shape"], cfg["ptcl_shape"])
    _, a = bo.los_scalefactor_pos(pos0, ctr, R, box, cfg["evol_shape"], cosmo, cfg["a_obs"], cfg["curved_sky"])
    phi_pos = None
    if png_type is None:
        png = None
        _, dvel = bo.lagrangian_bias(o.a2g(cosmo, a), pos0, box, init_mesh, bias, read_order=1)
    else:
        png = pf.fNL_bias({k: (png or {}).get(k, 0.) for k in pf.PNG_KEYS}, bias, 1., png_type)
        table = pf.trans_table(cosmo)
        _, dvel, phi = pf.lagrangian_bias(table, o.a2g(cosmo, a), pos0, box, init_mesh, bias, png, read_order=1)
        phi_pos = o.read(pos0, phi, 1)                                                                  # model.py:754
        init_mesh = pf.add_png(table, png["fNL"], init_mesh, box)
        init_mesh = o.chreshape(o.chreshape(init_mesh, o.r2chshape(cfg["init_shape"])), o.r2chshape(cfg["evol_shape"]))
    cosmo._workspace = {}
    if cfg["evolution"] == "lpt":
        dpos, vel = o.lpt(cosmo, init_mesh, pos0, a, lpt_order=cfg["lpt_order"], read_order=1)
        pos = pos0 + dpos
    else:
        p, v = o.nbody_bf(cosmo, init_mesh, pos0, a0=cfg["nbody_a_start"], a1=a, n_steps=cfg["nbody_n_steps"],
                          paint_order=cfg["paint_order"], lpt_order=cfg["lpt_order"])
        pos, vel = p[-1], v[-1]
    pos_c = bo.observe_pos(cosmo, pos, vel, ctr, R, box, cfg["evol_shape"], cfg["init_shape"], cfg["a_obs"], cfg["curved_sky"], dvel)
    return painted_bias(cfg, pos_c, phi_pos, bias, png)


def painted_bias(cfg, pos_c, phi_pos, bias, png=None):
    """model.py:815-831: the unweighted and (phi_pos not None) the phi-weighted paint of positions in cells of init_shape, then
    `eulerian_bias` with the coefficients of `l2e`.  `png`: the products of fNL_bias (None without PNG)."""
    from oracle import pm_oracle as o
    box = cfg["box_size"]
    jac = np.divide(cfg["init_shape"], cfg["ptcl_shape"]).prod()
    kshape = o.r2chshape(cfg["paint_shape"])
    spec = lambda wts: o.chreshape(o.nufft(pos_c, cfg["init_shape"], tuple(cfg["paint_shape"]), weights=wts, paint_order=cfg["paint_order"],
                                           interlace_order=cfg["interlace_order"], paint_deconv=cfg["paint_deconv"]) * jac, kshape)
    mk = spec(1.)
    pk = None if phi_pos is None else spec(phi_pos)
    return eulerian_bias(mk, pk, box, l2e(bias, png))[0]
