"""Float64 numpy restatement of the per-particle formulas of csrc/bias.hip and csrc/png.hip (Lagrangian bias weights, their PNG terms, the
light-cone LPT combination) with hand-written gradients, and of the mesh-side multipliers (bias fields, power multiplier, PNG potential,
add_png) for any nx, ny >= 2 and even nz.  The checker of tests/test_bias_f64_host.py, tests/test_gpu_reductions_ragged.py and
tests/test_gpu_model_mesh_odd.py; it never imports the library.  `dtype=np.float32` runs the same arithmetic in single precision on the CPU:
the measure of what float32 can deliver.  Sums over particles are always float64, as on the device, so a deviation measures the
per-particle arithmetic and not a summation order; `terms=True` also returns the per-particle integrands of every sum.  On the mesh side
`dtype=np.float32` means float32 wavevectors and multipliers (the 1 / M of the device's unnormalised C2R among them), complex64 products and
float32 real meshes, with every transform in float64.

Particle side, with g = growth (scalar or one per particle), d = dr g, sig = <d^2> (mean over the n particles), S2 = s2r g^2 - 2/3 sig:
  w    = 1 + b1 d + b2 (d^2 - sig) / 2 + bs2 S2 + b3 (d^3 - 3 sig d) / 6 + bds2 d S2 + bs3 s3r g^3 + bn2 lr g,     dvel = bnpar g gr
  PNG: w += bp ph + bpd (ph d - spd) + bpd2 (ph (d^2 - sig) - 2 spd d) + bps2 ph S2 + bn2p lp,     spd = <ph d>
  LPT: dpos = g F1 - g2 F2,  vel = F1 - c F2,   (g, g2, c) = gt[:, 0..2]"""
import numpy as np

F64 = np.float64


def _growth(g, n, dtype):
    g = np.asarray(g, dtype=dtype)
    return g if g.ndim == 0 else g.reshape(n)


def _cast(dtype, *arrs):
    return [np.asarray(a, dtype=dtype) for a in arrs]


def _dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


# ---- Lagrangian bias weights -------------------------------------------------------------------------------------------------------
def bias_weights(dr, s2r, s3r, lr, gr, g, bias8, dtype=F64, terms=False):
    """-> w (n), dvel (n, 3), sigma2 (float64) [, {'sigma2': per-particle integrand of sigma2}]."""
    dr, s2r, s3r, lr, gr = _cast(dtype, dr, s2r, s3r, lr, gr)
    n = dr.shape[0]
    g = _growth(g, n, dtype)
    b1, b2, bs2, b3, bds2, bs3, bn2, bnpar = (dtype(b) for b in bias8)
    d = dr * g
    mom = d.astype(F64) ** 2 / n
    sigma2 = float(mom.sum())
    sig = dtype(sigma2)
    s2, s3, l = s2r * g * g - dtype(2 / 3) * sig, s3r * g * g * g, lr * g
    w = dtype(1) + b1 * d
    w = w + b2 * (d * d - sig) * dtype(0.5)
    w = w + bs2 * s2
    w = w + b3 * (d * d * d - dtype(3) * sig * d) * dtype(1 / 6)
    w = w + bds2 * d * s2
    w = w + bs3 * s3
    w = w + bn2 * l
    dvel = (bnpar * g * np.ones(n, dtype=dtype))[:, None] * gr
    return (w, dvel, sigma2, dict(sigma2=mom)) if terms else (w, dvel, sigma2)


def bias_weights_vjp(dr, s2r, s3r, lr, gr, g, bias8, wb, vb, dtype=F64, terms=False):
    """Cotangents (wb (n), vb (n, 3)) of (w, dvel) -> drb, s2rb, s3rb, lrb (n), grb (n, 3), gbar (n: per-particle cotangent of g), the 8
    bias cotangents (float64) and the summed growth cotangent (float64) [, {'scalars': (9, n) integrands of the 8 bias cotangents and of the
    summed growth cotangent, 'sigma2': integrand of sigma2}]."""
    dr, s2r, s3r, lr, gr, wb, vb = _cast(dtype, dr, s2r, s3r, lr, gr, wb, vb)
    n = dr.shape[0]
    g = _growth(g, n, dtype)
    b1, b2, bs2, b3, bds2, bs3, bn2, bnpar = (dtype(b) for b in bias8)
    d = dr * g
    mom = d.astype(F64) ** 2 / n
    sig = dtype(mom.sum())
    s2, s3, l = s2r * g * g - dtype(2 / 3) * sig, s3r * g * g * g, lr * g
    dw_ds2 = bs2 + bds2 * d
    vg = _dot3(vb, gr)
    t = [wb * d, wb * (d * d - sig) * dtype(0.5), wb * s2, wb * (d * d * d - dtype(3) * sig * d) * dtype(1 / 6), wb * d * s2, wb * s3, wb * l,
         g * vg, wb * (dtype(-0.5) * b2 - dtype(0.5) * b3 * d - dtype(2 / 3) * dw_ds2)]
    t = np.stack([np.asarray(x, dtype=F64) * np.ones(n) for x in t])
    sums = t.sum(1)
    sigbar = dtype(sums[8])      # every particle feeds <d^2>: its cotangent comes back to each one as sigbar * 2 d / n
    dbar = wb * (b1 + b2 * d + b3 * (d * d - sig) * dtype(0.5) + bds2 * s2) + sigbar * dtype(2) * d / dtype(n)
    drb = dbar * g
    s2rb = wb * dw_ds2 * g * g
    s3rb = wb * bs3 * g * g * g
    lrb = wb * bn2 * g
    grb = (bnpar * g * np.ones(n, dtype=dtype))[:, None] * vb
    gbar = dbar * dr + wb * dw_ds2 * dtype(2) * g * s2r + wb * bs3 * dtype(3) * g * g * s3r + wb * bn2 * lr + bnpar * vg
    gcell = gbar.astype(F64)
    out = (drb, s2rb, s3rb, lrb, grb, gbar, sums[:8].copy(), float(gcell.sum()))
    return out + (dict(scalars=np.concatenate([t[:8], gcell[None]]), sigma2=mom),) if terms else out


# ---- PNG terms of the weights ------------------------------------------------------------------------------------------------------
def _png_terms(dr, s2r, ph, lp, g, dtype):
    n = dr.shape[0]
    d = dr * g
    mom = np.stack([d.astype(F64) ** 2, (ph * d).astype(F64)]) / n
    sig, spd = dtype(mom[0].sum()), dtype(mom[1].sum())
    D2, S2 = d * d - sig, s2r * g * g - dtype(2 / 3) * sig
    return d, D2, S2, [ph, ph * d - spd, ph * D2 - dtype(2) * spd * d, ph * S2, lp], sig, spd, mom


def png_weights(dr, s2r, ph, lp, g, png5, w, dtype=F64, terms=False):
    """-> w + the five PNG terms (n), moments = (<d^2>, <ph d>) (float64) [, {'moments': (2, n) integrands}]."""
    dr, s2r, ph, lp, w = _cast(dtype, dr, s2r, ph, lp, w)
    g = _growth(g, dr.shape[0], dtype)
    B = [dtype(b) for b in png5]
    _, _, _, t, _, _, mom = _png_terms(dr, s2r, ph, lp, g, dtype)
    out = w + (B[0] * t[0] + B[1] * t[1] + B[2] * t[2] + B[3] * t[3] + B[4] * t[4])
    return (out, mom.sum(1), dict(moments=mom)) if terms else (out, mom.sum(1))


def png_weights_vjp(dr, s2r, ph, lp, g, png5, wb, drb=0., s2rb=0., gbar=0., dtype=F64, terms=False):
    """Cotangent wb (n) of the weights -> drb, s2rb, gbar with the PNG terms' share ADDED (they come in holding the Gaussian terms'), phb,
    lpb (n), the 5 coefficient cotangents, <ph d>_bar, <d^2>_bar and the summed growth cotangent of the PNG terms alone (float64)
    [, {'scalars': (8, n) integrands in that order, 'moments': (2, n)}]."""
    dr, s2r, ph, lp, wb = _cast(dtype, dr, s2r, ph, lp, wb)
    n = dr.shape[0]
    drb, s2rb, gbar = (np.asarray(a, dtype=dtype) * np.ones(n, dtype=dtype) for a in (drb, s2rb, gbar))
    g = _growth(g, n, dtype)
    bp, bpd, bpd2, bps2, bn2p = (dtype(b) for b in png5)
    d, D2, S2, t, sig, spd, mom = _png_terms(dr, s2r, ph, lp, g, dtype)
    c = [wb * x for x in t] + [wb * (-bpd - dtype(2) * bpd2 * d), wb * ph * (-bpd2 - dtype(2 / 3) * bps2)]
    c = np.stack([np.asarray(x, dtype=F64) for x in c])
    sums = c.sum(1)
    spdb, sigb = dtype(sums[5] / n), dtype(sums[6] / n)      # the two means couple all particles
    phb = wb * (bp + bpd * d + bpd2 * D2 + bps2 * S2) + spdb * d
    lpb = wb * bn2p * np.ones(n, dtype=dtype)
    dbar = wb * (bpd * ph + dtype(2) * bpd2 * (ph * d - spd)) + spdb * ph + sigb * dtype(2) * d
    s2b = wb * bps2 * ph
    gb = dbar * dr + s2b * dtype(2) * g * s2r
    gcell = gb.astype(F64)
    out = (drb + dbar * g, s2rb + s2b * g * g, phb, lpb, gbar + gb, sums[:5].copy(), float(sums[5]), float(sums[6]), float(gcell.sum()))
    return out + (dict(scalars=np.concatenate([c, gcell[None]]), moments=mom),) if terms else out


# ---- light-cone LPT combination ----------------------------------------------------------------------------------------------------
def lpt_combine(F1, F2, gt, dtype=F64):
    """F1, F2 (n, 3) (F2 may be None), gt (n, 3) = (g, g2, c) -> dpos, vel."""
    F1, gt = _cast(dtype, F1, gt)
    F2 = np.zeros_like(F1) if F2 is None else np.asarray(F2, dtype=dtype)
    return gt[:, :1] * F1 - gt[:, 1:2] * F2, F1 - gt[:, 2:3] * F2


def lpt_combine_vjp(F1, F2, gt, xb, vb, dtype=F64):
    """Cotangents (xb, vb) of (dpos, vel) -> F2_bar, F1_bar, gt_bar (n, 3)."""
    F1, gt, xb, vb = _cast(dtype, F1, gt, xb, vb)
    F2 = np.zeros_like(F1) if F2 is None else np.asarray(F2, dtype=dtype)
    gtb = np.stack([_dot3(xb, F1), -_dot3(xb, F2), -_dot3(vb, F2)], axis=-1)
    return -gt[:, 1:2] * xb - gt[:, 2:3] * vb, gt[:, :1] * xb + vb, gtb


# ---- mesh side: any nx, ny; nz even -------------------------------------------------------------------------------------------------
def kvec(shape, box, dtype=F64):
    """k = 2 pi fftfreq(n) n / box per axis (h/Mpc), broadcastable over the half-spectrum; an odd axis has no Nyquist entry."""
    out = []
    for ax, (n, b) in enumerate(zip(shape, box)):
        s = np.fft.rfftfreq(n) * n if ax == 2 else np.fft.fftfreq(n) * n      # signed integer wave numbers
        k = dtype(2 * np.pi) * s.astype(dtype) / dtype(n) * dtype(n / b)      # (2 pi s / n) * kphys, kphys = n / box as the ABI's float
        sh = [1, 1, 1]
        sh[ax] = -1
        out.append(k.reshape(sh))
    return out


def kabs(shape, box, dtype=F64):
    """|k| in float64 from components of `dtype` (what the table look-ups inside the kernels see)."""
    k = [c.astype(F64) for c in kvec(shape, box, dtype)]
    return np.sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2])


def _c(X, dtype):
    return np.asarray(X).astype(np.complex128 if dtype == F64 else np.complex64)


def _irfftn(X, shape):
    """numpy's irfftn keeps the Hermitian part of the kz = 0 and kz = nz/2 planes: the projection the kernels restate."""
    return np.fft.irfftn(np.asarray(X, dtype=np.complex128), s=tuple(shape), axes=(0, 1, 2))


def bias_fields(X, box, dtype=F64):
    """Half-spectrum X -> (fields7, hess6): fields7 = {delta, shear^2, 3 det shear, laplacian delta, grad x, y, z}, hess6 = {delta, h00, h11,
    h01, h02, h12} with h_ij = d_i d_j laplace^-1 delta (what mcpm_bias_fields_save_f32 keeps)."""
    X = _c(X, dtype)
    shape = (X.shape[0], X.shape[1], 2 * (X.shape[2] - 1))
    k = kvec(shape, box, dtype)
    k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2]
    ik2 = np.where(k2 == 0, dtype(0), dtype(1) / np.where(k2 == 0, dtype(1), k2))
    # the device's C2R is unnormalised: the multipliers carry 1 / M, a number of `dtype` like the rest of them (1.f / (float)M in the kernels)
    M, sc = int(np.prod(shape)), dtype(1) / dtype(np.prod(shape))
    real = lambda m: (M * _irfftn(_c((sc * m) * X, dtype), shape)).astype(dtype)
    h = [real(np.ones_like(k2))] + [real(k[i] * k[j] * ik2) for i, j in ((0, 0), (1, 1), (0, 1), (0, 2), (1, 2))]
    t = h[0] * dtype(1 / 3)
    a, b = h[1] - t, h[2] - t
    c = -(a + b)
    d, e, f = h[3], h[4], h[5]
    s2 = a * a + b * b + c * c + dtype(2) * (d * d + e * e + f * f)
    s3 = dtype(3) * (a * (b * c - f * f) - d * (d * c - e * f) + e * (d * f - b * e))
    rest = [real(-k2)] + [real(1j * k[i].astype(X.dtype)) for i in range(3)]
    return np.stack([h[0], s2, s3] + rest).astype(F64), np.stack(h).astype(F64)


def _interp0(x, xp, fp):
    return np.interp(x, xp, fp, left=0., right=0.)


def power_mult(X, box, ks, pows, amp, dtype=F64):
    """X sqrt(amp P(|k|)), P linear in the table and zero outside it."""
    X = _c(X, dtype)
    shape = (X.shape[0], X.shape[1], 2 * (X.shape[2] - 1))
    t = np.sqrt(amp * _interp0(kabs(shape, box, dtype), ks, pows)).astype(dtype)
    return _c(t * X, dtype).astype(np.complex128)


def png_phi(table, X, box, dtype=F64):
    """-> phi = irfftn(safe_div(X, t)), lap phi = irfftn(-k^2 safe_div(X, t)); t = 0 outside the table."""
    X = _c(X, dtype)
    shape = (X.shape[0], X.shape[1], 2 * (X.shape[2] - 1))
    k = kabs(shape, box, dtype)
    t = _interp0(k, *table).astype(dtype)
    u = _c(np.where(t == 0, 0, X / np.where(t == 0, dtype(1), t)), dtype)
    M, sc = int(np.prod(shape)), dtype(1) / dtype(np.prod(shape))      # 1 / M of the unnormalised C2R, applied in `dtype` as in png_div_kernel
    mk2 = sc * (-(k * k)).astype(dtype)
    real = lambda v: (M * _irfftn(_c(v, dtype), shape)).astype(dtype).astype(F64)
    return real(sc * u), real(mk2 * u)


def add_png(table, fNL, X, box, dtype=F64):
    """-> t rfftn(phi + fNL (phi^2 - <phi^2>)), <phi^2> (float64 mean)."""
    X = _c(X, dtype)
    shape = (X.shape[0], X.shape[1], 2 * (X.shape[2] - 1))
    t = _interp0(kabs(shape, box, dtype), *table).astype(dtype)
    phi = png_phi(table, X, box, dtype)[0].astype(dtype)
    mean = float((phi.astype(F64) ** 2).mean())
    psi = phi + dtype(fNL) * (phi * phi - dtype(mean))
    out = t * _c(np.fft.rfftn(psi.astype(F64)), dtype)
    return _c(out, dtype).astype(np.complex128), mean
