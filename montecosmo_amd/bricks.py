"""The pieces of montecosmo/bricks.py the PM path touches: cosmology presets (bricks.py:16-47) as a
duck-typed object (the path reads Omega_m, Omega_de, Omega_k, w0, wa and uses `_workspace`, nbody.py:699)
and the initial particle lattice (bricks.py:593-603).

Primordial non-Gaussianity (png_type 'fNL' / 'bias'): the transfer table, `add_png`, the five PNG terms of `lagrangian_bias` and
the `fNL_bias` reparametrisation, each with its VJP.  Alcock-Paczynski: `scale_pos`, `parperp2isoap`, `isoap2parperp` on the host and
the `ap_auto` / `ap_param` remapping inside `observe_pos` (bricks.py:708-732, :795-857).  Kaiser model off the flat sky at fixed a (`kaiser_sky`,
bricks.py:200-231: curved sky and / or light cone, with the PNG term fNL_bp phi) and its VJP.  Eulerian bias expansion on the painted matter
field (`eulerian_bias`, bricks.py:513-586, with the conversions b1_L2E ... of bricks.py:454-464) and its VJP."""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib, nbody, power, tables, utils


class Cosmology:
    """Stand-in for jax_cosmo.Cosmology with the attributes the PM path reads."""

    def __init__(self, Omega_c, Omega_b, h, n_s, sigma8, Omega_k=0.0, w0=-1.0, wa=0.0):
        self.Omega_c, self.Omega_b, self.h, self.n_s, self.sigma8 = Omega_c, Omega_b, h, n_s, sigma8
        self.Omega_k, self.w0, self.wa = Omega_k, w0, wa
        self._workspace = {}

    @property
    def Omega_m(self):
        return self.Omega_b + self.Omega_c

    @property
    def Omega_de(self):
        return 1.0 - self.Omega_k - self.Omega_m


def _preset(**defaults):
    def make(**kw):
        args = dict(defaults)
        args.update(kw)
        return Cosmology(**args)
    return make


Planck15 = _preset(Omega_c=0.2589, Omega_b=0.04860, Omega_k=0.0, h=0.6774, n_s=0.9667, sigma8=0.8159, w0=-1.0, wa=0.0)
Planck18 = _preset(Omega_c=0.2607, Omega_b=0.0490, sigma8=0.8102, Omega_k=0.0, h=0.6766, n_s=0.9665, w0=-1.0, wa=0.0)
AbacusSummit0 = _preset(Omega_c=0.26447041, Omega_b=0.04930169, sigma8=0.8076353990239834, Omega_k=0.0, h=0.6736,
                        n_s=0.9649, w0=-1.0, wa=0.0)


def regular_pos(mesh_shape, ptcl_shape=None):
    """Regularly spaced positions in cell coordinates, x slowest / z fastest (bricks.py:593-603), float64 numpy.
    (`montecosmo_amd.nbody.LatticePos.regular` is the same lattice in the kernels' displacement encoding.)"""
    ptcl_shape = mesh_shape if ptcl_shape is None else ptcl_shape
    axes = [np.arange(p) * (m / p) for m, p in zip(mesh_shape, ptcl_shape)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------
# Lagrangian bias expansion (bricks.py:327-443)
BIAS_KEYS = ("b1", "b2", "bs2", "b3", "bds2", "bs3", "bn2", "bnpar")


BiasCtx = PngCtx = ObsCtx = _lib.Ctx


def lagrangian_bias(cosmo, pos, a, box_size, lin_mesh, bias, png=None, png_type=None, kpow=None, read_order: int = 2,
                    return_ctx=False):
    """Lagrangian bias expansion weights (bricks.py:327-443): returns (weights (N,), dvel (N,3), phi) like the
    reference.  `a`: scalar or (N,1) scale factor(s); `pos`: the Lagrangian positions in cell units ((N,3) array or
    LatticePos); `bias`: dict with the keys BIAS_KEYS (missing keys = 0).  HIP: mcpm_bias_fields_f32 -> mcpm_read_f32 x5 ->
    mcpm_bias_weights_f32.
    png_type None: phi = 0.  Otherwise `png` holds the products 'fNL_bp', 'fNL_bpd' (what `fNL_bias` returns), 'fNL_bpd2',
    'fNL_bps2', 'fNL_bn2p' (missing = 0); phi = irfftn(lin / t) and lap phi are formed (mcpm_png_phi_f32, two transforms), read
    at the particles and the five terms of bricks.py:413-441 added (mcpm_png_weights_f32); phi comes back as a device mesh."""
    if png_type not in (None, "fNL", "bias"):
        raise ValueError(f"png_type must be None, 'fNL' or 'bias', got {png_type!r}")
    spec = nbody._c64(lin_mesh)
    shape = nbody.ch2rshape(spec.shape)
    plan, p, n, mode = nbody._pos_args(pos, shape)
    M = plan.M
    dev = spec.device
    kphys = [float(s) / float(b) for s, b in zip(shape, box_size)]
    fields = torch.empty((7,) + tuple(shape), dtype=torch.float32, device=dev)
    # with a context for the adjoint, delta and the Hessian meshes stay resident for it (six transforms less per gradient)
    hess6 = torch.empty((6,) + tuple(shape), dtype=torch.float32, device=dev) if (return_ctx and os.environ.get("MCPM_BIAS_KEEP", "1") != "0") else None
    plan.call("mcpm_bias_fields_save_f32", spec, kphys[0], kphys[1], kphys[2], fields, hess6)
    # NGP read at the mesh's own lattice points is the identity: the fields themselves are the reads (no pass at all)
    ident = (int(read_order) == 1 and isinstance(pos, nbody.LatticePos) and pos.is_regular and tuple(pos.ptcl_shape) == tuple(shape))
    if ident:
        reads, gr, gcs = fields[:4].reshape(4, n), fields[4:7], M
    else:
        gcs = 0
        reads = torch.empty((4, n), dtype=torch.float32, device=dev)
        for c in range(4):
            plan.call("mcpm_read_f32", p, n, mode, fields[c], 1, int(read_order), reads[c])
        gr = torch.empty((n, 3), dtype=torch.float32, device=dev)
        plan.call("mcpm_read_f32", p, n, mode, fields[4], 3, int(read_order), gr)
    if isinstance(a, torch.Tensor) and a.is_cuda:      # per-particle scale factors on the device (light cone)
        gp, g_shape = nbody.growth_dev(cosmo, a, "g"), tuple(a.shape)
        if gp.numel() != n:
            raise ValueError("a must have one entry per particle")
        gs = 0.0
    else:
        g = np.asarray(nbody.a2g(cosmo, a), dtype=np.float64)
        g_shape = g.shape
        gp = nbody._f32(g.reshape(-1), (n,)) if g.size == n and n > 1 else None
        gs = float(g.reshape(-1)[0]) if gp is None else 0.0
    b8 = (C.c_float * 8)(*[float(bias.get(k, 0.0)) for k in BIAS_KEYS])
    w = torch.empty(n, dtype=torch.float32, device=dev)
    dvel = torch.empty((n, 3), dtype=torch.float32, device=dev)
    plan.call("mcpm_bias_weights_f32", n, reads[0], reads[1], reads[2], reads[3], gr, gcs, gp, gs, b8, w, dvel, None)
    phi, pctx = 0., None
    if png_type is not None:
        png = png or {}
        tab, nt = _png_table(cosmo, kpow, dev)
        pl = torch.empty((2,) + tuple(shape), dtype=torch.float32, device=dev)      # phi, lap phi
        plan.call("mcpm_png_phi_f32", spec, kphys[0], kphys[1], kphys[2], tab, tab[nt:], nt, pl[0], pl[1])
        if ident:
            pr = pl.reshape(2, n)
        else:
            pr = torch.empty((2, n), dtype=torch.float32, device=dev)
            for c in range(2):
                plan.call("mcpm_read_f32", p, n, mode, pl[c], 1, int(read_order), pr[c])
        b5 = (C.c_float * 5)(*[float(png.get(k, 0.0)) for k in PNG_KEYS[1:]])
        plan.call("mcpm_png_weights_f32", n, reads[0], reads[1], pr[0], pr[1], gp, gs, b5, w, None)
        phi, pctx = pl[0], BiasCtx(tab=tab, nt=nt, pr=pr, b5=b5)
    if return_ctx:
        ctx = BiasCtx(plan=plan, spec=spec, shape=shape, p=p, n=n, mode=mode, kphys=kphys, reads=reads, gr=gr, gp=gp, gs=gs,
                      g_shape=g_shape, b8=b8, read_order=int(read_order), gcs=gcs, hess6=hess6, png=pctx)
        return (w, dvel, phi), ctx
    return w, dvel, phi


def lagrangian_bias_vjp(ctx, weights_bar, dvel_bar, defer_phi=False):
    """VJP of lagrangian_bias w.r.t. (lin_mesh, bias, growth factor(s) a2g(a)): returns (lin_mesh_bar [complex64,
    real-pair convention], bias_bar dict, growths_bar [shape of a2g(a)]).  Positions are the fixed Lagrangian
    lattice of the model (model.py:738), so no position cotangent is formed.
    With png_type set three more outputs follow: png_bar (dict: cotangents of the five PNG coefficients), lin_mesh_bar and
    growths_bar then INCLUDE the PNG terms' share, and trans_bar (float64 numpy, per table node).  <phi delta> is a mean over
    particles: its cotangent is a fixed-order float64 sum handed back to every particle (mcpm_png_weights_vjp_f32).
    `defer_phi`: the sixth output is instead the pair of real meshes (phi_bar, lap_phi_bar) and lin_mesh_bar leaves their share
    out -- the caller hands them to `add_png_vjp`, where they meet add_png's own phi cotangent before the single divide by t."""
    plan, n, dev = ctx.plan, ctx.n, ctx.spec.device
    wb = nbody._f32(weights_bar, (n,))
    vb = nbody._f32(dvel_bar, (n, 3))
    fb = torch.empty((7,) + tuple(ctx.shape), dtype=torch.float32, device=dev)
    if ctx.gcs:      # identity reads: the read cotangents ARE the mesh cotangents
        rb, grb = fb[:4].reshape(4, n), fb[4:7]
    else:
        rb = torch.empty((4, n), dtype=torch.float32, device=dev)
        grb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    gbar = torch.empty(n, dtype=torch.float32, device=dev) if ctx.gp is not None else None
    scal = torch.zeros(10, dtype=torch.float64, device=dev)
    r = ctx.reads
    plan.call("mcpm_bias_weights_vjp_f32", n, r[0], r[1], r[2], r[3], ctx.gr, ctx.gcs, ctx.gp, ctx.gs, ctx.b8, wb, vb, rb[0], rb[1], rb[2], rb[3],
              grb, gbar, scal)
    pc = getattr(ctx, "png", None)
    if pc is not None:
        plb = torch.empty((2,) + tuple(ctx.shape), dtype=torch.float32, device=dev)      # cotangents of the phi, lap phi meshes
        prb = plb.reshape(2, n) if ctx.gcs else torch.empty((2, n), dtype=torch.float32, device=dev)
        pscal = torch.zeros(10, dtype=torch.float64, device=dev)
        plan.call("mcpm_png_weights_vjp_f32", n, r[0], r[1], pc.pr[0], pc.pr[1], ctx.gp, ctx.gs, pc.b5, wb, rb[0], rb[1], prb[0], prb[1], gbar,
                  pscal)
        if not ctx.gcs:
            for c in range(2):
                plan.call("mcpm_paint_f32", ctx.p, n, ctx.mode, prb[c], 1, 0.0, ctx.read_order, plb[c], 0)
    if not ctx.gcs:
        for c in range(4):       # adjoint of a read w.r.t. its mesh = a weighted paint
            plan.call("mcpm_paint_f32", ctx.p, n, ctx.mode, rb[c], 1, 0.0, ctx.read_order, fb[c], 0)
        plan.call("mcpm_paint3_f32", ctx.p, n, ctx.mode, grb, ctx.read_order, fb[4], 0)
    out = torch.empty(tuple(ctx.spec.shape), dtype=torch.complex64, device=dev)
    if getattr(ctx, "hess6", None) is not None:
        plan.call("mcpm_bias_fields_vjp_saved_f32", ctx.kphys[0], ctx.kphys[1], ctx.kphys[2], ctx.hess6, fb, out)
    else:
        plan.call("mcpm_bias_fields_vjp_f32", ctx.spec, ctx.kphys[0], ctx.kphys[1], ctx.kphys[2], fb, out)
    s = scal.cpu().numpy()
    bias_bar = {k: float(s[i]) for i, k in enumerate(BIAS_KEYS)}
    # per-particle growth cotangents stay on the device; a scalar one comes back as a float64 array of the shape of a2g(a)
    if pc is None:
        growths_bar = gbar.reshape(ctx.g_shape) if gbar is not None else np.asarray(s[8]).reshape(ctx.g_shape)
        return out, bias_bar, growths_bar
    ps = pscal.cpu().numpy()
    growths_bar = gbar.reshape(ctx.g_shape) if gbar is not None else np.asarray(s[8] + ps[7]).reshape(ctx.g_shape)
    png_bar = {k: float(ps[i]) for i, k in enumerate(PNG_KEYS[1:])}
    if defer_phi:
        return out, bias_bar, growths_bar, png_bar, None, (plb[0], plb[1])
    lb, trans_bar = png_phi_vjp(plan, ctx.spec, ctx.kphys, pc.tab, pc.nt, plb[0], plb[1])
    return out + lb, bias_bar, growths_bar, png_bar, trans_bar, None


# ------------------------------------------------------------------------------------------------
# Local primordial non-Gaussianity: transfer table, add_png (bricks.py:108-141), bias reparametrisation (bricks.py:466-508)
RH = 2997.92458      # c / (100 km/s/Mpc) in Mpc/h (jax_cosmo.constants.rh)
PNG_KEYS = ("fNL", "fNL_bp", "fNL_bpd", "fNL_bpd2", "fNL_bps2", "fNL_bn2p")


def trans_phi2delta_table(cosmo, a=1., kpow=None):
    """The 256-point table (ks [h/Mpc], trans) behind `trans_phi2delta_interp` (bricks.py:108-127): the transfer function from
    the primordial potential to the linear density at scale factor `a`,
        trans = 2 rh^2 k^2 T(k) D(a) / D_md / (3 Omega_m),  T = sqrt(P_lin / k^n_s) normalised to 1 at ks[0],
    with D_md = a2g(a_md) / a_md at z = 10.  P_lin is `kpow` (a (ks, pows) tabulation) or the Eisenstein & Hu table of
    `power.lin_power_table`; its amplitude cancels in T, so the table does not depend on sigma8.  The look-up is linear and 0
    outside the table (mcpm_png_add_f32 does it on the device).  Host float64."""
    ks, pows = power.lin_power_table(cosmo) if kpow is None else kpow
    ks, pows = np.asarray(ks, dtype=np.float64), np.asarray(pows, dtype=np.float64)
    pow_large = ks ** cosmo.n_s
    lin_trans = (pows / pow_large / (pows[0] / pow_large[0])) ** .5
    a_md = 1. / (1. + 10.)
    growth_md = float(nbody.a2g(cosmo, a_md)) / a_md
    trans = 2. * RH ** 2 * ks ** 2 * lin_trans * (nbody.a2g(cosmo, a) / growth_md) / (3. * cosmo.Omega_m)
    return ks, trans


def _png_table(cosmo, kpow, device):
    """(device float64 tensor [ks | trans], n): the table of `trans_phi2delta_table` at a = 1, as the PNG kernels take it."""
    tab = tables.on_device(cosmo, tables.TRANS, device, kpow=kpow)
    return tab.t, tab.n["ks"]


def add_png(cosmo, fNL, lin_mesh, box_size, kpow=None, return_ctx=False, phi=None):
    """Add local primordial non-Gaussianity to the linear field (bricks.py:129-141):
        phi = irfftn(safe_div(lin_mesh, t(|k|))),  phi <- phi + fNL (phi^2 - <phi^2>),  returns t(|k|) rfftn(phi)
    with t = trans_phi2delta_table(cosmo, kpow=kpow) looked up inside the kernels.  `phi`: the Gaussian potential if the caller
    already holds it (the third return value of `lagrangian_bias` on the same mesh), which saves the divide and one transform.
    HIP: mcpm_png_add_f32 (png_div_kernel -> C2R -> png_moment_kernel + fold -> png_quad_kernel -> R2C -> png_mult_kernel);
    <phi^2> is a fixed-order float64 sum, so repeat calls are bitwise equal."""
    spec = nbody._c64(lin_mesh)
    shape = nbody.ch2rshape(spec.shape)
    plan, dev = nbody.get_plan(shape), spec.device
    kphys = [float(s) / float(b) for s, b in zip(shape, box_size)]
    tab, nt = _png_table(cosmo, kpow, dev)
    phi_t = nbody._f32(phi, shape) if phi is not None else torch.empty(tuple(shape), dtype=torch.float32, device=dev)
    out = torch.empty(tuple(spec.shape), dtype=torch.complex64, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    plan.call("mcpm_png_add_f32", spec, kphys[0], kphys[1], kphys[2], tab, tab[nt:], nt, float(fNL), int(phi is not None), phi_t, out, mean)
    if return_ctx:
        return out, PngCtx(plan=plan, spec=spec, out=out, phi=phi_t, mean=mean, kphys=kphys, tab=tab, nt=nt, fNL=float(fNL))
    return out


def png_phi_vjp(plan, spec, kphys, tab, nt, phi_bar, lap_phi_bar=None):
    """Adjoint of (phi, lap phi) = irfftn((1, -k^2) safe_div(lin_mesh, t)) alone: real-mesh cotangents -> (lin_mesh_bar [complex64,
    real-pair convention], trans_bar [float64 numpy]).  HIP: mcpm_png_add_vjp_f32 without a cotangent of add_png's output."""
    lin_bar = torch.empty(tuple(spec.shape), dtype=torch.complex64, device=spec.device)
    scal = torch.empty(1 + nt, dtype=torch.float64, device=spec.device)
    plan.call("mcpm_png_add_vjp_f32", spec, None, None, None, kphys[0], kphys[1], kphys[2], tab, tab[nt:], nt, 0.0, None, nbody._f32(phi_bar),
              None if lap_phi_bar is None else nbody._f32(lap_phi_bar), lin_bar, scal, scal[1:])
    return lin_bar, scal[1:].cpu().numpy()


def add_png_vjp(ctx, out_bar, phi_bar=None, lap_phi_bar=None, sync=True):
    """VJP of add_png w.r.t. (lin_mesh, fNL, the table entries of t): cotangent of the output (complex, real-pair convention) ->
    (lin_mesh_bar [complex64, real-pair convention], fNL_bar [float], trans_bar [float64 numpy, one entry per table node]).
    trans_bar collects both uses of t (the divide and the multiply); contract it with d trans / d theta for a cosmological
    parameter.  `phi_bar`, `lap_phi_bar`: real-mesh cotangents of the Gaussian phi and of lap phi from their other readers (the
    bias weights, `lagrangian_bias_vjp(..., defer_phi=True)`); they are folded in before the divide by t.  `sync=False` returns the
    last two outputs as one device float64 tensor [fNL_bar, trans_bar...] instead of blocking on a copy to the host.
    HIP: mcpm_png_add_vjp_f32; every sum is order-independent, so repeat calls are bitwise equal."""
    dev = ctx.spec.device
    ob = nbody._c64(out_bar, tuple(ctx.spec.shape))
    lin_bar = torch.empty(tuple(ctx.spec.shape), dtype=torch.complex64, device=dev)
    scal = torch.empty(1 + ctx.nt, dtype=torch.float64, device=dev)
    ctx.plan.call("mcpm_png_add_vjp_f32", ctx.spec, ctx.out, ctx.phi, ctx.mean, ctx.kphys[0], ctx.kphys[1], ctx.kphys[2], ctx.tab, ctx.tab[ctx.nt:],
                  ctx.nt, ctx.fNL, ob, None if phi_bar is None else nbody._f32(phi_bar), None if lap_phi_bar is None else nbody._f32(lap_phi_bar),
                  lin_bar, scal, scal[1:])
    if not sync:
        return lin_bar, scal
    s = scal.cpu().numpy()
    return lin_bar, float(s[0]), s[1:].copy()


def bpd_L2E(bpd, bp):
    """bricks.py:466-467"""
    return bpd + bp / 2


def bpd_E2L(bpd, bp):
    """bricks.py:469-470"""
    return bpd - bp / 2


def b_phi(b1, p=1., delta_c=1.686):
    """Primordial scale-dependent bias parameter, 2 delta_c (b1 + 1 - p) for the Lagrangian b1 (bricks.py:472-481)."""
    return 2 * delta_c * (b1 + 1 - p)


def b_phi_delta(b1, b2, delta_c=1.686):
    """Primordial-density scale-dependent bias parameter, 2 (delta_c b2 - b1) (bricks.py:483-491)."""
    return 2 * (delta_c * b2 - b1)


def fNL_bias(png, bias, p=1., png_type=None):
    """The reparametrisation of bricks.py:493-508: a copy of `png` whose 'fNL_bp', 'fNL_bpd' are the products the bias expansion
    uses -- fNL b_phi(b1, p), fNL b_phi_delta(b1, b2) for png_type 'fNL'; fNL * fNL_bp, fNL * fNL_bpd for 'bias'; unchanged for
    None.  Missing keys count as 0."""
    png = {k: png.get(k, 0.) for k in PNG_KEYS} | {k: v for k, v in png.items() if k not in PNG_KEYS}
    fNL, b1, b2 = png["fNL"], bias.get("b1", 0.), bias.get("b2", 0.)
    if png_type == "fNL":
        png["fNL_bp"], png["fNL_bpd"] = fNL * b_phi(b1, p), fNL * b_phi_delta(b1, b2)
    elif png_type == "bias":
        png["fNL_bp"], png["fNL_bpd"] = fNL * png["fNL_bp"], fNL * png["fNL_bpd"]
    elif png_type is not None:
        raise ValueError(f"png_type must be None, 'fNL' or 'bias', got {png_type!r}")
    return png


def fNL_bias_vjp(png, bias, png_bar, p=1., png_type=None, delta_c=1.686):
    """VJP of fNL_bias: `png_bar` holds the cotangents of the RETURNED dict (missing keys = 0) -> (cotangents of the input png
    dict, cotangents of bias {'b1', 'b2'}).  'fNL': the cotangents of fNL_bp, fNL_bpd chain to fNL, b1, b2; 'bias': to fNL and
    the input fNL_bp, fNL_bpd.  The other entries pass through."""
    out = {k: float(png_bar.get(k, 0.)) for k in PNG_KEYS}
    bp_bar, bpd_bar = out["fNL_bp"], out["fNL_bpd"]
    fNL, b1, b2 = png.get("fNL", 0.), bias.get("b1", 0.), bias.get("b2", 0.)
    bias_bar = {"b1": 0., "b2": 0.}
    if png_type == "fNL":
        out["fNL"] += bp_bar * b_phi(b1, p, delta_c) + bpd_bar * b_phi_delta(b1, b2, delta_c)
        bias_bar["b1"] = fNL * (2 * delta_c * bp_bar - 2 * bpd_bar)
        bias_bar["b2"] = fNL * 2 * delta_c * bpd_bar
        out["fNL_bp"] = out["fNL_bpd"] = 0.
    elif png_type == "bias":
        out["fNL"] += bp_bar * png.get("fNL_bp", 0.) + bpd_bar * png.get("fNL_bpd", 0.)
        out["fNL_bp"], out["fNL_bpd"] = fNL * bp_bar, fNL * bpd_bar
    elif png_type is not None:
        raise ValueError(f"png_type must be None, 'fNL' or 'bias', got {png_type!r}")
    return out, bias_bar


# ------------------------------------------------------------------------------------------------
# Eulerian bias expansion on the painted matter field (bricks.py:454-464, :513-586)
def b1_L2E(b1):
    """bricks.py:454-455"""
    return 1 + b1


def b1_E2L(b1):
    """bricks.py:457-458"""
    return b1 - 1


def b2_L2E(b2, b1L):
    """bricks.py:460-461"""
    return b2 + 8 / 21 * b1L


def b2_E2L(b2, b1L):
    """bricks.py:463-464"""
    return b2 - 8 / 21 * b1L


def eulerian_bias(matter_mesh, phi_mesh, box_size, bias, png, png_type=None, return_ctx=False):
    """Eulerian bias expansion weights (bricks.py:513-586) on the mesh of `matter_mesh`:
        w = 1 + b1E d + b2E (d^2 - <d^2>) / 2 + bs2 (s^2 - 2/3 <d^2>) + bn2 lap d   [+ fNL_bp phi + fNL_bpdE (phi d - <phi d>) with png_type]
    d = irfftn(matter_mesh with its zero mode dropped), s^2 the squared tidal shear of d, phi = irfftn(phi_mesh); wavevectors in h/Mpc.
    `matter_mesh`, `phi_mesh` (read only with png_type; may be None otherwise): half-spectra; `bias`: the LAGRANGIAN parameters (missing
    keys = 0); `png`: the products 'fNL_bp', 'fNL_bpd' that `fNL_bias` returns.  Returns the real mesh w (float32 device tensor).
    HIP: mcpm_eulerian_bias_f32 (two batched C2R, a moment pass, one streaming weights pass; the shear never goes to memory).
    Where the reference's unfinished branch is not followed literally:
      1. the weights mesh alone is returned; the `dvel = 0.` of bricks.py:584, which model.py:831 packs into a tuple with it, is dropped;
      2. (the caller's paint Jacobian: `FieldLevelForward.evolve` uses prod(init_shape / ptcl_shape), not model.py:820, :827);
      3. fNL_bpdE = fNL_bpd + fNL_bp / 2, the algebraic value of bricks.py:523, whose form fNL * bpd_L2E(fNL_bpd / fNL, fNL_bp / fNL) is
         NaN at fNL = 0;
      4. b1E = 1 + b1, b2E = b2 + 8/21 b1 with the Lagrangian b1 (bricks.py:522); bs2, bn2 as given; b3, bds2, bs3 (and bnpar) are not read."""
    if png_type not in (None, "fNL", "bias"):
        raise ValueError(f"png_type must be None, 'fNL' or 'bias', got {png_type!r}")
    mk = nbody._c64(matter_mesh)
    shape = nbody.ch2rshape(mk.shape)
    plan, dev = nbody.get_plan(shape), mk.device
    has_phi = png_type is not None
    if has_phi and phi_mesh is None:
        raise ValueError("png_type is set: eulerian_bias needs phi_mesh")
    pk = nbody._c64(phi_mesh, tuple(mk.shape)) if has_phi else None
    kphys = [float(s) / float(b) for s, b in zip(shape, box_size)]
    b1, b2 = float(bias.get("b1", 0.0)), float(bias.get("b2", 0.0))
    png = png or {}
    bp, bpd = (float(png.get("fNL_bp", 0.0)), float(png.get("fNL_bpd", 0.0))) if has_phi else (0.0, 0.0)
    coef = (C.c_float * 6)(b1_L2E(b1), b2_L2E(b2, b1), float(bias.get("bs2", 0.0)), float(bias.get("bn2", 0.0)), bp, bpd_L2E(bpd, bp))
    w = torch.empty(tuple(shape), dtype=torch.float32, device=dev)
    saved = torch.empty((8 if has_phi else 7,) + tuple(shape), dtype=torch.float32, device=dev)
    moments = torch.empty(2, dtype=torch.float64, device=dev)
    plan.call("mcpm_eulerian_bias_f32", mk, pk, kphys[0], kphys[1], kphys[2], coef, w, saved, moments)
    if return_ctx:
        return w, BiasCtx(plan=plan, shape=tuple(shape), kshape=tuple(mk.shape), kphys=kphys, coef=coef, saved=saved, moments=moments,
                          has_phi=has_phi)
    return w


def eulerian_bias_vjp(ctx, w_bar):
    """VJP of eulerian_bias: cotangent of w -> (matter_mesh_bar, phi_mesh_bar or None [complex64, real-pair convention; the zero mode of
    matter_mesh_bar is 0], bias_bar dict over BIAS_KEYS, png_bar dict {'fNL_bp', 'fNL_bpd'} or None).  The Lagrangian -> Eulerian chain rule
    is applied: b1_bar = b1E_bar + 8/21 b2E_bar, fNL_bp_bar += fNL_bpdE_bar / 2; b3, bds2, bs3, bnpar are not read: exactly 0.0.
    HIP: mcpm_eulerian_bias_vjp_f32; every sum has a fixed order, so repeat calls are bitwise equal."""
    plan, dev = ctx.plan, ctx.saved.device
    wb = nbody._f32(w_bar, ctx.shape)
    mb = torch.empty(ctx.kshape, dtype=torch.complex64, device=dev)
    pb = torch.empty(ctx.kshape, dtype=torch.complex64, device=dev) if ctx.has_phi else None
    cb = torch.empty(6, dtype=torch.float64, device=dev)
    plan.call("mcpm_eulerian_bias_vjp_f32", ctx.saved, ctx.moments, int(ctx.has_phi), ctx.kphys[0], ctx.kphys[1], ctx.kphys[2], ctx.coef, wb, mb, pb,
              cb)
    c = cb.cpu().numpy()
    bias_bar = {k: 0.0 for k in BIAS_KEYS}
    bias_bar.update(b1=float(c[0] + 8 / 21 * c[1]), b2=float(c[1]), bs2=float(c[2]), bn2=float(c[3]))
    png_bar = {"fNL_bp": float(c[4] + c[5] / 2), "fNL_bpd": float(c[5])} if ctx.has_phi else None
    return mb, pb, bias_bar, png_bar


# ------------------------------------------------------------------------------------------------
# Cell <-> physical coordinates, line of sight, redshift-space distortions (bricks.py:628-662, :750-803)
def rot_matrix(box_rot):
    """3x3 matrix of `box_rot`: a scipy Rotation (as the reference passes), a rotation vector (3,) or a matrix."""
    if hasattr(box_rot, "as_matrix"):
        return np.asarray(box_rot.as_matrix(), dtype=np.float64)
    r = np.asarray(box_rot, dtype=np.float64)
    if r.shape == (3, 3):
        return r
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def cell2phys_pos(pos, box_center, box_rot, box_size, mesh_shape):
    """Cell positions to physical positions (bricks.py:628-636); host numpy (set-up sized arrays)."""
    pos = np.asarray(pos, dtype=np.float64) * np.divide(box_size, mesh_shape) - np.asarray(box_size) / 2
    return pos @ rot_matrix(box_rot).T + np.asarray(box_center)


def phys2cell_pos(pos, box_center, box_rot, box_size, mesh_shape):
    """bricks.py:638-646"""
    pos = (np.asarray(pos, dtype=np.float64) - np.asarray(box_center)) @ rot_matrix(box_rot) + np.asarray(box_size) / 2
    return pos / np.divide(box_size, mesh_shape)


def cell2phys_vel(vel, box_rot, box_size, mesh_shape):
    """bricks.py:648-654"""
    return (np.asarray(vel, dtype=np.float64) * np.divide(box_size, mesh_shape)) @ rot_matrix(box_rot).T


def phys2cell_vel(vel, box_rot, box_size, mesh_shape):
    """bricks.py:656-662"""
    return (np.asarray(vel, dtype=np.float64) @ rot_matrix(box_rot)) / np.divide(box_size, mesh_shape)


AP_KEYS = ("alpha_iso", "alpha_ap")


def scale_pos(pos, los, scale_par, scale_perp):
    """Scale positions in the directions parallel and perpendicular to `los` (bricks.py:708-716); host float64."""
    pos, los = np.asarray(pos, dtype=np.float64), np.asarray(los, dtype=np.float64)
    pos_par = (pos * los).sum(-1, keepdims=True) * los
    pos_perp = pos - pos_par
    return pos_par * scale_par + pos_perp * scale_perp


def parperp2isoap(alpha_par, alpha_perp):
    """Parallel and perpendicular scalings -> isotropic and anisotropic scalings (bricks.py:718-724)."""
    alpha_iso = (alpha_par * alpha_perp ** 2) ** (1 / 3)
    alpha_ap = alpha_par / alpha_perp
    return alpha_iso, alpha_ap


def isoap2parperp(alpha_iso, alpha_ap):
    """Isotropic and anisotropic scalings -> parallel and perpendicular scalings (bricks.py:726-732)."""
    alpha_par = alpha_iso * alpha_ap ** (2 / 3)
    alpha_perp = alpha_iso * alpha_ap ** (-1 / 3)
    return alpha_par, alpha_perp


def _ap_args(ctx):
    return (ctx.ap_mode, ctx.alpha_iso, ctx.alpha_ap, ctx.ap_tables, ctx.nap, ctx.nfid)


def observe_pos(cosmo, pos, vel, box_center, box_rot, box_size, evol_shape, paint_shape, a_obs=None, curved_sky=True,
                dvel=None, return_ctx=False, ap_auto=None, ap=None, cosmo_fid=None):
    """Evolved particles (cell units of evol_shape) -> redshift-space positions in cell units of paint_shape: the chain
    los_scalefactor_pos -> cell2phys_pos -> + rsd(vel, los, a, dvel) -> [ap_auto | ap_param] -> phys2cell_pos of
    model.py:780-797, fused in one HIP pass (mcpm_observe_pos_f32 / mcpm_observe_pos_ap_f32).  a_obs=None is the light cone
    (a = chi2a(|x|)).  A LatticePos comes back as a LatticePos on the paint mesh (same particle lattice), an array as an (N,3) tensor.
    Alcock-Paczynski (model.py:787-794): ap_auto=None none (nothing new runs); True: positions scaled by
    a2chi(cosmo_fid, chi2a(cosmo, r)) / r (bricks.py:795-814; `cosmo_fid` required); False: by the parameters of
    `ap` = {'alpha_iso', 'alpha_ap'} (missing = 1; bricks.py:848-857)."""
    evol_shape = tuple(int(s) for s in evol_shape)
    paint_shape = tuple(int(s) for s in paint_shape)
    plan, p, n, mode = nbody._pos_args(pos, evol_shape)
    v = nbody._f32(vel, (n, 3))
    dv = nbody._f32(dvel, (n, 3)) if dvel is not None else None
    R = rot_matrix(box_rot)
    lightcone = a_obs is None
    gf = 0.0 if lightcone else float(nbody.a2g(cosmo, a_obs) * nbody.a2f(cosmo, a_obs))
    geom = (C.c_float * 19)(*[float(x) for x in list(R.reshape(-1)) + list(box_size) + list(box_center) + list(paint_shape) + [gf]])
    flags = (1 if curved_sky else 0) | (2 if lightcone else 0)
    lc = tables.on_device(cosmo, tables.LIGHTCONE, p.device) if lightcone else None
    lctab, nchi, ngrow = (lc.t, lc.n["chi"], lc.n["a"]) if lightcone else (None, 0, 0)
    out = torch.empty((n, 3), dtype=torch.float32, device=p.device)
    apkw = dict(ap_mode=_lib.AP_NONE, alpha_iso=1.0, alpha_ap=1.0, ap_tables=None, nap=0, nfid=0)
    if ap_auto is None:
        plan.call("mcpm_observe_pos_f32", p, v, dv, n, mode, geom, flags, lctab, nchi, ngrow, out)
    else:
        if ap_auto:
            if cosmo_fid is None:
                raise ValueError("ap_auto=True needs the fiducial cosmology `cosmo_fid`")
            apt = tables.on_device(cosmo, tables.AP, p.device, fid=cosmo_fid)
            apkw.update(ap_mode=_lib.AP_AUTO, nap=apt.n["chi"], nfid=apt.n["a_fid"], ap_tables=apt.t)
        else:
            ap = ap or {}
            apkw.update(ap_mode=_lib.AP_PARAM, alpha_iso=float(ap.get("alpha_iso", 1.0)), alpha_ap=float(ap.get("alpha_ap", 1.0)))
        plan.call("mcpm_observe_pos_ap_f32", p, v, dv, n, mode, geom, flags, lctab, nchi, ngrow, apkw["ap_mode"], apkw["alpha_iso"],
                  apkw["alpha_ap"], apkw["ap_tables"], apkw["nap"], apkw["nfid"], out)
    res = nbody.LatticePos(out, paint_shape, pos.ptcl_shape) if isinstance(pos, nbody.LatticePos) else out
    if return_ctx:
        return res, ObsCtx(plan=plan, p=p, v=v, dv=dv, n=n, mode=mode, geom=geom, flags=flags, tables=lctab, nchi=nchi, ngrow=ngrow, lc=lc, **apkw)
    return res


def observe_pos_vjp(ctx, out_bar):
    """VJP of observe_pos: cotangent of the returned positions (N,3) -> (pos_bar, vel_bar, dvel_bar or None, gf_bar) where
    gf_bar is the cotangent of the scalar a2g(a_obs) a2f(a_obs) (0.0 on the light cone).  With Alcock-Paczynski (ap_auto not None)
    a fifth output follows: {'alpha_iso': ..., 'alpha_ap': ...}, the cotangents of the two parameters (0 for ap_auto=True, whose
    cosmology dependence is a table cotangent: `observe_pos_tables_vjp`; alpha_ap's is 0 on a curved sky)."""
    n, dev = ctx.n, ctx.p.device
    ob = nbody._f32(out_bar, (n, 3))
    pb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    vb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    db = torch.empty((n, 3), dtype=torch.float32, device=dev) if ctx.dv is not None else None
    if getattr(ctx, "ap_mode", _lib.AP_NONE) == _lib.AP_NONE:
        gfb = torch.zeros(1, dtype=torch.float64, device=dev)
        ctx.plan.call("mcpm_observe_pos_vjp_f32", ctx.p, ctx.v, ctx.dv, n, ctx.mode, ctx.geom, ctx.flags, ctx.tables, ctx.nchi, ctx.ngrow, ob, pb, vb,
                      db, gfb)
        return pb, vb, db, float(gfb.item())
    sc = torch.zeros(3, dtype=torch.float64, device=dev)      # gf_bar, alpha_iso_bar, alpha_ap_bar
    ctx.plan.call("mcpm_observe_pos_ap_vjp_f32", ctx.p, ctx.v, ctx.dv, n, ctx.mode, ctx.geom, ctx.flags, ctx.tables, ctx.nchi, ctx.ngrow,
                  *_ap_args(ctx), ob, pb, vb, db, sc, sc[1:])
    s = sc.cpu().numpy()
    return pb, vb, db, float(s[0]), {"alpha_iso": float(s[1]), "alpha_ap": float(s[2])}


def observe_pos_tables_vjp(ctx, out_bar):
    """Cotangents of the look-up tables inside observe_pos (device float64): chi_bar[nchi], g_bar[ngrow], f_bar[ngrow] on the light
    cone (the growth look-ups at the evolved positions plus, with ap_auto=True, the chi2a(cosmo, r') of the Alcock-Paczynski
    step); at fixed a_obs with ap_auto=True chi_bar alone.  mcpm_observe_pos_tables_vjp_f32 / mcpm_observe_pos_ap_tables_vjp_f32."""
    n, dev = ctx.n, ctx.p.device
    ob = nbody._f32(out_bar, (n, 3))
    if getattr(ctx, "ap_mode", _lib.AP_NONE) == _lib.AP_NONE:
        tb = torch.empty(ctx.nchi + 2 * ctx.ngrow, dtype=torch.float64, device=dev)
        ctx.plan.call("mcpm_observe_pos_tables_vjp_f32", ctx.p, ctx.v, ctx.dv, n, ctx.mode, ctx.geom, ctx.flags, ctx.tables, ctx.nchi, ctx.ngrow, ob,
                      tb)
        return tb
    lc = bool(ctx.flags & 2)
    tb = torch.empty((ctx.nchi + 2 * ctx.ngrow) if lc else ctx.nap, dtype=torch.float64, device=dev)
    ctx.plan.call("mcpm_observe_pos_ap_tables_vjp_f32", ctx.p, ctx.v, ctx.dv, n, ctx.mode, ctx.geom, ctx.flags, ctx.tables, ctx.nchi, ctx.ngrow,
                  *_ap_args(ctx), ob, tb)
    return tb


# ------------------------------------------------------------------------------------------------
# Kaiser model on the curved sky and on the light cone (bricks.py:186-231 kaiser_model, :760-778 los_scalefactor_mesh)
_KAISER_MU2 = {}


def kaiser_mu2(shape, box_size, los):
    """mu^2 = (k . los)^2 / k^2 on the half-spectrum of `shape`, k in h/Mpc (bricks.py:201-204), as irfftn sees it: on the kz = 0 and
    kz = Nyquist planes a mode and its mirror image are both stored, and irfftn keeps the Hermitian part of the product mu^2 lin.  For a
    real field's spectrum that drops the terms k_a k_b with exactly one of a, b on its Nyquist index (k_a keeps its sign -pi under the
    mirror image, k_b does not) -- the rule of the Hessian kernel (kspace.hip).  Off those planes it is the plain mu^2.  Host float64."""
    shape = tuple(int(s) for s in shape)
    kvec = nbody.rfftk(shape, box_size)
    kk = sum(k ** 2 for k in kvec)
    nyq = [np.zeros(k.shape, bool) for k in kvec]
    for a in range(3):
        if shape[a] % 2 == 0:
            nyq[a].reshape(-1)[shape[a] // 2] = True
    special = np.zeros(kvec[2].shape, bool)
    special.reshape(-1)[[0, shape[2] // 2]] = True
    num = 0.
    for a in range(3):
        for b in range(3):
            num = num + np.where(special & (nyq[a] != nyq[b]), 0., los[a] * los[b] * kvec[a] * kvec[b])
    return nbody.safe_div(num, kk)


def _kaiser_mu2_dev(shape, box_size, los, device):
    key = (tuple(shape), tuple(float(b) for b in box_size), tuple(float(l) for l in los), str(device))
    hit = _KAISER_MU2.get(key)
    if hit is None:
        if len(_KAISER_MU2) > 4:
            _KAISER_MU2.clear()
        hit = _KAISER_MU2[key] = torch.from_numpy(np.ascontiguousarray(kaiser_mu2(shape, box_size, los), dtype=np.float32)).to(device)
    return hit


def kaiser_sky(cosmo, lin_mesh, box_size, box_center, box_rot, b1E, fNL_bp=None, a_obs=None, curved_sky=True, kpow=None, return_ctx=False):
    """The two branches of `kaiser_model` that are not diagonal in k (bricks.py:200-231), with the geometry of `los_scalefactor_mesh` on the
    mesh of `lin_mesh`: the cell (i, j, k) sits at x = (i, j, k) box_size / shape - box_size / 2 + R^T box_center in cell axes, and
        curved sky:  r = |x|, l = safe_div(x, r);  out = 1 + g(a) [ b1E delta + f(a) sum_ab l_a l_b irfftn(k_a k_b / k^2 lin) ] + fNL_bp phi
        flat sky:    r = |x . los|;                out = 1 + g(a) [ b1E delta + f(a) irfftn(mu^2 lin) ] + fNL_bp phi
    with a = a_obs or chi2a(cosmo, r) per cell (a_obs = None, the light cone), delta = irfftn(lin), phi = irfftn(safe_div(lin, t(|k|)))
    (only when `fNL_bp` is not None; t from `kpow`, as the reference's Kaiser model takes it).  On the curved sky k is in cell units
    (metrics.py:422, rfftk without a box) and the sum is the tensor form of the reference's delta / 3 + 8 pi / 15 sum_m Y_2m(l) irfftn(Y_2m(k) lin)
    (the addition theorem); delta is taken as the trace of the six meshes, so `lin_mesh` MUST have a zero k = 0 mode (white2lin leaves
    none).  On the flat sky k is in h/Mpc (bricks.py:201-204).  At r = 0 the direction is 0 and a the clamped end of the table: finite.
    HIP: mcpm_kspace_hessian_f32 (or the mu^2 multiply) -> batched C2R -> mcpm_kaiser_sky_f32.  Returns the real mesh (float32)."""
    spec = nbody._c64(lin_mesh)
    shape = nbody.ch2rshape(spec.shape)
    plan, dev = nbody.get_plan(shape), spec.device
    curved, lightcone = bool(curved_sky), a_obs is None
    c = rot_matrix(box_rot).T @ np.asarray(box_center, dtype=np.float64)
    los = nbody.safe_div(c, np.linalg.norm(c))
    geom = np.ascontiguousarray(np.concatenate([np.asarray(box_size, dtype=np.float64), c, los]))
    flags = (1 if curved else 0) | (2 if lightcone else 0)
    lc = tables.on_device(cosmo, tables.LIGHTCONE, dev) if lightcone else None
    lctab, nchi, ngrow = (lc.t, lc.n["chi"], lc.n["a"]) if lightcone else (None, 0, 0)
    g, f = (0., 0.) if lightcone else (float(nbody.a2g(cosmo, a_obs)), float(nbody.a2f(cosmo, a_obs)))
    nm = 6 if curved else 2
    specs = torch.empty((nm,) + tuple(spec.shape), dtype=torch.complex64, device=dev)
    mu2 = None
    if curved:
        plan.call("mcpm_kspace_hessian_f32", spec, specs, 1.0 / plan.M, _lib.FD_INF, _lib.FD_INF)
    else:
        mu2 = _kaiser_mu2_dev(shape, box_size, los, dev)
        torch.mul(spec, 1.0 / plan.M, out=specs[0])
        torch.mul(specs[0], mu2, out=specs[1])
    meshes = torch.empty((nm,) + tuple(shape), dtype=torch.float32, device=dev)
    plan.call("mcpm_fft_c2r", specs, meshes, nm)
    phi = kphys = tab = nt = None
    if fNL_bp is not None:
        kphys = [float(s) / float(b) for s, b in zip(shape, box_size)]
        tab, nt = _png_table(cosmo, kpow, dev)
        plan.call("mcpm_png_div_f32", spec, kphys[0], kphys[1], kphys[2], tab, tab[nt:], nt, 1.0 / plan.M, specs[0])
        phi = torch.empty(tuple(shape), dtype=torch.float32, device=dev)
        plan.call("mcpm_fft_c2r", specs[0], phi, 1)
    del specs
    out = torch.empty(tuple(shape), dtype=torch.float32, device=dev)
    args = (geom, flags, lctab, nchi, ngrow, g, f, float(b1E), 0.0 if fNL_bp is None else float(fNL_bp))
    plan.call("mcpm_kaiser_sky_f32", meshes, phi, *args, out)
    if return_ctx:
        return out, _lib.Ctx(plan=plan, spec=spec, shape=tuple(shape), meshes=meshes, phi=phi, args=args, curved=curved, lightcone=lightcone,
                             mu2=mu2, kphys=kphys, tab=tab, nt=nt, lc=lc)
    return out


def kaiser_sky_vjp(ctx, out_bar):
    """VJP of kaiser_sky: cotangent of the returned mesh -> dict with 'lin_mesh' (complex64, real-pair convention), 'b1E', 'fNL_bp' (floats;
    0.0 without phi), at fixed a_obs 'g', 'f' (cotangents of a2g(a_obs), a2f(a_obs)), on the light cone 'tables': {'chi', 'g', 'f'}
    (float64 numpy cotangents of the chi nodes of chi2a and of the growth tables, for `cosmo_vjp`), and with phi 'trans_bar' (cotangent of
    the transfer table's entries).  HIP: mcpm_kaiser_sky_vjp_f32 -> batched R2C -> mcpm_kspace_hessian_vjp_f32 (or the mu^2 multiply),
    mcpm_png_add_vjp_f32 for phi, mcpm_kaiser_sky_tables_vjp_f32.  Every sum is order-independent: repeat calls are bitwise equal."""
    plan, shape, dev = ctx.plan, ctx.shape, ctx.spec.device
    ob = nbody._f32(out_bar, shape)
    nm = 6 if ctx.curved else 2
    mb = torch.empty((nm,) + shape, dtype=torch.float32, device=dev)
    pb = torch.empty(shape, dtype=torch.float32, device=dev) if ctx.phi is not None else None
    scal = torch.empty(4, dtype=torch.float64, device=dev)
    plan.call("mcpm_kaiser_sky_vjp_f32", ctx.meshes, ctx.phi, *ctx.args, ob, mb, pb, scal)
    specs = torch.empty((nm,) + tuple(ctx.spec.shape), dtype=torch.complex64, device=dev)
    plan.call("mcpm_fft_r2c", mb, specs, nm)
    if ctx.curved:
        lin_bar = torch.empty(tuple(ctx.spec.shape), dtype=torch.complex64, device=dev)
        plan.call("mcpm_kspace_hessian_vjp_f32", specs, lin_bar, 1.0 / plan.M, _lib.FD_INF, _lib.FD_INF, 1, 0)
    else:      # the adjoint of irfftn (rfftn / M, the modes 1 : nz // 2 doubled) behind the two real multipliers
        lin_bar = (specs[0] + specs[1] * ctx.mu2) * (1.0 / plan.M)
        lin_bar[..., 1:shape[-1] // 2] *= 2.0
    res = {"trans_bar": None}
    if ctx.phi is not None:
        lb, res["trans_bar"] = png_phi_vjp(plan, ctx.spec, ctx.kphys, ctx.tab, ctx.nt, pb)
        lin_bar = lin_bar + lb
    if ctx.lightcone:
        geom, flags, lctab, nchi, ngrow, _, _, b1E, _ = ctx.args
        tb = torch.empty(nchi + 2 * ngrow, dtype=torch.float64, device=dev)
        plan.call("mcpm_kaiser_sky_tables_vjp_f32", ctx.meshes, geom, flags, lctab, nchi, ngrow, b1E, ob, tb)
        res["tables"] = ctx.lc.bars(tb)
    s = scal.cpu().numpy()
    res.update({"lin_mesh": lin_bar, "b1E": float(s[0]), "fNL_bp": float(s[1]) if ctx.phi is not None else 0.0})
    if not ctx.lightcone:
        res.update({"g": float(s[2]), "f": float(s[3])})
    return res


# ------------------------------------------------------------------------------------------------
# Posterior of the initial field under the fiducial linear Kaiser model (bricks.py:234-247), lin2white (bricks.py:159-164) and
# count2delta (bricks.py:927-937): what `FieldLevelLogDensity.kaiser_post` starts chains from
def power_mult(plan, spec, kphys, cosmo, kpow, sigma8, out):
    """out = spec sqrt(sigma8^2 P(|k|)) (mcpm_power_mult_f32), P the table `kpow` (sigma8 = 1) or the Eisenstein & Hu one of `cosmo`."""
    tab = tables.on_device(cosmo, tables.POWER, spec.device, kpow=kpow)
    plan.call("mcpm_power_mult_f32", spec, kphys[0], kphys[1], kphys[2], float(sigma8) ** 2, tab.t, tab.v["pows"], tab.n["ks"], out)
    return out


def kaiser_post_white(delta_obs, noise, cosmo, a, box_size, var_noise, b1E, los=(0., 0., 0.), kpow=None, temp=1., scale_field=1.,
                      moments=False):
    """The one call of mcpm_kaiser_post_c64 (csrc/kaiser_post.hip).  delta_obs: half-spectrum of the observed contrast; noise: None (no
    white field is formed), or rg2cgh of unit normal meshes with a leading chain axis, (n_chains, *half-spectrum shape).  Returns
    (white, means, stds): white = scale_field * lin2white(sqrt(temp) stds noise + means) per chain (None without noise), means / stds the
    posterior moments (None unless `moments`)."""
    spec = nbody._c64(delta_obs)
    shape = nbody.ch2rshape(spec.shape)
    plan, dev = nbody.get_plan(shape), spec.device
    kphys = [float(s) / float(b) for s, b in zip(shape, box_size)]
    tab = tables.on_device(cosmo, tables.POWER, dev, kpow=kpow)
    white, n_chains = None, 1
    if noise is not None:
        noise = nbody._c64(noise)
        if noise.ndim != 4 or tuple(noise.shape[1:]) != tuple(spec.shape):
            raise ValueError(f"noise must have shape (n_chains, {tuple(spec.shape)}), got {tuple(noise.shape)}")
        n_chains = int(noise.shape[0])
        white = torch.empty_like(noise)
    means = torch.empty_like(spec) if moments else None
    stds = torch.empty(tuple(spec.shape), dtype=torch.float32, device=dev) if moments else None
    plan.call("mcpm_kaiser_post_c64", spec, noise, n_chains, kphys[0], kphys[1], kphys[2], float(cosmo.sigma8) ** 2, tab.t, tab.v["pows"], tab.n["ks"],
              *[float(l) for l in los], float(nbody.a2g(cosmo, a)), float(nbody.a2f(cosmo, a)), float(b1E), float(var_noise), float(temp),
              float(scale_field), float(np.prod(kphys)), white, means, stds)
    return white, means, stds


def kaiser_posterior(delta_obs, cosmo, a, box_size, var_noise, b1E, los=(0., 0., 0.), kpow=None):
    """Posterior mean and std of the linear matter field (at a = 1) given the observed contrast `delta_obs` (half-spectrum), under the
    flat-sky Kaiser model at scale factor `a` (bricks.py:234-247); the power is `kpow` (sigma8 = 1) or Eisenstein & Hu, times cosmo.sigma8^2:
        p = P(|k|) prod(shape / box_size),  boost = a2g (b1E + a2f mu^2),  stds = sqrt(p / (1 + boost^2 / var_noise p)),
        means = stds^2 boost / var_noise delta_obs.
    HIP: mcpm_kaiser_post_c64 with temp = 0 and its two optional outputs.  Returns (means complex64, stds float32), device tensors."""
    _, means, stds = kaiser_post_white(delta_obs, None, cosmo, a, box_size, var_noise, b1E, los=los, kpow=kpow, temp=0., moments=True)
    return means, stds


def lin2white(cosmo, lin_mesh, init_shape, box_size, kpow=None):
    """Linear matter mesh -> white noise mesh (bricks.py:159-164): safe_div(lin_mesh, sqrt(P(|k|))), 0 where P = 0 (k = 0 and the modes
    outside the table).  The divisor is the multiplier of white2lin (mcpm_power_mult_f32 on a mesh of ones), its reciprocal made safe."""
    spec = nbody._c64(lin_mesh, utils.r2chshape(init_shape))
    kphys = [float(s) / float(b) for s, b in zip(init_shape, box_size)]
    t = power_mult(nbody.get_plan(init_shape), torch.ones_like(spec), kphys, cosmo, kpow, cosmo.sigma8, torch.empty_like(spec)).real
    ok = t != 0
    return torch.where(ok, spec / torch.where(ok, t, torch.ones_like(t)), torch.zeros_like(spec))


def count2delta(mesh, selec_mesh):
    """Count mesh -> contrast mesh under the global integral constraint (bricks.py:927-937):
        alpha = selec_mesh mean(mesh) / mean(selec_mesh),   delta = (mesh - alpha) / sqrt(mean(alpha^2))
    `selec_mesh`: a mesh of the same shape, or a scalar (then delta = (mesh - mean) / |mean|).  Means in float64; float32 device tensor."""
    m = nbody._f32(mesh).double()
    sel = nbody._f32(selec_mesh).double() if (torch.is_tensor(selec_mesh) or np.ndim(selec_mesh) > 0) else \
        torch.full((), float(selec_mesh), dtype=torch.float64, device=m.device)
    alpha = sel * (m.mean() / sel.mean())
    return ((m - alpha) / (alpha ** 2).mean() ** .5).float()


# ------------------------------------------------------------------------------------------------
# Sample mesh -> base mesh (bricks.py:290-320)
def samp2base_mesh(init: dict, precond, transfer, inv=False, temp=1.) -> dict:
    """Transform the sample mesh into the base mesh, i.e. the initial wavevector coefficients (bricks.py:290-320):
    'real': rfftn(mesh) * transfer; 'fourier' / 'kaiser': rg2cgh(mesh) * transfer; and the inverse.  `transfer` is the
    model's (fiducial, fixed) real k-space array; the permutation runs in mcpm_rg2cgh_f32 / mcpm_cgh2rg_f32."""
    assert len(init) <= 1, "init dict should only have one or zero key"
    for in_name, mesh in init.items():
        out_name = in_name + '_' if inv else in_name[:-1]
        tr = torch.as_tensor(np.asarray(transfer, dtype=np.float32) * temp ** .5, device=nbody._device())
        if not inv:
            mesh = nbody.rfftn(mesh) if precond == 'real' else utils.rg2cgh(mesh)
            mesh = mesh * tr
        else:
            mesh = nbody._c64(mesh)
            mesh = torch.where(tr != 0, mesh / torch.where(tr != 0, tr, torch.ones_like(tr)), torch.zeros_like(mesh))
            mesh = nbody.irfftn(mesh) if precond == 'real' else utils.cgh2rg(mesh)
        return {out_name: mesh}
    return {}


def samp2base_mesh_vjp(base_bar, precond, transfer, temp=1.):
    """VJP of samp2base_mesh (forward direction): cotangent of the base mesh (complex, real-pair convention) -> cotangent
    of the real sample mesh."""
    tr = torch.as_tensor(np.asarray(transfer, dtype=np.float32) * temp ** .5, device=nbody._device())
    kb = nbody._c64(base_bar) * tr
    return nbody.rfftn_vjp(kb) if precond == 'real' else utils.rg2cgh_vjp(kb)


# ------------------------------------------------------------------------------------------------
# Catalogue -> count, selection and mask meshes (bricks.py:882-1103).  The per-object coordinate chains, the footprint and the
# reductions are the HIP passes of csrc/catalog.hip; the paints are nbody.nufft.  A catalogue is a dict-like of equally long columns
# (a dict, an open .npz, a structured array), or a list / tuple of them; objects go to the device at most `chunk` at a time, and
# paints and footprints accumulate across chunks, so device memory is bounded by the meshes plus one chunk.
CATALOG_CHUNK = 1 << 24


def radecz2cart(cosmo, radecz):
    """RA, DEC (degrees), Z dict-like -> cartesian array (N, 3) in Mpc/h (bricks.py:882-890); host float64."""
    radius = nbody.a2chi(cosmo, 1 / (1 + np.asarray(radecz['Z'], dtype=np.float64)))
    return utils.radecrad2cart(radecz['RA'], radecz['DEC'], radius)


def cart2radecz(cosmo, cart):
    """Cartesian array (Mpc/h) -> RA, DEC (degrees), Z dict (bricks.py:892-899); host float64."""
    ra, dec, radius = utils.cart2radecrad(cart)
    return {'RA': ra, 'DEC': dec, 'Z': 1 / nbody.chi2a(cosmo, radius) - 1}


def minmax_box(pos):
    """(size, center, rotvec) of the axis-aligned box spanned by the positions (bricks.py:993-1002); host float64."""
    pos = np.asarray(pos, dtype=np.float64)
    low_corner, high_corner = pos.min(0), pos.max(0)
    return high_corner - low_corner, (low_corner + high_corner) / 2, np.zeros(pos.shape[-1])


def get_mesh_shape(box_size, cell_budget, padding=0.):
    """Mesh shape (even integers) and cell length for a box size and a cell budget, with an optional padded fraction
    (bricks.py:1004-1012).  The input is not modified."""
    box_size = np.multiply(box_size, 1 + padding)
    cell_length = float((box_size.prod() / cell_budget) ** (1 / 3))
    mesh_shape = 2 * np.rint(box_size / cell_length / 2).astype(int)
    return tuple(map(int, mesh_shape)), cell_length


def _is_table(d):
    return hasattr(d, "keys") or getattr(getattr(d, "dtype", None), "names", None) is not None


def _has(table, key):
    return key in (table.keys() if hasattr(table, "keys") else table.dtype.names)


def catalog_tables(data, what="data", iterable_ok=False):
    """`data` as a sequence of dict-likes: a dict-like itself, a list or a tuple of them, or (iterable_ok: full sky, where one pass
    is enough) any iterable of them.  A one-shot iterator is refused otherwise: a cut-sky catalogue is read more than once."""
    if _is_table(data):
        return [data]
    if isinstance(data, (list, tuple)):
        if not all(_is_table(d) for d in data):
            raise TypeError(f"{what}: every chunk must be a dict-like of columns")
        return list(data)
    if iterable_ok and hasattr(data, "__iter__"):
        return data
    raise TypeError(f"{what} must be a dict-like of columns, or a list or tuple of them (it is read more than once, so a one-shot "
                    f"iterator cannot serve), got {type(data).__name__}")


def _column(table, key, what):
    if not _has(table, key):
        raise KeyError(f"{what}: column {key!r} is missing")
    return np.asarray(table[key])


def _checked_weights(w, what):
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError(f"{what}: WEIGHT must be one-dimensional")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"{what}: WEIGHT must be finite and non-negative")
    return w


def check_catalog(tables, keys, what="data", optional=()):
    """Host checks of every chunk before anything is uploaded: the columns `keys` exist with one length and finite values (the
    bounding box's fmin / fmax would pass over a NaN and the paint would then meet it), 'pos' is (N, 3), an `optional` column that
    is there has the shape of the first one and finite values, weights are finite and >= 0."""
    for t in tables:
        if not _is_table(t):
            raise TypeError(f"{what}: every chunk must be a dict-like of columns")
        cols = [_column(t, k, what) for k in keys]
        n = len(cols[0])
        if any(len(c) != n for c in cols):
            raise ValueError(f"{what}: columns {keys} differ in length")
        if keys[0] == 'pos' and (cols[0].ndim != 2 or cols[0].shape[1] != 3):
            raise ValueError(f"{what}: pos must have shape (N, 3)")
        names = list(keys)
        for k in optional:
            if _has(t, k):
                cols.append(np.asarray(t[k]))
                names.append(k)
                if cols[-1].shape != cols[0].shape:
                    raise ValueError(f"{what}: {k} must have the shape of {keys[0]}, got {cols[-1].shape} against {cols[0].shape}")
        for k, c in zip(names, cols):
            if not np.all(np.isfinite(c)):
                raise ValueError(f"{what}: {k} must be finite")
        if _has(t, 'WEIGHT') and len(_checked_weights(t['WEIGHT'], what)) != n:
            raise ValueError(f"{what}: WEIGHT and {keys[0]} differ in length")


class _Checked(list):
    """Catalogue tables that check_catalog has passed: the bricks below take them as they are."""


def checked_tables(data, keys, what="data", optional=(), iterable_ok=False):
    """catalog_tables(data) with every table checked ONCE, here, where the catalogue enters (check_catalog scans every column, which
    at 1e8-1e9 objects is real host time): the passes over the tables then only slice.  A lazily consumed iterable (iterable_ok) is
    checked table by table as it is read; tables already checked are returned as they are."""
    if isinstance(data, _Checked):
        return data
    tables = catalog_tables(data, what, iterable_ok)
    if not isinstance(tables, list):
        return _checked_lazily(tables, keys, what, optional)
    check_catalog(tables, keys, what, optional)
    return _Checked(tables)


def _checked_lazily(tables, keys, what, optional):
    for t in tables:
        check_catalog([t], keys, what, optional)
        yield t


SKY_KEYS = ('RA', 'DEC', 'Z')


def _pieces(tables, keys, chunk, optional=()):
    """Dicts of host columns of checked tables, at most `chunk` objects each, in catalogue order."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be a positive number of objects")
    for t in tables:
        cols = {k: np.asarray(t[k]) for k in keys + tuple(optional) + ('WEIGHT',) if k in keys or _has(t, k)}
        n = len(cols[keys[0]])
        for i in range(0, n, chunk):
            yield {k: v[i:i + chunk] for k, v in cols.items()}


def weighted_size(tables, key='RA'):
    """Sum of the WEIGHT column over checked tables in host float64, an object without one counting 1 (the length of column `key`)."""
    return math.fsum(float(np.sum(t['WEIGHT'], dtype=np.float64)) if _has(t, 'WEIGHT') else float(len(t[key])) for t in tables)


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(nbody._device())


def _cell_geom(box_center, box_rotvec, box_size, mesh_shape):
    """geom18 of include/mcpm.h: box_center, the matrix of box_rotvec (row-major), box_size, mesh_shape."""
    g = np.concatenate([np.asarray(box_center, dtype=np.float64).reshape(3), rot_matrix(box_rotvec).reshape(9),
                        np.asarray(box_size, dtype=np.float64).reshape(3), np.asarray(mesh_shape, dtype=np.float64).reshape(3)])
    if not np.all(np.isfinite(g)) or np.any(g[12:] <= 0):
        raise ValueError("box_center, box_rotvec, box_size and mesh_shape must be finite, box_size and mesh_shape positive")
    return g


def _radecz_dev(radecz):
    ra, dec, z = (_up(radecz[k], np.float64) for k in ('RA', 'DEC', 'Z'))
    if ra.ndim != 1 or dec.shape != ra.shape or z.shape != ra.shape:
        raise ValueError("RA, DEC and Z must be one-dimensional and equally long")
    return ra, dec, z


def sky_extent(cosmo, radecz, weights=None):
    """(low corner (3,), high corner (3,), weight sum) of radecz2cart(cosmo, radecz), all float64, in one pass on the device
    (mcpm_sky2cart_minmax_f64); no objects: (+inf, -inf, 0)."""
    ra, dec, z = _radecz_dev(radecz)
    tab = tables.on_device(cosmo, tables.DISTANCE, ra.device)
    w = None if weights is None else _up(weights, np.float64)
    if w is not None and w.shape != ra.shape:
        raise ValueError("weights must be as long as RA")
    out = torch.empty(7, dtype=torch.float64, device=ra.device)
    nbody.get_plan((8, 8, 8)).call("mcpm_sky2cart_minmax_f64", ra, dec, z, ra.numel(), tab.t, tab.v["chi_dist"], tab.n["a_dist"], w, out, out[6:])
    out = out.cpu().numpy()
    return out[:3], out[3:6], float(out[6])


def sky2cell_pos(cosmo, radecz, box_center, box_rotvec, box_size, mesh_shape, ratio=None):
    """phys2cell_pos(radecz2cart(cosmo, radecz), ...) as an (N, 3) float32 device tensor, formed in float64 and rounded once
    (mcpm_sky2cell_f32).  With `ratio` (3,): also that tensor times float32(ratio), the positions at another mesh shape."""
    ra, dec, z = _radecz_dev(radecz)
    tab = tables.on_device(cosmo, tables.DISTANCE, ra.device)
    geom = _cell_geom(box_center, box_rotvec, box_size, mesh_shape)
    out = torch.empty((ra.numel(), 3), dtype=torch.float32, device=ra.device)
    out2 = None if ratio is None else torch.empty_like(out)
    ratio = None if ratio is None else np.ascontiguousarray(ratio, dtype=np.float64).reshape(3)
    nbody.get_plan(mesh_shape).call("mcpm_sky2cell_f32", ra, dec, z, ra.numel(), tab.t, tab.v["chi_dist"], tab.n["a_dist"], geom, ratio, out, out2)
    return out if ratio is None else (out, out2)


def box2cell_pos(pos, vel, los, vscale, box_center, box_rotvec, box_size, mesh_shape):
    """phys2cell_pos(pos + vscale (vel . los) los, ...) as an (N, 3) float32 device tensor (mcpm_box2cell_f32); `vel` may be None.
    float32 input stays float32 on the way to the device, anything else travels as float64; the arithmetic is float64."""
    dt = np.float32 if np.asarray(pos).dtype == np.float32 else np.float64
    p = _up(pos, dt)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("pos must have shape (N, 3)")
    v = None if vel is None else _up(vel, dt)
    if v is not None and v.shape != p.shape:
        raise ValueError("vel must have the shape of pos")
    geom = _cell_geom(box_center, box_rotvec, box_size, mesh_shape)
    out = torch.empty((p.shape[0], 3), dtype=torch.float32, device=p.device)
    nbody.get_plan(mesh_shape).call("mcpm_box2cell_f32", p, v, int(dt is np.float64), p.shape[0], geom,
                                    np.ascontiguousarray(los, dtype=np.float64).reshape(3), float(vscale), out)
    return out


def footprint(pos, shape, weights=None, order: int = 2, mask=None):
    """Cells where an object of positive weight has a non-zero assignment weight: `paint(pos, shape, weights, order) > 0` of
    bricks.py:1045 made exact (mcpm_footprint_u8; the paints here deposit through integer accumulators, where a small positive
    deposit can round to zero).  uint8 device tensor of `shape`; `mask`: a previous result to add to (chunks)."""
    shape = tuple(int(s) for s in shape)
    plan, p, n, mode = nbody._pos_args(pos, shape)
    if mode != _lib.POS_ABSOLUTE:
        raise TypeError("footprint takes plain (N, 3) positions")
    w = None if weights is None else nbody._f32(weights, (n,))
    acc = mask is not None
    if acc and (tuple(mask.shape) != shape or mask.dtype != torch.uint8):
        raise ValueError("mask must be a uint8 tensor of the mesh shape")
    mask = mask if acc else torch.empty(shape, dtype=torch.uint8, device=p.device)
    plan.call("mcpm_footprint_u8", p, n, w, int(order), mask, int(acc))
    return mask


def masked_sum(mesh, mask):
    """(float64 sum of `mesh` over mask != 0, number of such cells), in a fixed order (mcpm_masked_sum_f64)."""
    m = nbody._f32(mesh)
    k = torch.as_tensor(mask).to(device=m.device).contiguous()
    if k.dtype not in (torch.uint8, torch.bool) or k.shape != m.shape:
        raise ValueError("mask must be a bool or uint8 array of the mesh's shape")
    out = torch.empty(2, dtype=torch.float64, device=m.device)
    nbody.get_plan((8, 8, 8)).call("mcpm_masked_sum_f64", m, k, m.numel(), out)
    s, c = out.cpu().numpy()
    return float(s), int(c)


def _catalog_extent(tables, cosmo, chunk=CATALOG_CHUNK):
    """(low corner, high corner, weighted size) of checked sky tables, chunk by chunk; objects without WEIGHT count 1."""
    lo, hi, wsum = np.full(3, np.inf), np.full(3, -np.inf), 0.
    for piece in _pieces(tables, SKY_KEYS, chunk):
        l, h, s = sky_extent(cosmo, piece, piece.get('WEIGHT'))
        lo, hi = np.minimum(lo, l), np.maximum(hi, h)
        wsum += s if 'WEIGHT' in piece else float(len(piece['RA']))
    return lo, hi, wsum


def _cutsky_box(data, cosmo, cell_budget, padding, box_size, box_center, box_rotvec, chunk, what="data"):
    """cutsky2config's answer and the weighted size of the catalogue, which the same pass over it yields."""
    lo, hi, wsum = _catalog_extent(checked_tables(data, SKY_KEYS, what), cosmo, chunk)
    if not np.all(np.isfinite(lo)):
        raise ValueError(f"the {what} catalogue is empty")
    computed = (hi - lo, (lo + hi) / 2, np.zeros(3))
    provided = (box_size, box_center, box_rotvec)
    box_size, box_center, box_rotvec = (np.array(prov, dtype=np.float64) if prov is not None else comp
                                        for prov, comp in zip(provided, computed))
    final_shape, cell_length = get_mesh_shape(box_size, cell_budget, padding)
    return final_shape, cell_length, box_center, box_rotvec, wsum


def cutsky2config(data, cosmo, cell_budget: float, padding: float = 0., box_size=None, box_center=None, box_rotvec=None,
                  chunk=CATALOG_CHUNK):
    """(final_shape, cell_length, box_center, box_rotvec) of the box around a sky catalogue (bricks.py:1015-1026): what is not
    given comes from the catalogue's bounding box.  box_size may change afterwards, to final_shape * cell_length."""
    return _cutsky_box(data, cosmo, cell_budget, padding, box_size, box_center, box_rotvec, chunk)[:4]


def _weights32(piece):
    """The paints' weights: the float32 of the WEIGHT column, or the scalar 1."""
    return _up(piece['WEIGHT'], np.float32) if 'WEIGHT' in piece else 1.


def cutsky2selection(data, cosmo, mask_shape, selec_shape, paint_shape, box_size, box_center, box_rotvec, paint_order: int = 2,
                     interlace_order: int = 2, paint_deconv: bool = True, chunk=CATALOG_CHUNK):
    """(selec_mesh at selec_shape, mask_mesh at mask_shape) painted from a sky catalogue of randoms (bricks.py:1028-1051); device
    tensors, float32 and bool.  The selection is normalised to unit mean over its own footprint at selec_shape
    (mcpm_masked_sum_f64); the mask is the footprint of the same float32 positions scaled to mask_shape."""
    mask_shape, selec_shape = tuple(int(s) for s in mask_shape), tuple(int(s) for s in selec_shape)
    ratio = np.divide(mask_shape, selec_shape)
    spec, fp_selec, fp_mask = None, None, None
    for piece in _pieces(checked_tables(data, SKY_KEYS, "random"), SKY_KEYS, chunk):
        pos, pos_mask = sky2cell_pos(cosmo, piece, box_center, box_rotvec, box_size, selec_shape, ratio)
        w = _weights32(piece)
        part = nbody.nufft(pos, selec_shape, paint_shape, weights=w, paint_order=paint_order, interlace_order=interlace_order,
                           paint_deconv=paint_deconv)
        spec = part if spec is None else spec + part
        wf = w if torch.is_tensor(w) else None
        fp_selec = footprint(pos, selec_shape, wf, paint_order, fp_selec)
        fp_mask = footprint(pos_mask, mask_shape, wf, paint_order, fp_mask)
    if spec is None:
        raise ValueError("cutsky2selection: the catalogue is empty")
    selec_mesh = nbody.irfftn(spec)
    total, cells = masked_sum(selec_mesh, fp_selec)
    if cells == 0:
        raise ValueError("cutsky2selection: no object has a positive weight")
    selec_mesh /= total / cells
    return selec_mesh, fp_mask.bool()


def cutsky2count(data, cosmo, count_shape, paint_shape, box_size, box_center, box_rotvec, paint_order: int = 2,
                 interlace_order: int = 2, paint_deconv: bool = True, chunk=CATALOG_CHUNK):
    """Count mesh at count_shape painted from a sky catalogue (bricks.py:1054-1069); float32 device tensor."""
    count_shape = tuple(int(s) for s in count_shape)
    spec = None
    for piece in _pieces(checked_tables(data, SKY_KEYS), SKY_KEYS, chunk):
        pos = sky2cell_pos(cosmo, piece, box_center, box_rotvec, box_size, count_shape)
        part = nbody.nufft(pos, count_shape, paint_shape, weights=_weights32(piece), paint_order=paint_order,
                           interlace_order=interlace_order, paint_deconv=paint_deconv)
        spec = part if spec is None else spec + part
    if spec is None:
        raise ValueError("cutsky2count: the catalogue is empty")
    return nbody.irfftn(spec)


def fullsky2count(data, cosmo, a_obs: float, los, box_size, box_center, box_rotvec, final_shape, paint_shape, paint_order: int = 2,
                  interlace_order: int = 2, paint_deconv: bool = True, chunk=CATALOG_CHUNK):
    """Count mesh at final_shape from cartesian positions in a periodic box (bricks.py:1072-1103); float32 device tensor.  `data`: a
    dict-like with 'pos' (and optional 'vel', 'WEIGHT'), or any iterable of them, accumulated in Fourier space.  With 'vel', redshift-
    space distortion at `a_obs` along `los`.  RuntimeError if the mesh does not sum to the weighted number of objects to 1e-5."""
    final_shape = tuple(int(s) for s in final_shape)
    vscale = 1. / (a_obs * 100 * float(nbody._Esqr(cosmo, a_obs)) ** .5)      # peculiar velocity -> Mpc/h
    spec, n_tracers = None, 0.
    for piece in _pieces(checked_tables(data, ('pos',), optional=('vel',), iterable_ok=True), ('pos',), chunk, optional=('vel',)):
        pos = box2cell_pos(piece['pos'], piece.get('vel'), los, vscale, box_center, box_rotvec, box_size, final_shape)
        part = nbody.nufft(pos, final_shape, paint_shape, weights=_weights32(piece), paint_order=paint_order,
                           interlace_order=interlace_order, paint_deconv=paint_deconv)
        spec = part if spec is None else spec + part
        n_tracers += float(np.sum(piece['WEIGHT'], dtype=np.float64)) if 'WEIGHT' in piece else float(len(piece['pos']))
    if spec is None:
        raise ValueError("fullsky2count: the catalogue is empty")
    count_mesh = nbody.irfftn(spec)
    total = float(count_mesh.sum(dtype=torch.float64))      # nufft applies the final -> paint jacobian: the mesh sums to n_tracers
    if not abs(total - n_tracers) <= 1e-5 * n_tracers:
        raise RuntimeError(f"Count mesh sum {total} does not match number of tracers {n_tracers}.")
    return count_mesh
