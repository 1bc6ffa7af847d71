"""`FieldLevelModel.evolve` (montecosmo/model.py:686-838) on the HIP path, with its hand-written reverse sweep.

Built branches: bias_type 'lagrangian' or 'eulerian' (model.py:68, :753-754, :797-831; `FieldLevelForward(bias_type=)`), evolution 'lpt'
(scalar a_obs or light cone), 'nbody' (scalar a_obs as the reference asserts, or the light cone: every particle at the time of its Lagrangian lattice point) or 'kaiser' (any sky, scalar a_obs or light cone: bricks.py:170-231), png_type None, 'fNL' or 'bias' (local primordial
non-Gaussianity: `evolve(..., png={'fNL': ..., ...})`, model.py:688, :751-758), ap_auto None, True or False (Alcock-Paczynski:
model.py:64, :787-794; `evolve(..., ap={'alpha_iso': ..., 'alpha_ap': ...})` for False), kernel_type 'rectangular', linear power from a table (`lin_kpow`,
bricks.py:75-77) or, with lin_kpow = None, from the Eisenstein-Hu fit of the current cosmology (bricks.py:72-74; power.py).
With png_type and 'lpt' / 'nbody' the Gaussian potential phi that the likelihood's stochastic term s_ep * phi reads (model.py:837, :869, :894)
is `ctx.phi` of `evolve(..., return_ctx=True)`; `phi_final` brings it to the final mesh and `evolve_vjp(..., phi_bar=)` takes its cotangent back.
Priors, likelihood and samplers: logdensity.py, samplers.py.  Not built: the tempered prior `temp_prior` (`samp2base(temp=)`,
model.py:640-679), Alcock-Paczynski in the Kaiser model (model.py:703-729
computes the moved positions and discards them), `ap_auto_absdetjac` and `rsd_ap_auto` (no live call site in the reference).

    fwd = FieldLevelForward(final_shape=(64, 64, 64), cell_length=20., box_center=(0, 0, 2000.), evolution='nbody',
                            a_obs=0.7, lin_kpow=(ks, pows))
    gxy_mesh, ctx = fwd.evolve(cosmology, bias, white_mesh, return_ctx=True)       # gxy_mesh = 1 + delta_obs
    grads = fwd.evolve_vjp(ctx, gxy_mesh_bar)      # {'white_mesh': ..., 'bias': {...}, 'sigma8': ..., 'growth': ...}

Chain (every arrow is a HIP kernel sequence of libmcpm.so, each with its VJP):
white_mesh -white2lin-> init_mesh -chreshape-> evol mesh -lagrangian_bias-> (weights, dvel, phi); [-add_png(phi)-> -chreshape to
init_shape and back->] -lpt | nbody_bf-> (pos, vel)
-observe_pos (los, rsd, Alcock-Paczynski)-> pos on init_shape -nufft(weights, paint_shape)-> spectrum -chreshape-> -irfftn-> gxy_mesh.
bias_type 'eulerian': the particles are painted unweighted (and, with png_type, once more weighted by phi read at their Lagrangian
positions), -nufft(1 | phi_pos)-> matter / phi spectra -chreshape-> -eulerian_bias-> gxy_mesh; `lagrangian_bias` still supplies dvel and phi.
"""
from __future__ import annotations

import numpy as np
import torch

from . import nbody, bricks, metrics, tables
from ._lib import Ctx as EvolveCtx
from .utils import scale_shape, r2chshape, chreshape, chreshape_vjp


class FieldLevelForward:
    def __init__(self, final_shape=(64, 64, 64), cell_length=20., box_center=(0., 0., 0.), box_rotvec=(0., 0., 0.),
                 evolution='lpt', nbody_a_start=0., nbody_n_steps=10, lpt_order=2, paint_order=2, paint_deconv=True,
                 init_oversamp=3 / 2, evol_oversamp=7 / 4, ptcl_oversamp=7 / 4, paint_oversamp=7 / 4, interlace_order=2,
                 a_obs=None, curved_sky=True, lin_kpow=None, png_type=None, ap_auto=None, cosmo_fid=None, bias_type='lagrangian'):
        if bias_type not in ('lagrangian', 'eulerian'):
            raise ValueError("bias_type must be 'lagrangian' or 'eulerian'")
        self.bias_type = bias_type      # evolution 'kaiser' ignores it, as in the reference (model.py:690-696)
        if evolution not in ('kaiser', 'lpt', 'nbody'):
            raise ValueError("evolution must be 'kaiser', 'lpt' or 'nbody'")
        if png_type not in (None, 'fNL', 'bias'):
            raise ValueError("png_type must be None, 'fNL' or 'bias'")
        self.png_type = png_type
        if ap_auto is not None and evolution == 'kaiser':
            raise NotImplementedError("Alcock-Paczynski is not built for the Kaiser model: the reference's branch (model.py:703-729) "
                                      "computes the moved positions and discards them")
        if ap_auto and cosmo_fid is None:
            raise ValueError("ap_auto=True needs the fiducial cosmology `cosmo_fid` (the one the catalogue was gridded with)")
        # None: no Alcock-Paczynski; True: automatic, from the sampled and the fiducial cosmology; False: alpha_iso / alpha_ap (model.py:64)
        self.ap_auto = None if ap_auto is None else bool(ap_auto)
        self.cosmo_fid = cosmo_fid
        self.final_shape = tuple(int(s) for s in final_shape)
        self.cell_length = float(cell_length)
        self.box_center = np.asarray(box_center, dtype=np.float64)
        self.box_rotvec = np.asarray(box_rotvec, dtype=np.float64)
        self.box_size = np.multiply(self.final_shape, self.cell_length)            # model.py:568-573
        self.init_shape = scale_shape(self.final_shape, init_oversamp)
        self.evol_shape = scale_shape(self.final_shape, evol_oversamp)
        self.ptcl_shape = scale_shape(self.final_shape, ptcl_oversamp)
        self.paint_shape = scale_shape(self.final_shape, paint_oversamp)
        self.evolution, self.nbody_a_start, self.nbody_n_steps = evolution, float(nbody_a_start), int(nbody_n_steps)
        self.lpt_order, self.paint_order, self.paint_deconv = int(lpt_order), int(paint_order), bool(paint_deconv)
        self.interlace_order, self.a_obs, self.curved_sky = int(interlace_order), a_obs, bool(curved_sky)
        # lin_kpow = (ks, pows) normalised to sigma8 = 1, or None: the Eisenstein-Hu power of the CURRENT cosmology
        # (bricks.py:69-79; montecosmo_amd/power.py), re-tabulated whenever Omega_m / Omega_b / h / n_s change
        self.lin_kpow = None if lin_kpow is None else (np.asarray(lin_kpow[0], dtype=np.float64), np.asarray(lin_kpow[1], dtype=np.float64))
        self._r0 = self._r_min = self._los_cell = None

    def config(self):
        """The model attributes as a dict (what the parity tests hand to their float64 checker)."""
        keys = ("init_shape", "evol_shape", "ptcl_shape", "paint_shape", "box_size", "box_center", "box_rotvec", "a_obs",
                "curved_sky", "evolution", "nbody_a_start", "nbody_n_steps", "lpt_order", "paint_order", "paint_deconv",
                "interlace_order", "lin_kpow", "bias_type")
        return {k: getattr(self, k) for k in keys}

    @classmethod
    def register_catalog(cls, cell_budget: float, cosmo_fid, data, random=None, **kwargs):
        """register.register_catalog under the reference's name (model.py:1287-1362): catalogue -> register dict, no model instance needed."""
        from .register import register_catalog
        return register_catalog(cell_budget, cosmo_fid, data, random, **kwargs)

    # ---- metrics (model.py:1370-1379) ----------------------------------------------------------------------
    def spectrum(self, mesh0, mesh1=None, ells: int | list = 0, kedges: int | float | list = None, include_corners=True):
        """metrics.spectrum with the model's box_size and box_center."""
        return metrics.spectrum(mesh0, mesh1=mesh1, box_size=self.box_size, box_center=self.box_center, ells=ells, kedges=kedges,
                                include_corners=include_corners)

    def powtranscoh(self, mesh0, mesh1, kedges: int | float | list = None, include_corners=True):
        """(k, pow1, (pow1 / pow0)^.5, pow01 / (pow0 pow1)^.5) with the model's box_size; a batched mesh1 gives batched outputs."""
        return metrics.powtranscoh(mesh0, mesh1, box_size=self.box_size, kedges=kedges, include_corners=include_corners)

    def powtranscoh_chains(self, chains, mesh0, names: str | list = (), kedges: int | float | list = None):
        """A copy of `chains` (chains.Chains) with, for every entry `name` of meshes (C, N, *mesh), the tuple `kptc_<name>` =
        powtranscoh(mesh0, mesh) per draw, each of shape (C, N, bins) (model.py:1429-1442): the chain and draw axes go through the
        batch axis of metrics.powtranscoh together."""
        out = chains.copy()
        for name in np.atleast_1d(names):
            x = torch.as_tensor(chains[str(name)])
            c, n = x.shape[:2]
            res = self.powtranscoh(mesh0, x.reshape((c * n,) + tuple(x.shape[2:])), kedges=kedges)
            out[f"kptc_{name}"] = tuple(r.reshape((c, n) + r.shape[1:]) for r in res)
        return out

    def bispectrum(self, mesh, kedges: int | float | list = None, triangles=None, deconv: int = 0, reduced=False):
        """metrics.bispectrum with the model's box_size: (tri, kmean, ntri, bk[, qk]); a batched mesh gives batched bk and qk."""
        return metrics.bispectrum(mesh, box_size=self.box_size, kedges=kedges, triangles=triangles, deconv=deconv, reduced=reduced)

    def bispectrum_chains(self, chains, names: str | list = (), kedges: int | float | list = None, triangles=None, reduced=False):
        """A copy of `chains` (chains.Chains) with, for every entry `name` of meshes (C, N, *mesh), the tuple `kb_<name>` =
        (tri, kmean, ntri, bk[, qk]) of bispectrum(mesh) per draw, bk and qk of shape (C, N, T): the chain and draw axes go through the
        batch axis of metrics.bispectrum together, as in powtranscoh_chains."""
        out = chains.copy()
        for name in np.atleast_1d(names):
            x = torch.as_tensor(chains[str(name)])
            c, n = x.shape[:2]
            res = self.bispectrum(x.reshape((c * n,) + tuple(x.shape[2:])), kedges=kedges, triangles=triangles, reduced=reduced)
            out[f"kb_{name}"] = res[:3] + tuple(r.reshape((c, n) + r.shape[1:]) for r in res[3:])
        return out

    def mse_value(self, mesh0, mesh1, cell_length=None, vedges: int | float | list = 50, min_count=None, aggr_fn=None):
        """metrics.mse_value with the model's cell_length (model.py:1390-1394): by default 50 quantile bins of mesh0."""
        return metrics.mse_value(mesh0, mesh1, self.cell_length if cell_length is None else cell_length, vedges=vedges, min_count=min_count,
                                 aggr_fn=aggr_fn)

    def mse_wave(self, mesh0, mesh1, kedges: int | float | list = None, include_corners=True):
        """metrics.mse_wave with the model's box_size (model.py:1396-1397)."""
        return metrics.mse_wave(mesh0, mesh1, self.box_size, kedges=kedges, include_corners=include_corners)

    # ---- data (model.py:1249-1257) ----------------------------------------------------------------------------
    def pos_mesh(self, shape=None):
        """Physical positions of the cells of a mesh of `shape` (default final_shape): host float64, shape + (3,)."""
        shape = self.final_shape if shape is None else tuple(int(s) for s in shape)
        p = bricks.cell2phys_pos(bricks.regular_pos(shape), self.box_center, self.box_rotvec, self.box_size, shape)
        return np.asarray(p, dtype=np.float64).reshape(shape + (3,))

    def radius_mesh(self, shape=None):
        """Physical distance of the cells of a mesh of `shape` (default final_shape): `lattice_radius` as a mesh, host float64; |x| on the
        curved sky, |x . los| on the flat one."""
        shape = self.final_shape if shape is None else tuple(int(s) for s in shape)
        return np.asarray(self.lattice_radius(shape), dtype=np.float64).reshape(shape)

    # ---- pieces ------------------------------------------------------------------------------------------
    def _kphys(self, shape):
        return [float(s) / float(b) for s, b in zip(shape, self.box_size)]

    def _power_mult(self, spec, cosmo, sigma8=None):
        """white2lin (bricks.py:149-154): spec * sqrt(sigma8^2 P(|k|)); real multiplier, self-adjoint.  `sigma8` overrides the
        cosmology's (1.0 gives d init_mesh / d sigma8, which stays finite where a bounded latent has walked to sigma8 = 0)."""
        return bricks.power_mult(nbody.get_plan(self.init_shape), spec, self._kphys(self.init_shape), cosmo, self.lin_kpow,
                                 cosmo.sigma8 if sigma8 is None else sigma8, torch.empty_like(spec))

    def los_cell(self):
        """Line of sight (the direction of the box centre) in cell axes (model.py:607-608); host float64, computed once."""
        if self._los_cell is None:
            self._los_cell = bricks.rot_matrix(self.box_rotvec).T @ nbody.safe_div(self.box_center, np.linalg.norm(self.box_center))
        return self._los_cell

    def lattice_radius(self, mesh_shape, ptcl_shape=None, flat_dot=np.matmul):
        """Physical distance of the points of a regular lattice (bricks.py:665-686), flat host float64 array: |x| on the curved sky, |x . los|
        on the flat one (`flat_dot` forms the product)."""
        p = bricks.cell2phys_pos(bricks.regular_pos(mesh_shape, ptcl_shape), self.box_center, self.box_rotvec, self.box_size, mesh_shape)
        if self.curved_sky:
            return np.linalg.norm(p, axis=-1)
        return np.abs(flat_dot(p, nbody.safe_div(self.box_center, np.linalg.norm(self.box_center))))

    def _scale_factors(self, cosmo):
        """Scale factor(s) of the Lagrangian lattice (model.py:741-742): a_obs, or chi2a(|x|) per particle as a device
        tensor (N,1).  The lattice is fixed, so its physical distances are computed once (host float64) and kept on
        the device; the cosmology-dependent look-up runs there (mcpm_interp_f32)."""
        if self.a_obs is not None:
            return self.a_obs
        if self._r0 is None:
            # the flat-sky product is summed per row here and by `@` in the log density: the two differ in the last bit of a float64,
            # and each consumer keeps the bits it has always had
            r0 = self.lattice_radius(self.evol_shape, self.ptcl_shape, flat_dot=lambda p, los: (p * los).sum(-1))
            self._r_min = float(r0.min())      # host float64: the nearest lattice point ends the N-body run on the light cone (`_a_end`)
            self._r0 = nbody._f32(r0)
        c = tables.on_device(cosmo, tables.CHI2A, self._r0.device)
        return nbody.interp_dev(self._r0, c.v["chi"], c.v["a_of_chi"]).reshape(-1, 1)

    def _a_end(self, cosmo):
        """End of the N-body run on the light cone: the scale factor of the nearest lattice point, chi2a(cosmo, r_min) -- host float64 from
        the cached lattice radii (no device synchronisation).  It moves with the cosmology: cosmo_vjp's central differences recompute it."""
        if self._r_min is None:
            self._scale_factors(cosmo)
        return float(nbody.chi2a(cosmo, self._r_min))

    # ---- Kaiser model: growth, Eulerian linear bias and RSD.  Flat sky at fixed a (bricks.py:170-198): diagonal in k, `_kaiser`;
    # curved sky and / or light cone (bricks.py:200-231): a real-space pass with a line of sight and a growth factor per cell, `_kaiser_sky` ----
    def _mu2_mesh(self, device):
        """(k . los)^2 / k^2 on the half-spectrum of the evolution mesh, los = the box centre's direction in cell axes."""
        if getattr(self, "_mu2", None) is None:
            kvec = nbody.rfftk(self.evol_shape, self.box_size)
            kk = sum(k ** 2 for k in kvec)
            mu2 = nbody.safe_div(sum(k * l for k, l in zip(kvec, self.los_cell())) ** 2, kk)
            self._mu2 = torch.from_numpy(np.ascontiguousarray(mu2, dtype=np.float32)).to(device)
        return self._mu2

    def _png_div(self, spec, cosmo, scale):
        """scale * safe_div(spec, t(|k|)) on the evolution mesh, t from `lin_kpow` as the reference's Kaiser model takes it."""
        tab, nt = bricks._png_table(cosmo, self.lin_kpow, spec.device)
        out, kp = torch.empty_like(spec), self._kphys(self.evol_shape)
        nbody.get_plan(self.evol_shape).call("mcpm_png_div_f32", spec, kp[0], kp[1], kp[2], tab, tab[nt:], nt, float(scale), out)
        return out

    def _kaiser(self, cosmo, bias, white, evol_k, return_ctx, png=None):
        if self.curved_sky or self.a_obs is None:
            return self._kaiser_sky(cosmo, bias, white, evol_k, return_ctx, png=png)
        D, f = float(nbody.a2g(cosmo, self.a_obs)), float(nbody.a2f(cosmo, self.a_obs))
        mu2 = self._mu2_mesh(evol_k.device)
        boost = D * ((1.0 + float(bias["b1"])) + f * mu2)                 # b1E = 1 + b1 (bricks.py:454)
        gxy_k = evol_k * boost
        if png is not None:      # boost += safe_div(fNL_bp, t) (bricks.py:181-183)
            gxy_k = gxy_k + self._png_div(evol_k, cosmo, png["fNL_bp"])
        gxy = nbody.irfftn(gxy_k) + 1.0
        cosmo._workspace = {}
        if return_ctx:
            return gxy, EvolveCtx(cosmo=cosmo, white=white, evol_k=evol_k, kaiser=(D, f, float(bias["b1"]), boost), png=png, bias=bias)
        return gxy

    def _kaiser_sky(self, cosmo, bias, white, evol_k, return_ctx, png=None):
        """bricks.kaiser_sky on the evolution mesh (model.py:690-695); the PNG term fNL_bp phi with the table of `lin_kpow`."""
        gxy, sky = bricks.kaiser_sky(cosmo, evol_k, self.box_size, self.box_center, self.box_rotvec, 1.0 + float(bias["b1"]),
                                     fNL_bp=None if png is None else png["fNL_bp"], a_obs=self.a_obs, curved_sky=self.curved_sky,
                                     kpow=self.lin_kpow, return_ctx=True)
        # the growth-table Jacobian of cosmo_vjp at fixed a_obs: host work done while the device runs the forward pass (see `evolve`)
        fd = self._cosmo_scalar_fd(cosmo, self.cosmo_fd_params) if (return_ctx and self.a_obs is not None and getattr(self, "cosmo_fd_params", None)) else None
        cosmo._workspace = {}
        if return_ctx:
            return gxy, EvolveCtx(cosmo=cosmo, white=white, evol_k=evol_k, sky=sky, scalar_fd=fd, png=png, bias=bias)
        return gxy

    def _kaiser_sky_vjp(self, ctx, gxy_bar):
        cosmo = ctx.cosmo
        r = bricks.kaiser_sky_vjp(ctx.sky, nbody._f32(gxy_bar, self.evol_shape))
        evol_b, extra = r["lin_mesh"], {}
        bias_bar = {k: 0.0 for k in bricks.BIAS_KEYS}
        bias_bar["b1"] = r["b1E"]
        if ctx.png is not None:
            png_bar, bb = bricks.fNL_bias_vjp(ctx.png_in, ctx.bias, {"fNL_bp": r["fNL_bp"]}, p=1., png_type=self.png_type)
            bias_bar["b1"] += bb["b1"]
            bias_bar["b2"] += bb["b2"]
            extra = {"png": png_bar, "trans_bar": r["trans_bar"]}
        init_b = chreshape_vjp(evol_b, r2chshape(self.init_shape))
        white_b = self._power_mult(init_b, cosmo)
        s8b = float((init_b.conj() * self._power_mult(ctx.white, cosmo, sigma8=1.0)).real.sum().item())
        # fixed a_obs: cotangents of a2g(a_obs), a2f(a_obs); light cone: of the chi nodes of chi2a and of the growth tables (cosmo_vjp)
        kaiser = {"g": r["g"], "f": r["f"]} if self.a_obs is not None else r["tables"]
        return {"white_mesh": white_b, "bias": bias_bar, "sigma8": s8b, "init_bar": init_b, "kaiser": kaiser, **extra}

    def _kaiser_vjp(self, ctx, gxy_bar):
        if getattr(ctx, "sky", None) is not None:
            return self._kaiser_sky_vjp(ctx, gxy_bar)
        cosmo = ctx.cosmo
        D, f, b1, boost = ctx.kaiser
        gb = nbody._f32(gxy_bar, self.evol_shape)
        kb = nbody.irfftn_vjp(gb)
        prod = kb.conj() * ctx.evol_k
        c0 = float(prod.real.double().sum())                              # d/d(D b1E)
        c1 = float((prod.real * self._mu2_mesh(kb.device)).double().sum())    # d/d(D f)
        evol_b, extra = kb * boost, {}
        bias_bar = {k: 0.0 for k in bricks.BIAS_KEYS}
        bias_bar["b1"] = D * c0
        if getattr(ctx, "png", None) is not None:
            # the PNG term is fNL_bp phi in real space, phi = irfftn(evol_k / t): phi_bar = fNL_bp gxy_bar, pulled back to evol_k and the table
            bp_bar = float((kb.conj() * self._png_div(ctx.evol_k, cosmo, 1.0)).real.double().sum())
            tab, nt = bricks._png_table(cosmo, self.lin_kpow, kb.device)
            lb, trans_bar = bricks.png_phi_vjp(nbody.get_plan(self.evol_shape), ctx.evol_k, self._kphys(self.evol_shape), tab, nt,
                                               gb * float(ctx.png["fNL_bp"]))
            evol_b = evol_b + lb
            png_bar, bb = bricks.fNL_bias_vjp(ctx.png_in, ctx.bias, {"fNL_bp": bp_bar}, p=1., png_type=self.png_type)
            bias_bar["b1"] += bb["b1"]
            bias_bar["b2"] += bb["b2"]
            extra = {"png": png_bar, "trans_bar": trans_bar}
        init_b = chreshape_vjp(evol_b, r2chshape(self.init_shape))
        white_b = self._power_mult(init_b, cosmo)
        s8b = float((init_b.conj() * self._power_mult(ctx.white, cosmo, sigma8=1.0)).real.sum().item())
        return {"white_mesh": white_b, "bias": bias_bar, "sigma8": s8b, "init_bar": init_b,
                "kaiser": {"g": (1.0 + b1) * c0 + f * c1, "f": D * c1}, **extra}

    # ---- forward -----------------------------------------------------------------------------------------
    def evolve(self, cosmo, bias, white_mesh, png=None, return_ctx=False, ap=None):
        """cosmo: duck-typed cosmology (Omega_m, Omega_de, Omega_k, w0, wa, sigma8, _workspace); bias: dict of the
        Lagrangian bias parameters; white_mesh: complex half-spectrum of shape r2chshape(init_shape) (what
        samp2base_mesh returns); png: dict with the keys bricks.PNG_KEYS (missing = 0), read only when the model's png_type is
        set; ap: dict with 'alpha_iso', 'alpha_ap' (missing = 1), read only when the model's ap_auto is False (model.py:793).
        Returns gxy_mesh (paint_shape, float32 device tensor) = 1 + delta_obs.
        With png_type (model.py:688, :751-758): fNL_bias -> bias weights from the GAUSSIAN evolution mesh -> add_png on it (phi is
        handed over from the bias step: three extra transforms in all) -> chreshape to init_shape and back, which cuts the modes
        phi^2 filled above the initial Nyquist -> lpt / nbody.  As in the reference, the transfer table of these two steps is the
        Eisenstein-Hu one (model.py:751, :757 pass no kpow); the Kaiser model's follows `lin_kpow` (model.py:695).
        The context of an 'lpt' / 'nbody' run carries `phi`: with png_type the Gaussian potential that `lagrangian_bias` returned (the
        Gaussian evolution mesh divided by the transfer, real, evol_shape; model.py:837), else None (phi = 0)."""
        white = nbody._c64(white_mesh, r2chshape(self.init_shape))
        init_k = self._power_mult(white, cosmo)
        evol_k = chreshape(init_k, r2chshape(self.evol_shape))
        png_in = png
        png = bricks.fNL_bias(png or {}, bias, p=1., png_type=self.png_type) if self.png_type is not None else None
        if self.evolution == 'kaiser':      # gxy_mesh lives on the evolution mesh (model.py:690-696: no oversampling needed)
            res = self._kaiser(cosmo, bias, white, evol_k, return_ctx, png=png)
            if return_ctx:
                res[1].png_in = png_in or {}
            return res
        pos0 = getattr(self, "_pos0", None)      # the undisplaced lattice: built once (201 MB of zeros per call at 256^3 otherwise); never written to
        if pos0 is None:
            pos0 = self._pos0 = nbody.LatticePos.regular(self.evol_shape, self.ptcl_shape)
        a = self._scale_factors(cosmo)
        lin_k, actx = evol_k, None
        if png is None:
            (w, dvel, _), bctx = bricks.lagrangian_bias(cosmo, pos0, a, self.box_size, evol_k, bias, read_order=1, return_ctx=True)
        else:
            (w, dvel, phi), bctx = bricks.lagrangian_bias(cosmo, pos0, a, self.box_size, evol_k, bias, png=png, png_type=self.png_type,
                                                          read_order=1, return_ctx=True)
            lin_k, actx = bricks.add_png(cosmo, png["fNL"], evol_k, self.box_size, return_ctx=True, phi=phi)
            lin_k = chreshape(chreshape(lin_k, r2chshape(self.init_shape)), r2chshape(self.evol_shape))      # model.py:758
        cosmo._workspace = {}                                                        # model.py:762, :769
        if self.evolution == 'lpt':
            (dpos, vel), lctx = nbody.lpt(cosmo, lin_k, pos0, a, lpt_order=self.lpt_order, read_order=1, return_ctx=True)
            pos, nctx = pos0 + dpos, lctx      # (the LPT context rides in the N-body context's slot)
        else:
            # light cone: every particle at the scale factor of its Lagrangian lattice point (as 'lpt' does, model.py:739-741), the run ending
            # at the nearest one's
            lckw = {} if self.a_obs is not None else {"a_end": self._a_end(cosmo)}
            (pos, vel), nctx = nbody.nbody_bf(cosmo, lin_k, pos0, a0=self.nbody_a_start, a1=a, n_steps=self.nbody_n_steps,
                                              paint_order=self.paint_order, lpt_order=self.lpt_order, return_ctx=True,
                                              lattice_out=True, **lckw)
            vel = vel.reshape(-1, 3)
        # the growth-table Jacobian of cosmo_vjp: a millisecond of host work, done HERE -- the device has the whole evolution queued
        fd = self._cosmo_scalar_fd(cosmo, self.cosmo_fd_params) if (return_ctx and self.a_obs is not None and getattr(self, "cosmo_fd_params", None)) else None
        apkw = {} if self.ap_auto is None else dict(ap_auto=self.ap_auto, ap=ap, cosmo_fid=self.cosmo_fid)
        pos_c, octx = bricks.observe_pos(cosmo, pos, vel, self.box_center, self.box_rotvec, self.box_size, self.evol_shape,
                                         self.init_shape, a_obs=self.a_obs, curved_sky=self.curved_sky, dvel=dvel, return_ctx=True, **apkw)
        jac = float(np.divide(self.init_shape, self.ptcl_shape).prod())
        ectx = phi_pos = None
        if self.bias_type == 'eulerian':
            gxy, ectx, phi_pos = self._eulerian_paint(pos_c, pos0, bias, png, None if png is None else phi, jac)
        else:
            gxy_k = nbody.nufft(pos_c, self.init_shape, self.paint_shape, weights=w, paint_order=self.paint_order,
                                interlace_order=self.interlace_order, paint_deconv=self.paint_deconv)
            gxy_k = chreshape(gxy_k * jac, r2chshape(self.paint_shape))
            gxy = nbody.irfftn(gxy_k)
        if return_ctx:
            return gxy, EvolveCtx(cosmo=cosmo, white=white, evol_k=evol_k, pos0=pos0, a=a, bctx=bctx, nctx=nctx, octx=octx,
                                  pos_c=pos_c, w=w, jac=jac, scalar_fd=fd, lin_k=lin_k, actx=actx, png=png, png_in=png_in or {}, bias=bias,
                                  phi=None if png is None else phi, ectx=ectx, phi_pos=phi_pos)
        return gxy

    # ---- Eulerian bias (model.py:815-831): unweighted paint(s), then the expansion on the painted mesh ----------------------
    def _nufft_kw(self):
        return dict(paint_order=self.paint_order, interlace_order=self.interlace_order, paint_deconv=self.paint_deconv)

    def _phi_lattice(self):
        """True where the NGP read of phi at the Lagrangian lattice is the identity (the particles are the evolution mesh's own points)."""
        return tuple(self.ptcl_shape) == tuple(self.evol_shape)

    def _eulerian_paint(self, pos_c, pos0, bias, png, phi, jac):
        """-> (gxy_mesh, context of bricks.eulerian_bias, phi_pos or None).  Both paints carry the Jacobian prod(init_shape / ptcl_shape) of the
        Lagrangian branch (model.py:806): nufft returns counts per init cell and chreshape keeps the mean, so this is what makes the painted
        field mean-one; model.py:820, :827 have paint_shape there, which scales delta by (paint / init)^3."""
        kshape = r2chshape(self.paint_shape)
        mk = chreshape(nbody.nufft(pos_c, self.init_shape, self.paint_shape, weights=1., **self._nufft_kw()) * jac, kshape)
        pk = phi_pos = None
        if png is not None:      # phi advected with the particles (model.py:754, :824-828)
            phi_pos = phi.reshape(-1) if self._phi_lattice() else nbody.read(pos0, phi, order=1)
            pk = chreshape(nbody.nufft(pos_c, self.init_shape, self.paint_shape, weights=phi_pos, **self._nufft_kw()) * jac, kshape)
        gxy, ectx = bricks.eulerian_bias(mk, pk, self.box_size, bias, png, png_type=self.png_type, return_ctx=True)
        return gxy, ectx, phi_pos

    def _eulerian_paint_vjp(self, ctx, gb):
        """Cotangent of gxy_mesh -> (cotangent of pos_c from both paints, bias_bar, png_bar or None, cotangent of phi on evol_shape or None)."""
        mkb, pkb, bias_bar, png_bar = bricks.eulerian_bias_vjp(ctx.ectx, gb)
        ishape = r2chshape(self.init_shape)
        kw = dict(self._nufft_kw(), paint_shape=self.paint_shape)
        pb, _ = nbody.nufft_vjp(ctx.pos_c, self.init_shape, 1., chreshape_vjp(mkb, ishape) * ctx.jac, **kw)
        phi_b = None
        if pkb is not None:
            pb2, ppb = nbody.nufft_vjp(ctx.pos_c, self.init_shape, ctx.phi_pos, chreshape_vjp(pkb, ishape) * ctx.jac, **kw)
            pb = pb + pb2
            if self._phi_lattice():
                phi_b = ppb.reshape(self.evol_shape)
            else:      # adjoint of the NGP read w.r.t. its mesh: a weighted paint on the Lagrangian lattice
                plan, p, n, mode = nbody._pos_args(ctx.pos0, self.evol_shape)
                phi_b = torch.empty(self.evol_shape, dtype=torch.float32, device=ppb.device)
                plan.call("mcpm_paint_f32", p, n, mode, ppb.contiguous(), 1, 0.0, 1, phi_b, 0)
        return pb, bias_bar, png_bar, phi_b

    def phi_final(self, phi):
        """phi of `evolve`'s context on the final mesh: irfftn(chreshape(rfftn(phi), final_shape)) (model.py:869)."""
        if tuple(phi.shape) == self.final_shape:
            return phi
        return nbody.irfftn(chreshape(nbody.rfftn(phi), r2chshape(self.final_shape)))

    def phi_final_vjp(self, phi_bar):
        """Adjoint of `phi_final`: a final-shape cotangent -> the cotangent of phi on evol_shape."""
        if tuple(self.evol_shape) == self.final_shape:
            return phi_bar
        return nbody.rfftn_vjp(chreshape_vjp(nbody.irfftn_vjp(phi_bar), r2chshape(self.evol_shape)), overwrite=True)

    # ---- reverse sweep -----------------------------------------------------------------------------------
    def evolve_vjp(self, ctx, gxy_bar, phi_bar=None):
        """Cotangent of gxy_mesh (real, paint_shape) -> {'white_mesh': complex64 cotangent (real-pair convention),
        'bias': dict, 'sigma8': float, 'growth': cotangents of the growth scalars (see nbody.lpt_vjp / nbody_bf_vjp),
        'bias_growth': cotangent(s) of a2g(a) through the bias weights, 'gf': cotangent of a2g(a_obs) a2f(a_obs) through rsd}.
        evolution 'kaiser': 'white_mesh', 'bias', 'sigma8' and 'kaiser': {'g', 'f'}, the cotangents of a2g(a_obs), a2f(a_obs), or on the light cone
        {'chi', 'g', 'f'}, the cotangents of the chi nodes of chi2a and of the growth tables (float64 arrays).
        With ap_auto also 'ap': {'alpha_iso', 'alpha_ap'} cotangents (0 for ap_auto=True), and for ap_auto=True at fixed a_obs 'ap_chi_bar':
        the cotangent of the chi nodes of chi2a(cosmo, r') (device float64; cosmo_vjp).
        With png_type also 'png': cotangents of the six entries of the `png` dict given to evolve (the fNL_bias reparametrisation
        chained back, its b1 / b2 share added to 'bias'), and 'trans_bar': cotangent of the transfer table's entries (cosmo_vjp).
        `phi_bar` (real, final_shape; 'lpt' / 'nbody' with png_type): the cotangent of `phi_final(ctx.phi)` from the likelihood.  It is pulled back
        to evol_shape and joins the phi cotangent of the bias weights in front of `add_png_vjp`, so there is still one divide by the transfer
        table, and 'trans_bar' carries its share."""
        if self.evolution == 'kaiser':
            if phi_bar is not None:
                raise ValueError("evolution 'kaiser' defines no phi (model.py:690-696): there is nothing a phi_bar could be the cotangent of")
            return self._kaiser_vjp(ctx, gxy_bar)
        if phi_bar is not None and ctx.actx is None:
            raise ValueError("phi_bar needs a context of a model with png_type set: without it phi = 0")
        cosmo = ctx.cosmo
        gb = nbody._f32(gxy_bar, self.paint_shape)
        eul = getattr(ctx, "ectx", None) is not None
        if eul:      # the Lagrangian weights are not painted: their cotangent is zero, lagrangian_bias_vjp still pulls dvel's back
            pb, ebias_bar, epng_bar, ephi_b = self._eulerian_paint_vjp(ctx, gb)
            wb = torch.zeros_like(ctx.w)
        else:
            kb = chreshape_vjp(nbody.irfftn_vjp(gb), r2chshape(self.init_shape)) * ctx.jac
            pb, wb = nbody.nufft_vjp(ctx.pos_c, self.init_shape, ctx.w, kb, self.paint_order, self.interlace_order, self.paint_deconv,
                                     paint_shape=self.paint_shape)
        extra = {}
        if self.ap_auto is None:
            xb, vb, dvb, gfb = bricks.observe_pos_vjp(ctx.octx, pb)
        else:
            xb, vb, dvb, gfb, extra["ap"] = bricks.observe_pos_vjp(ctx.octx, pb)
            if self.ap_auto and self.a_obs is not None:      # the one new launch group: auto AP is the only per-particle table look-up here
                extra["ap_chi_bar"] = bricks.observe_pos_tables_vjp(ctx.octx, pb)
        if ctx.actx is None:
            mesh_b, bias_bar, bg_bar = bricks.lagrangian_bias_vjp(ctx.bctx, wb, dvb)
        else:
            mesh_b, bias_bar, bg_bar, png_bar, _, (phb, lpb) = bricks.lagrangian_bias_vjp(ctx.bctx, wb, dvb, defer_phi=True)
        if eul:
            for k in ("b1", "b2", "bs2", "bn2"):
                bias_bar[k] += ebias_bar[k]
            if epng_bar is not None:      # the advected phi joins the other readers of phi in front of add_png_vjp's one divide by t
                png_bar["fNL_bp"] += epng_bar["fNL_bp"]
                png_bar["fNL_bpd"] += epng_bar["fNL_bpd"]
                phb = phb + ephi_b
        if self.evolution == 'lpt':
            mb, growth = nbody.lpt_vjp(cosmo, ctx.lin_k, ctx.pos0, ctx.a, xb, vb, lpt_order=self.lpt_order, ctx=ctx.nctx)
        else:
            mb, growth = nbody.nbody_bf_vjp(ctx.nctx, xb, vb)
        if ctx.actx is not None:
            # three transforms: the cotangents of phi (bias weights and add_png) and of lap phi meet in k-space before the one divide by t
            ob = chreshape_vjp(chreshape_vjp(mb, r2chshape(self.init_shape)), r2chshape(self.evol_shape))
            if phi_bar is not None:
                phb = phb + self.phi_final_vjp(nbody._f32(phi_bar, self.final_shape))
            mb, png_bar["fNL"], trans_bar = bricks.add_png_vjp(ctx.actx, ob, phi_bar=phb, lap_phi_bar=lpb)
            png_bar, bb = bricks.fNL_bias_vjp(ctx.png_in, ctx.bias, png_bar, p=1., png_type=self.png_type)
            bias_bar["b1"] += bb["b1"]
            bias_bar["b2"] += bb["b2"]
            extra.update({"png": png_bar, "trans_bar": trans_bar})
        mesh_b = mesh_b + mb
        init_b = chreshape_vjp(mesh_b, r2chshape(self.init_shape))
        white_b = self._power_mult(init_b, cosmo)
        # d/d sigma8: init_mesh is linear in sigma8
        s8b = float((init_b.conj() * self._power_mult(ctx.white, cosmo, sigma8=1.0)).real.sum().item())
        return {"white_mesh": white_b, "bias": bias_bar, "sigma8": s8b, "growth": growth, "bias_growth": bg_bar, "gf": gfb,
                "init_bar": init_b, "obs_bar": pb if self.a_obs is None else None, **extra}

    def cosmo_vjp(self, ctx, grads, params=("Omega_m",), rel_eps=1e-5):
        """Chains the growth cotangents of `evolve_vjp` to cosmological parameters (fixed a_obs): besides sigma8 and the
        Eisenstein-Hu table (when no `lin_kpow` is given; central differences of the 256-point table, applied to the white
        field on the device) the cosmology enters evolve through host float64 scalars looked up in the 128-point growth tables -- the
        BullFrog coefficients and the 2LPT start (nbody.cosmo_vjp), a2g(a_obs) in the bias weights, a2g a2f in the
        RSD -- so dL/dtheta = sum_s s_bar ds/dtheta with the table Jacobian taken by central finite differences.
        With ap_auto=True <chi_bar, d chi / d theta> is added: the chi nodes of the Alcock-Paczynski look-up chi2a(cosmo, r'), by the
        same central difference of the host distance table as `_cosmo_vjp_lightcone` (the fiducial table does not move).
        `params`: attribute names of the cosmology object; 'Omega_m' varies Omega_c at fixed Omega_b.  On the light cone
        (a_obs = None) the look-ups are per particle: `_cosmo_vjp_lightcone`."""
        if self.a_obs is None:
            return self._cosmo_vjp_lightcone(ctx, grads, params, rel_eps)
        pre = getattr(ctx, "scalar_fd", None) or {}
        if self.evolution == 'kaiser':
            bars = [float(grads["kaiser"]["g"]), float(grads["kaiser"]["f"])]
        else:
            g = grads["growth"]
            bars = [float(np.asarray(grads["bias_growth"]).sum()), float(grads["gf"])]
            if self.evolution == 'nbody':
                bars += [float(g["dg"])] + list(g["alpha"]) + list(g["beta"])
            bars += [float(g["g"]), float(g["g2"]), float(g["dg2dg"])]
        chi_bar = grads["ap_chi_bar"].cpu().numpy() if grads.get("ap_chi_bar") is not None else None

        def terms(name, h, pair):
            # the table Jacobian's two evaluations, (scalars, chi nodes) each: made while the device ran the forward pass, or here
            vals = pre.get((name, rel_eps)) or [self._cosmo_scalars_chi(c) for c in pair]
            return [float(np.dot(b, (p - m) / (2 * h))) for b, p, m in zip((np.array(bars), chi_bar), *vals) if b is not None]

        out = self._cosmo_fd(ctx, grads, params, rel_eps, terms)
        ctx.cosmo._workspace = {}
        return out

    def _cosmo_fd(self, ctx, grads, params, rel_eps, terms):
        """{name: dL/dtheta} by one central difference per parameter (tables.fd_pair).  `terms(name, h, pair)` lists the contractions of the
        growth and distance tables; the transfer-table and Eisenstein-Hu terms are the same at fixed a_obs and on the light cone.  Summed in
        a fixed order: first table term, transfer, further table terms, Eisenstein-Hu."""
        out = {}
        for name in params:
            h, pair = tables.fd_pair(ctx.cosmo, name, rel_eps)
            first, *rest = terms(name, h, pair)
            out[name] = sum(rest, first + self._trans_term(grads, pair, h))
            if self.lin_kpow is None:      # the Eisenstein-Hu shape moves with the cosmology: init_mesh = white sqrt(P)
                inits = [self._power_mult(ctx.white, c) for c in pair]
                out[name] += float((grads["init_bar"].conj() * (inits[0] - inits[1])).real.sum().item()) / (2 * h)
        return out

    def _trans_term(self, grads, pair, h):
        """<trans_bar, d trans / d theta> for the phi -> delta transfer table (png_type set), the table Jacobian by the same host
        central difference (`pair`, `h` of `tables.fd_pair`) as the growth tables.  (sigma8 cancels in the table, so its derivative has no
        such term.)"""
        if grads.get("trans_bar") is None:
            return 0.0
        kpow = self.lin_kpow if self.evolution == 'kaiser' else None
        tr = [bricks.trans_phi2delta_table(c, kpow=kpow)[1] for c in pair]
        return float(np.dot(grads["trans_bar"], (tr[0] - tr[1]) / (2 * h)))

    def _cosmo_scalars(self, c):
        """The host float64 scalars through which a cosmology enters `evolve` at fixed a_obs (see cosmo_vjp)."""
        a = self.a_obs
        c._workspace = {}
        if self.evolution == 'kaiser':
            return np.array([float(nbody.a2g(c, a)), float(nbody.a2f(c, a))])
        out = [float(nbody.a2g(c, a)), float(nbody.a2g(c, a) * nbody.a2f(c, a))]
        if self.evolution == 'lpt':
            out += [float(nbody.a2g(c, a)), float(nbody.a2g2(c, a)), float(nbody.a2dg2dg(c, a))]
        else:
            dg, al, be, ls = nbody._step_scalars(c, self.nbody_a_start, a, self.nbody_n_steps, "bullfrog")
            out += [dg] + list(al) + list(be) + list(ls)
        return np.array(out)

    def _cosmo_scalars_chi(self, c):
        """(`_cosmo_scalars`, chi nodes ascending of the distance table or None): the second entry only with ap_auto=True, where the
        Alcock-Paczynski look-up chi2a(cosmo, r') is the one per-particle table dependence at fixed a_obs."""
        s = self._cosmo_scalars(c)
        return s, (tables.host_tables(c, tables.CHI2A)["chi"] if (self.ap_auto and self.evolution != 'kaiser') else None)

    def _cosmo_scalar_fd(self, cosmo, params, rel_eps=1e-5):
        """{(name, rel_eps): ((scalars, chi nodes) at +h, the same at -h)}: the two evaluations of cosmo_vjp's central difference.  Host work of about
        a millisecond (two growth-table solves per parameter) that `evolve` does right after it has queued the forward pass, while the
        device runs it; left to cosmo_vjp it sits at the very end of a gradient, with the device idle (`cosmo_fd_params`)."""
        # (the copies carry their own tables: `cosmo`'s cached ones stay for the rest of evolve)
        return {(name, rel_eps): tuple(self._cosmo_scalars_chi(c) for c in tables.fd_pair(cosmo, name, rel_eps)[1]) for name in params}

    # ---- light cone: the cosmology enters through per-particle table look-ups -----------------------------------------
    def lightcone_table_bars(self, ctx, grads):
        """Cotangents of those tables (dict of float64 arrays): the Lagrangian look-ups a_q = chi2a(r0_q) -> a2g (bias weights,
        model.py:756, and lpt), a2g2, a2dg2dg (lpt, nbody.py:652-666) contracted with the per-particle cotangents of
        `evolve_vjp` (mcpm_lightcone_tables_vjp_f32), plus the observation-side a2g a2f at the evolved positions
        (model.py:781-784; mcpm_observe_pos_tables_vjp_f32) and, with ap_auto=True, the chi2a(cosmo, r') of ap_auto in the same chi bar
        (mcpm_observe_pos_ap_tables_vjp_f32)."""
        dev = ctx.evol_k.device
        tab = tables.on_device(ctx.cosmo, tables.LIGHTCONE_VJP, dev)
        nchi, ng = tab.n["chi"], tab.n["a"]
        plan, g = nbody.get_plan(self.evol_shape, self.ptcl_shape), grads["growth"]
        if self.evolution == 'nbody':      # the per-particle look-up of the N-body light cone is a2g alone ('g_lc'); its g / g2 / dg2dg are host scalars
            gB = (nbody._f32(grads["bias_growth"]).reshape(-1) + nbody._f32(g["g_lc"]).reshape(-1)).contiguous()
            g2B, dB = torch.zeros_like(gB), torch.zeros_like(gB)
        else:
            gB = (nbody._f32(grads["bias_growth"]).reshape(-1) + nbody._f32(g["g"]).reshape(-1)).contiguous()
            g2B, dB = nbody._f32(g["g2"]).reshape(-1).contiguous(), nbody._f32(g["dg2dg"]).reshape(-1).contiguous()
        tbL = torch.empty(nchi + 4 * ng, dtype=torch.float64, device=dev)
        plan.call("mcpm_lightcone_tables_vjp_f32", self._r0, plan.N, tab.t, nchi, ng, gB, g2B, dB, tbL)
        # with ap_auto=True the Alcock-Paczynski look-up arrives in the chi bar of the observation side
        L, O = tab.bars(tbL), ctx.octx.lc.bars(bricks.observe_pos_tables_vjp(ctx.octx, grads["obs_bar"]))
        return {k: L[k] + O[k] if k in O else L[k] for k in L}

    def _cosmo_vjp_lightcone(self, ctx, grads, params, rel_eps):
        """cosmo_vjp on the light cone (a_obs = None, the reference's default configuration, model.py:45, :62): dL/dtheta =
        sum over the five tables (three for 'kaiser') of <table_bar, d table / d theta>, the table Jacobian by central differences of the host
        float64 RK4 tables (256-point distance table, 128-point growth tables), plus the Eisenstein-Hu term as at fixed a_obs.
        'nbody' adds the host scalars of the run, as at fixed a_obs: central differences of `_step_scalars(c, a_start, a_end(c), K)` contracted
        with alpha / beta / dg / g / g2 / dg2dg, the end of the run a_end(c) = chi2a(c, r_min) recomputed for each perturbed cosmology; its
        per-particle look-up is a2g(a_p) alone (cotangent bias_growth + g_lc, in `lightcone_table_bars`)."""
        # 'kaiser': the per-cell look-ups a = chi2a(r), a2g(a), a2f(a) of bricks.kaiser_sky, already contracted by evolve_vjp (chi, g, f)
        bars = grads["kaiser"] if self.evolution == 'kaiser' else self.lightcone_table_bars(ctx, grads)

        sbar = None
        if self.evolution == 'nbody':
            g = grads["growth"]
            sbar = np.array([float(g["dg"])] + list(g["alpha"]) + list(g["beta"]) + [float(g["g"]), float(g["g2"]), float(g["dg2dg"])])

        def run_scalars(c):
            c._workspace = {}
            dg, al, be, ls = nbody._step_scalars(c, self.nbody_a_start, self._a_end(c), self.nbody_n_steps, "bullfrog")
            return np.array([dg] + list(al) + list(be) + list(ls))

        def terms(name, h, pair):
            p, m = [tables.host_tables(c, tables.LIGHTCONE_VJP) for c in pair]
            out = [float(sum(np.dot(bars[k], (p[k] - m[k]) / (2 * h)) for k in tables.LIGHTCONE_VJP if k in bars))]
            if sbar is not None:
                out.append(float(np.dot(sbar, (run_scalars(pair[0]) - run_scalars(pair[1])) / (2 * h))))
            return out

        return self._cosmo_fd(ctx, grads, params, rel_eps, terms)
