"""Log density of the field-level model and its gradient, assembled around `FieldLevelForward` (the piece
`samplers.py` consumes as `logdensity_fn(position)`; montecosmo/model.py:362-363, :640-679, :840-908).

Built branch (everything else stays in the reference): latents with a Normal prior -- in sample space
`name_ ~ Normal((loc - loc_fid) / scale_fid, scale / scale_fid)` (model.py:1117-1119) with the affine
reparametrisation `base = name_ * scale_fid + loc_fid` (bricks.py:270-276); initial conditions `white_mesh_ ~ N(0, scale)`
per cell with the 'fourier' (rg2cgh) or 'real' (rfftn) preconditioning at unit scale, or the reference's default 'kaiser'
preconditioning (rg2cgh with the per-mode posterior width of the fiducial linear Kaiser model; model.py:1127-1148);
`evolve`; the 'quad_gauss' likelihood (model.py:852-870, :893-908), an optional selection mesh (paint_shape),
an optional mask over the final cells and radial shells with their own (fixed) mean densities:
    count = rc * irfftn(chreshape(rfftn(gxy_mesh * selec_mesh), final_shape)),   rc = ngbars[shell(r)] cell^3 per cell
    selec = |rc * irfftn(chreshape(rfftn(selec_mesh), final_shape))|  (or mean(ngbars) cell^3 without a selection mesh)
    delta = count / selec - 1;   phi = irfftn(chreshape(rfftn(phi of `evolve`), final_shape)) with png_type set, else 0
    scale1 = (|s_e + s_ed delta + s_ep phi| + 1e-9) sqrt(selec) sqrt(temp),   scale2 = s_e2 sqrt(selec)
    obs[mask] ~ QuadGaussian(count, scale1, scale2).
temp = `temp_lik` of `logdensity_and_grad`, the temperature of the tempered likelihood (model.py:840; 1 = the posterior itself).
Bounded latents (`low` / `high` in their config) use the reference's detruncated truncated-normal parametrisation
(utils.py:189-226, :267-311) within |x| < 12 sigma; latents without `loc` / `scale` have a uniform prior on [low, high] in the
same parametrisation (DetruncUnif, utils.py:314-353).

Other likelihoods (`lik_type`; value and gradient in one HIP kernel each, csrc/likelihood.hip, on the same count / selec):
    'shash'         obs[mask] ~ SinhArcsinh(count, sqrt(scale1^2 + 2 scale2^2), 3.540 scale2 / scale1, 1 + 5.884 (scale2 / scale1)^2) with the
                    scales of 'quad_gauss' (model.py:911-932; the default of the reference's drivers)
    'two_quad_gauss' obs[mask] ~ TwoQuadGaussian(count, scale1, scale2): obs = count + scale1 eps1 + scale2 (eps2^2 - 1) with independent
                    eps1, eps2, its density by the 64-node Gauss-Hermite rule of the reference (model.py:903-909, utils.py:541-616)
    'poisson'       obs[mask] ~ Poisson(|count|^(1 / temp)) (model.py:872-873)
    'fourier_gauss' cgh2rg(rfftn(obs)) ~ Normal(cgh2rg(rfftn(count)), cgh2rg_amp(|s_e + s_k2e k^2 + s_kmu2e (k mu)^2|) sqrt(selec) sqrt(temp)), full
                    sky and scalar selection only (model.py:875-886).
'quad_gauss' itself stays on its torch path.  Not built: the tempered prior `temp_prior` (`samp2base(temp=)`, model.py:640-679).

The gradient is hand-derived end to end: elementwise likelihood / prior terms here (device tensors), the mesh and
particle operators through their `*_vjp` twins -- no autodiff framework.

`logdensity_and_grad` runs three stages and one reverse tail:
    1. `_prior`: every latent -- scalars and the per-shell ngbars alike, and `base_params` -- through `latent_log_prob_and_grad`, which picks
       uniform / truncated normal / normal from the latent's config; a saturated tail ends the call here with -inf and a zero gradient.
    2. `_forward`: white field -> transfer -> `evolve` -> mean counts `cm` and selection on the final mesh; `mean_counts` is this stage alone.
    3. one likelihood method (`_lik_quad_gauss`, `_lik_hip`): (base, forward result, need_grad) -> (lp, cm_bar, stoch_bar, rcounts_bar or
       None); the forward result carries the temperature in (`temp`) and the cotangent of the final-mesh phi out (`phi_bar`).
       A new likelihood is one more such method.  Each keeps its own closed form of the shell gradient; `_per_shell` is the shared plumbing.
    tail: gxy_bar = cm_bar rc -> `_down_vjp` -> selection -> `evolve_vjp` (with phi_bar) -> white-field adjoint -> `_base_bar` chained to the latents.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import nbody, bricks, metrics, tables, _lib
from .utils import r2chshape, chreshape, chreshape_vjp, rg2cgh, rg2cgh_vjp, cgh2rg, mesh2masked, masked2mesh

LOG2PI = math.log(2 * math.pi)


def quad_gaussian_log_prob_and_grad(value, loc, b, a):
    """QuadGaussian.log_prob (utils.py:497-510) per element and its derivatives w.r.t. (loc, scale1 = b, scale2 = a).
    `a` is a python float (one value for the whole mesh) or a device tensor; as in the reference the Gaussian limit is
    selected PER ELEMENT where |a| < 1e-8 (utils.py:510), with a_safe = 1 there so that nothing non-finite is formed."""
    z = (value - loc) / b
    lp_g = -0.5 * LOG2PI - torch.log(b) - 0.5 * z * z
    if not torch.is_tensor(a) and abs(a) < 1e-8:
        return lp_g, z / b, (z * z - 1.0) / b, torch.zeros_like(lp_g)
    if torch.is_tensor(a):
        small = a.abs() < 1e-8
        a = torch.where(small, torch.ones_like(a), a)
    else:
        small = None
    r = value - loc + a
    D = b * b + 4.0 * a * r
    ok = D > 0
    Ds = torch.where(ok, D, torch.ones_like(D))
    sq = torch.sqrt(Ds)
    ep, em = (-b + sq) / (2.0 * a), (-b - sq) / (2.0 * a)
    lpp, lpm = -0.5 * ep * ep, -0.5 * em * em
    m = torch.maximum(lpp, lpm)
    sp, sm = torch.exp(lpp - m), torch.exp(lpm - m)
    lse = m + torch.log(sp + sm)
    wp, wm = sp / (sp + sm), sm / (sp + sm)
    lp = torch.where(ok, -0.5 * LOG2PI - 0.5 * torch.log(Ds) + lse, torch.full_like(D, -float("inf")))
    # d lp = -dD / (2 D) - wp ep d(ep) - wm em d(em);  dD = 2 b db + 4 a dr + 4 r da,  dr = -dloc + da,
    # d(sq) = dD / (2 sq);  d(ep) = (-db + d sq) / (2a) - ep da / a;  d(em) = (-db - d sq) / (2a) - em da / a
    t = (wp * ep - wm * em) / (2.0 * a)            # coefficient of d(sq) in -(wp ep d ep + wm em d em), sign included below
    s = (wp * ep + wm * em) / (2.0 * a)            # coefficient of db
    dD_dloc, dD_db, dD_da = -4.0 * a, 2.0 * b, 4.0 * a + 4.0 * r
    g_loc = -dD_dloc / (2 * Ds) - t * dD_dloc / (2 * sq)
    g_b = -dD_db / (2 * Ds) - t * dD_db / (2 * sq) + s
    g_a = -dD_da / (2 * Ds) - t * dD_da / (2 * sq) + (wp * ep * ep + wm * em * em) / a
    zero = torch.zeros_like(D)
    g_loc, g_b, g_a = torch.where(ok, g_loc, zero), torch.where(ok, g_b, zero), torch.where(ok, g_a, zero)
    if small is not None:
        lp, g_loc, g_b, g_a = (torch.where(small, lp_g, lp), torch.where(small, z / b, g_loc),
                               torch.where(small, (z * z - 1.0) / b, g_b), torch.where(small, zero, g_a))
    return lp, g_loc, g_b, g_a


_TAIL_TEMP = 1 / 6.2842226 / 2      # utils.py:190, :195: "best temperature at 12 sigma"
_TAIL_LIM = 12.0                     # utils.py:222


def std2trunc_and_derivs(x, loc, scale, low, high):
    """std2trunc (utils.py:189-226) with its first two derivatives, host float64.
    Body: y = Phi^-1(c_l + (c_h - c_l) Phi(x)) (and the mirrored form for x >= 0); dy/dx = phi(x) (c_h - c_l) / phi(y).
    Beyond 12 sigma, when the bound on that side is beyond 12 sigma too (utils.py:223), the reference switches to
    lowtail = T logsumexp([x, low] / T) (a soft maximum) and hightail = -T logsumexp(-[x, high] / T) (a soft minimum)."""
    from scipy.special import ndtr, ndtri
    lo, hi = (low - loc) / scale, (high - loc) / scale
    T = _TAIL_TEMP
    if x < -_TAIL_LIM and lo < -_TAIL_LIM:
        m = max(x, lo)
        ex, el = math.exp((x - m) / T), math.exp((lo - m) / T)
        y = m + T * math.log(ex + el)
        d1 = ex / (ex + el)
        return loc + scale * y, scale * d1, scale * d1 * (1.0 - d1) / T
    if x > _TAIL_LIM and hi > _TAIL_LIM:
        m = min(x, hi)
        ex, eh = math.exp(-(x - m) / T), math.exp(-(hi - m) / T)
        y = m - T * math.log(ex + eh)
        d1 = ex / (ex + eh)
        return loc + scale * y, scale * d1, -scale * d1 * (1.0 - d1) / T
    phi = lambda t: math.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)
    if x < 0:
        cl, ch = ndtr(lo), ndtr(hi)
        y = float(ndtri(cl + (ch - cl) * ndtr(x)))
        w = ch - cl
    else:
        cnl, cnh = ndtr(-lo), ndtr(-hi)
        y = -float(ndtri(cnh - (cnh - cnl) * ndtr(-x)))
        w = cnl - cnh
    d1 = phi(x) * w / phi(y)                    # dy/dx
    d2 = d1 * (-x + y * d1)                     # d2y/dx2 = d1 (dlog phi(x)/dx - dlog phi(y)/dy dy/dx)
    return loc + scale * y, scale * d1, scale * d2


def detrunc_truncnorm_log_prob_and_grad(x, c):
    """DetruncTruncNorm.log_prob (utils.py:296-311) and d/dx, plus the base value and d base / dx."""
    from scipy.special import ndtr
    y, d1, d2 = std2trunc_and_derivs(x, c["loc_fid"], c["scale_fid"], c["low"], c["high"])
    z = (y - c["loc"]) / c["scale"]
    logZ = math.log(ndtr((c["high"] - c["loc"]) / c["scale"]) - ndtr((c["low"] - c["loc"]) / c["scale"]))
    if not (math.isfinite(d1) and abs(d1) > 0.0 and math.isfinite(y)):
        # far in a tail the map has saturated in double precision (d std2trunc / dx underflows): the density there is zero for
        # every purpose -- jax would return -inf / nan and the sampler would reject; a math domain error would end the chain
        return -math.inf, 0.0, y, 0.0
    lp = -0.5 * LOG2PI - math.log(c["scale"]) - 0.5 * z * z - logZ + math.log(abs(d1))
    return lp, -z / c["scale"] * d1 + d2 / d1, y, d1


def detrunc_unif_log_prob_and_grad(x, c):
    """DetruncUnif.log_prob (utils.py:314-353): Uniform(low, high).log_prob(std2trunc(x; fid)) + log |d std2trunc / dx|, its
    d/dx, the base value and d base / dx."""
    y, d1, d2 = std2trunc_and_derivs(x, c["loc_fid"], c["scale_fid"], c["low"], c["high"])
    if not (math.isfinite(d1) and abs(d1) > 0.0 and math.isfinite(y)):
        return -math.inf, 0.0, y, 0.0          # saturated tail (see detrunc_truncnorm_log_prob_and_grad)
    return -math.log(c["high"] - c["low"]) + math.log(abs(d1)), d2 / d1, y, d1


def latent_log_prob_and_grad(x, c):
    """Prior of ONE latent at the sample value `x`, by its config `c`: (lp, d lp / dx, base, d base / dx).  No `loc` / `scale`: uniform on
    [low, high] (model.py:1122-1123); a finite `low` or `high`: truncated normal (model.py:1120-1121, bricks.py:271-273); else
    x ~ Normal((loc - loc_fid) / scale_fid, scale / scale_fid) with base = x scale_fid + loc_fid (model.py:1117-1119, bricks.py:270-276)."""
    if "loc" not in c:
        return detrunc_unif_log_prob_and_grad(x, c)
    if c["low"] != -math.inf or c["high"] != math.inf:
        return detrunc_truncnorm_log_prob_and_grad(x, c)
    mu, sd = (c["loc"] - c["loc_fid"]) / c["scale_fid"], c["scale"] / c["scale_fid"]
    return -0.5 * LOG2PI - math.log(sd) - 0.5 * ((x - mu) / sd) ** 2, -(x - mu) / sd ** 2, x * c["scale_fid"] + c["loc_fid"], c["scale_fid"]


def trunc2std(y, loc, scale, low, high):
    """Inverse of `std2trunc_and_derivs` (utils.py:229-264: invbody, invlowtail, invhightail), host float64.  As in the reference the branch
    is chosen from the standardised y: beyond 12 sigma, with the bound on that side beyond 12 sigma too, the inverse of the soft maximum /
    minimum, x = T log(e^(y/T) - e^(low/T)) and x = -T log(e^(-y/T) - e^(-high/T)); else the body, Phi^-1 of the rescaled cdf."""
    from scipy.special import ndtr, ndtri
    y, lo, hi = (y - loc) / scale, (low - loc) / scale, (high - loc) / scale
    T = _TAIL_TEMP
    if y < -_TAIL_LIM and lo < -_TAIL_LIM:
        return y + T * math.log1p(-math.exp((lo - y) / T)) if y > lo else -math.inf
    if y > _TAIL_LIM and hi > _TAIL_LIM:
        return y - T * math.log1p(-math.exp((y - hi) / T)) if y < hi else math.inf
    if y < 0:
        cl, ch = ndtr(lo), ndtr(hi)
        return float(ndtri((ndtr(y) - cl) / (ch - cl)))
    cnl, cnh = ndtr(-lo), ndtr(-hi)
    return -float(ndtri((cnh - ndtr(-y)) / (cnh - cnl)))


def latent_sample_value(y, c):
    """Sample value of ONE latent at the base value `y`, by its config `c`: the inverse of the third output of `latent_log_prob_and_grad`
    (bricks.py:277-283).  Uniform and truncated latents: trunc2std with the fiducial parameters; else (y - loc_fid) / scale_fid."""
    if "loc" not in c or c["low"] != -math.inf or c["high"] != math.inf:
        return trunc2std(float(y), c["loc_fid"], c["scale_fid"], c["low"], c["high"])
    return (float(y) - c["loc_fid"]) / c["scale_fid"]


def _elementwise(fn, v, c):
    """fn(v, c) for a number, or element by element for an array (a leading chain axis)."""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 0:
        return fn(float(v), c)
    return np.array([fn(float(x), c) for x in v.reshape(-1)]).reshape(v.shape)


class FieldLevelLogDensity:
    """log p(sample params, observed counts) and its gradient.

    fwd      : FieldLevelForward (shapes, box, evolution, a_obs ...)
    count_obs: observed count mesh, real, fwd.final_shape
    latents  : name -> dict(loc, scale, loc_fid, scale_fid) for every SAMPLED scalar base parameter (unbounded Normal)
    fixed    : name -> value for the base parameters that are not sampled; between them `latents` and `fixed` must
               provide Omega_m, sigma8, the eight bias parameters, ngbars, s_e, s_ed, s_e2.  The six PNG parameters
               (bricks.PNG_KEYS: fNL, fNL_bp, fNL_bpd, fNL_bpd2, fNL_bps2, fNL_bn2p) may appear in either; a missing one is
               fixed at 0.  They reach the model only when `fwd.png_type` is set.  The Alcock-Paczynski parameters alpha_iso, alpha_ap
               (bricks.AP_KEYS; the reference's prior: truncated normal, loc 1, scale 0.1, low 0, model.py:189-204) may appear in
               either as well; a missing one is fixed at 1.  They are read only when `fwd.ap_auto is False`.  s_ep, the coefficient of the
               primordial stochastic term s_ep * phi of scale1 (model.py:894), may appear in either; a missing one is fixed at 0, and a
               sampled one takes the reference's prior for the entries its config leaves out (S_EP_LATENT; model.py:248-253).  It is read
               by 'quad_gauss', 'shash' and 'two_quad_gauss' when `fwd.png_type` is set (else phi = 0); the Kaiser model defines no phi.
    make_cosmo(base) -> cosmology object (default: Planck18 with Omega_c = Omega_m - Omega_b and sigma8)
    """

    COSMO = ("Omega_m", "sigma8")
    STOCH = ("s_e", "s_ed", "s_e2")
    # stochastic parameters each likelihood reads; one it does not read need not be supplied, and gets a zero likelihood gradient if sampled
    LIK_STOCH = {"quad_gauss": STOCH, "shash": STOCH, "two_quad_gauss": STOCH, "fourier_gauss": ("s_e", "s_k2e", "s_kmu2e"), "poisson": ()}
    ALL_STOCH = ("s_e", "s_ed", "s_e2", "s_ep", "s_k2e", "s_kmu2e")
    PHI_LIKS = ("quad_gauss", "shash", "two_quad_gauss")      # the families whose scale1 has the term s_ep * phi
    S_EP_LATENT = dict(loc=0., scale=1e5, loc_fid=0., scale_fid=1e2)      # model.py:248-253
    N_QUAD = 64      # nodes of the Gauss-Hermite rule of 'two_quad_gauss' (utils.py:582)

    def __init__(self, fwd, count_obs, latents, fixed, precond="fourier", make_cosmo=None, selec_mesh=None, mask_mesh=None,
                 redges=None, n_rbins=None, lik_type="quad_gauss"):
        """selec_mesh: real, fwd.paint_shape (None = 1); mask_mesh: bool, final_shape, True = observed cell (None = all);
        ngbars: fixed (a scalar or one mean density per radial shell) or a latent whose config entries are broadcast to the
        n_rbins shells (model.py:1087-1103; sample key 'ngbars_' is then an array); redges: shell edges (default: equal-width
        shells over the observed cells); n_rbins: number of shells of a sampled ngbars (default: the reference's
        max(int((rmax - rmin) / (sqrt(3) cell)), 1)).  count_obs is the full final mesh (only observed cells are used)."""
        if precond not in ("fourier", "real", "kaiser"):
            raise ValueError(f"Unknown preconditioning type: {precond}")
        if lik_type not in self.LIK_STOCH:
            raise ValueError(f"Unknown likelihood type: {lik_type} (built: {sorted(self.LIK_STOCH)})")
        if lik_type == "fourier_gauss" and mask_mesh is not None:
            raise ValueError("Fourier likelihood not implemented for cut-sky.")      # model.py:876
        if lik_type == "fourier_gauss" and selec_mesh is not None:
            raise ValueError("Fourier likelihood takes a scalar selection: the per-mode scale does not broadcast with a selection mesh")
        self.fwd, self.precond, self.lik_type = fwd, precond, lik_type
        latents = dict(latents)
        if "s_ep" in latents:
            latents["s_ep"] = dict(self.S_EP_LATENT, **{k: v for k, v in latents["s_ep"].items() if v is not None})
        # s_ep is read (and has a likelihood gradient) only where there is a phi: a real-space family on a model with png_type
        self.reads_phi = lik_type in self.PHI_LIKS and fwd.png_type is not None
        if lik_type in self.PHI_LIKS and ("s_ep" in latents or float(fixed.get("s_ep", 0.)) != 0.) and fwd.evolution == "kaiser":
            raise ValueError("s_ep needs the phi of an 'lpt' or 'nbody' evolution: the Kaiser model defines none (model.py:690-696, :837)")
        self._ngb_conf = latents.pop("ngbars", None)
        self._n_rbins = n_rbins
        self.latents = {k: dict({"low": -math.inf, "high": math.inf}, **{kk: float(vv) for kk, vv in v.items() if vv is not None})
                        for k, v in latents.items()}
        for k, c in self.latents.items():      # no loc / scale: a uniform prior on [low, high] (model.py:1122-1123)
            if "loc" not in c or "scale" not in c:
                if not (math.isfinite(c["low"]) and math.isfinite(c["high"])):
                    raise ValueError(f"latent '{k}' not valid: low and high must be finite for uniform distribution")
                c.pop("loc", None), c.pop("scale", None)
                c.setdefault("loc_fid", (c["low"] + c["high"]) / 2)              # model.py:1081-1084
                c.setdefault("scale_fid", (c["high"] - c["low"]) / 12 ** .5)
        self.fixed = dict(fixed)
        need = set(self.COSMO) | set(bricks.BIAS_KEYS) | {"ngbars"} | set(self.LIK_STOCH[lik_type])
        missing = need - set(self.latents) - set(self.fixed) - ({"ngbars"} if self._ngb_conf is not None else set())
        if missing:
            raise ValueError(f"parameters neither sampled nor fixed: {sorted(missing)}")
        self.final_shape = tuple(fwd.final_shape)
        self.count_obs = nbody._f32(count_obs, self.final_shape)
        self.make_cosmo = make_cosmo or self._planck
        self._setup_selection(selec_mesh, mask_mesh, redges)
        self.scale, self.transfer = self._precond_scale_and_transfer()
        if lik_type == "fourier_gauss":      # the observation in the real layout, once (model.py:885 applied to the data)
            self.los_fid = fwd.los_cell()
            self.obs_rg = cgh2rg(nbody.rfftn(self.count_obs))
        if lik_type == "two_quad_gauss":      # nodes and log weights of E_{N(0,1)}[f] ~ sum wn_i f(z_i), host float64 (utils.py:589-591)
            z, w = np.polynomial.hermite_e.hermegauss(self.N_QUAD)
            self.quad = torch.from_numpy(np.stack([z, np.log(w) - 0.5 * LOG2PI])).to(self.count_obs.device)

    @staticmethod
    def _planck(base):
        c = bricks.Planck18()
        c.Omega_c = float(base["Omega_m"]) - c.Omega_b
        c.sigma8 = float(base["sigma8"])
        return c

    def _down(self, mesh):
        """irfftn(chreshape(rfftn(mesh), final_shape)) (model.py:855, :861); identity when the shapes agree."""
        if tuple(mesh.shape) == self.final_shape:
            return mesh
        return nbody.irfftn(chreshape(nbody.rfftn(mesh), r2chshape(self.final_shape)))

    def _down_vjp(self, mesh_bar, shape):
        """Adjoint of `_down` for a mesh of `shape`: the adjoints of irfftn, chreshape and rfftn (real-pair convention)."""
        if tuple(shape) == self.final_shape:
            return mesh_bar
        return nbody.rfftn_vjp(chreshape_vjp(nbody.irfftn_vjp(mesh_bar), r2chshape(tuple(shape))), overwrite=True)

    def _setup_selection(self, selec_mesh, mask_mesh, redges):
        """Radial shells as a per-cell index (set_radial_count, bricks.py:1106-1122: cell -> its shell's count), the
        down-sampled selection and the 0/1 mask as device tensors computed once; a sampled ngbars gets its per-shell
        prior configuration (model.py:1099-1103)."""
        fwd, dev = self.fwd, self.count_obs.device
        mask = None if mask_mesh is None else np.asarray(mask_mesh, dtype=bool).reshape(self.final_shape)
        rmesh = fwd.lattice_radius(self.final_shape).reshape(self.final_shape)      # distance of the final-mesh cells; set-up only
        if self._ngb_conf is None:
            nb = len(np.atleast_1d(self.fixed["ngbars"]))
        elif redges is not None:
            nb = len(redges) - 1
        elif self._n_rbins is not None:
            nb = int(self._n_rbins)
        else:
            r = rmesh if mask is None else rmesh[mask]
            nb = max(int((r.max() - r.min()) / (3 ** .5 * fwd.cell_length)), 1)            # model.py:1095
        if redges is None:
            r = rmesh if mask is None else rmesh[mask]
            dr = 3 ** .5 * fwd.cell_length
            redges = np.linspace(r.min() - dr / 1000, r.max() + dr / 1000, nb + 1)
        redges = np.asarray(redges, dtype=np.float64)
        if len(redges) != nb + 1:
            raise ValueError("redges must have one more entry than ngbars")
        shell = np.full(self.final_shape, nb, dtype=np.int64)          # nb: in no shell (count multiplier 1)
        for i, (lo, hi) in enumerate(zip(redges[:-1], redges[1:])):
            shell[(lo < rmesh) & (rmesh <= hi)] = i
        self.n_rbins, self.shell = nb, torch.from_numpy(shell).to(dev)
        if self._ngb_conf is not None:
            c = {k: v for k, v in self._ngb_conf.items() if v is not None and k in ("loc", "scale", "loc_fid", "scale_fid", "low", "high")}
            c.setdefault("low", -math.inf), c.setdefault("high", math.inf)
            self.ngb_lat = {k: np.broadcast_to(np.asarray(v, dtype=np.float64), (nb,)).copy() for k, v in c.items()}
            self.ngbar_mean = float(self.ngb_lat["loc_fid"].mean())
        else:
            self.ngb_lat = None
            self.ngbar_mean = float(np.mean(self.fixed["ngbars"]))
        self.mask = None if mask is None else torch.from_numpy(np.asarray(mask).astype(bool)).to(dev)
        if selec_mesh is None:
            self.selec_mesh, self.sel_down, self.selec_fid = None, None, 1.0
        else:
            sm = np.asarray(selec_mesh, dtype=np.float64)
            self.selec_fid = float((sm ** 2).mean() ** .5 / sm.mean())                 # model.py:609
            self.selec_mesh = nbody._f32(selec_mesh, fwd.paint_shape)
            self.sel_down = self._down(self.selec_mesh)

    def _ngb_elem(self, i):
        return {k: float(v[i]) for k, v in self.ngb_lat.items()}

    # ---- real-space diagnostics of meshes against a truth (model.py:1259-1263, :1381-1405) ------------------------------
    def mesh2masked(self, mesh):
        """The observed cells of a final mesh (or a batch of them) as a vector; the mesh itself without a mask."""
        return mesh2masked(mesh, self.mask)

    def masked2mesh(self, masked):
        """Inverse of mesh2masked, zeros in the unobserved cells."""
        return masked2mesh(masked, self.mask)

    @property
    def rmasked(self):
        """Distances of the observed cells (of every cell without a mask): float64 on the device, built on first use and kept."""
        if getattr(self, "_rmasked", None) is None:
            self._rmesh = torch.from_numpy(self.fwd.radius_mesh(self.final_shape)).to(self.count_obs.device)
            self._rmasked = self._rmesh.reshape(-1) if self.mask is None else self._rmesh[self.mask]
        return self._rmasked

    def _radial(self, fn, meshes, cell_length, redges, aggr_fn, from_masked):
        """fn = metrics.mse_radius or metrics.distr_radial on the model's radii; the last of `meshes` may carry a batch axis.  On a cut sky the
        edges come from the observed radii, and both routes run the same pass over full meshes with the mask (so they agree to the bit):
        full meshes as they are, masked vectors scattered into zero-filled meshes first, a bounded number of batch rows at a time."""
        cell_length = self.fwd.cell_length if cell_length is None else cell_length
        rmasked = self.rmasked
        if self.mask is None:      # meshes or flat vectors of every cell
            as_mesh = tuple(np.shape(meshes[-1])[-3:]) == self.final_shape
            return fn(*meshes, self._rmesh if as_mesh else rmasked, cell_length, redges=redges, aggr_fn=aggr_fn)
        if aggr_fn is not None:      # the host path takes the masked vectors
            if not from_masked:
                meshes = [self.mesh2masked(torch.as_tensor(m)) for m in meshes]
            return fn(*meshes, rmasked, cell_length, redges=redges, aggr_fn=aggr_fn)
        edges = metrics._vedges(rmasked, redges, 1, cell_length)[0]
        if not from_masked:
            return fn(*meshes, self._rmesh, cell_length, redges=edges, mask=self.mask)
        meshes = [torch.as_tensor(m) for m in meshes]
        for m in meshes:
            if m.ndim not in (1, 2) or m.shape[-1] != rmasked.numel():
                raise ValueError(f"from_masked=True takes vectors of the {rmasked.numel()} observed cells (one optional batch axis), got shape {tuple(m.shape)}")
        if getattr(self, "_mask_index", None) is None:      # masked2mesh with the mask's cell numbers found once, not per call
            self._mask_index = self.mask.reshape(-1).nonzero().squeeze(1)

        def full(m):
            out = torch.zeros(tuple(m.shape[:-1]) + (self._rmesh.numel(),), dtype=torch.float32, device=self.mask.device)
            out.index_copy_(-1, self._mask_index, m.to(device=self.mask.device, dtype=torch.float32))
            return out.reshape(tuple(m.shape[:-1]) + self.final_shape)
        lead, last = [full(m) for m in meshes[:-1]], meshes[-1]
        if last.ndim == 1:
            return fn(*lead, full(last), self._rmesh, cell_length, redges=edges, mask=self.mask)
        chunk = int(max(1, metrics.CHUNK_BYTES // (8 * self._rmesh.numel())))
        outs = []
        for lo in range(0, last.shape[0], chunk):
            count, mean, aggr = fn(*lead, full(last[lo:lo + chunk]), self._rmesh, cell_length, redges=edges, mask=self.mask)
            outs.append(aggr)      # count and mean are the same bits from every chunk
        return count, mean, np.concatenate(outs)

    def mse_radius(self, mesh0, mesh1, cell_length=None, redges: int | float | list = None, aggr_fn=None, from_masked=True):
        """Mean squared error between mesh0 and mesh1 (which may be batched) over the observed cells, binned by distance: (rcount, rmean,
        mse).  from_masked: the inputs are vectors of the observed cells (mesh2masked); else full final meshes, binned in place."""
        return self._radial(metrics.mse_radius, (mesh0, mesh1), cell_length, redges, aggr_fn, from_masked)

    def distr_radial(self, mesh, cell_length=None, redges: int | float | list = None, aggr_fn=None, from_masked=True):
        """Radial distribution of a mesh (which may be batched) over the observed cells: (rcount, rmean, mean per shell / cell_length^3)."""
        return self._radial(metrics.distr_radial, (mesh,), cell_length, redges, aggr_fn, from_masked)

    def mse_value(self, mesh0, mesh1, cell_length=None, vedges: int | float | list = 50, min_count=None, aggr_fn=None):
        return self.fwd.mse_value(mesh0, mesh1, cell_length=cell_length, vedges=vedges, min_count=min_count, aggr_fn=aggr_fn)

    def mse_wave(self, mesh0, mesh1, kedges: int | float | list = None, include_corners=True):
        return self.fwd.mse_wave(mesh0, mesh1, kedges=kedges, include_corners=include_corners)

    def fiducial(self):
        """Fiducial base values: loc_fid of the latents, else the fixed value (model.py:1214-1223)."""
        fid = dict(self.fixed)
        fid.update({k: c["loc_fid"] for k, c in self.latents.items()})
        if self.ngb_lat is not None:
            fid["ngbars"] = self.ngb_lat["loc_fid"].copy()
        return fid

    def _fiducial_scale_factor(self, cosmo_fid):
        """a_fid = g2a(mean a2g(a)) over the final-mesh cells (model.py:604-606)."""
        fwd = self.fwd
        a = fwd.a_obs if fwd.a_obs is not None else nbody.chi2a(cosmo_fid, fwd.lattice_radius(self.final_shape))
        return float(nbody.g2a(cosmo_fid, np.mean(nbody.a2g(cosmo_fid, a))))

    def _kaiser_fiducial(self):
        """What the fiducial linear Kaiser model is made of, for the 'kaiser' preconditioning and for `kaiser_post` alike (model.py:602-609,
        :1140, :1457-1458): fid, cosmo, a = a_fid, los (cell axes), b1E = 1 + b1 and var_noise = s_e / (mean count per cell * selec_fid)."""
        fwd, fid = self.fwd, self.fiducial()
        cosmo_fid = self.make_cosmo(fid)
        a_fid = self._fiducial_scale_factor(cosmo_fid)
        var_fid = float(fid.get("s_e", 1.0)) / (self.ngbar_mean * fwd.cell_length ** 3 * self.selec_fid)   # model.py:602, :609, :1140 ('poisson' reads no s_e: 1)
        return SimpleNamespace(fid=fid, cosmo=cosmo_fid, a=a_fid, los=fwd.los_cell(), b1E=1.0 + float(fid["b1"]), var_noise=var_fid)

    def _precond_scale_and_transfer(self):
        """(scale, transfer) of the white-field preconditioning (model.py:1127-1148): `scale` is the prior std of
        white_mesh_ (None = 1), `transfer` the factor taking rg2cgh / rfftn of it to unit-power white noise (a float, or
        a per-mode device tensor).  'kaiser' (bricks.py:170-184, :96-106; uniform selection, selec_fid = 1): a one-off
        host float64 set-up of two init_shape-sized meshes."""
        fwd = self.fwd
        unit = float(np.divide(fwd.init_shape, fwd.box_size).prod() ** .5)
        if self.precond in ("real", "fourier"):
            return None, unit
        k = self._kaiser_fiducial()
        fid, cosmo_fid, a_fid, var_fid = k.fid, k.cosmo, k.a, k.var_noise
        kvec = nbody.rfftk(fwd.init_shape, fwd.box_size)
        kmesh = sum(ki ** 2 for ki in kvec) ** .5
        mu = nbody.safe_div(sum(ki * li for ki, li in zip(kvec, k.los)), kmesh)
        boost = float(nbody.a2g(cosmo_fid, a_fid)) * (k.b1E + float(nbody.a2f(cosmo_fid, a_fid)) * mu ** 2)
        ks, pows = tables.host_tables(cosmo_fid, tables.POWER, kpow=fwd.lin_kpow).values()
        pmesh = np.interp(kmesh.reshape(-1), ks, pows * float(fid["sigma8"]) ** 2, left=0., right=0.).reshape(kmesh.shape)
        pmesh *= unit ** 2                                                                # power in cell units
        scale_k = (1 + boost ** 2 / var_fid * pmesh) ** .5
        cosmo_fid._workspace = {}
        dev = self.count_obs.device
        transfer = torch.from_numpy((unit / scale_k).astype(np.float32)).to(dev)
        scale = cgh2rg(torch.from_numpy(scale_k.astype(np.complex64)).to(dev), norm="amp")
        return scale, transfer

    # ---- stage 1: priors of the latents --------------------------------------------------------------------------------------------
    def _prior(self, sample):
        """(lp, base, grad, dbase) of the scalar latents and the per-shell ngbars (same priors, model.py:1105-1125): the summed prior, the
        base parameters (fixed ones included), grad[name_] = d lp / d name_ and dbase[name] = d base / d name_ (arrays for ngbars)."""
        lp, base, grad, dbase = 0.0, dict(self.fixed), {}, {}
        for name, c in self.latents.items():
            l, grad[name + "_"], base[name], dbase[name] = latent_log_prob_and_grad(float(sample[name + "_"]), c)
            lp += l
        if self.ngb_lat is not None:
            xs = np.atleast_1d(np.asarray(sample["ngbars_"], dtype=np.float64))
            terms = np.array([latent_log_prob_and_grad(float(xs[i]), self._ngb_elem(i)) for i in range(self.n_rbins)])
            for l in terms[:, 0]:
                lp += float(l)
            grad["ngbars_"], base["ngbars"], dbase["ngbars"] = terms[:, 1].copy(), terms[:, 2].copy(), terms[:, 3].copy()
        return lp, base, grad, dbase

    def base_params(self, sample):
        return self._prior(sample)[1]

    def sample_params(self, base):
        """Inverse of `base_params` (bricks.py:255-287, :310-318 with inv=True): base values -> sample values, for every sampled latent found
        in `base` (fixed keys are ignored).  Scalars by their kind (`latent_sample_value`), a per-shell ngbars element by element,
        'white_mesh' (half-spectrum at init_shape) -> 'white_mesh_' = cgh2rg(white / transfer) ('fourier', 'kaiser') or irfftn(white / transfer)
        ('real').  Every value may carry a leading chain axis."""
        out = {}
        for name, c in self.latents.items():
            if name in base:
                out[name + "_"] = _elementwise(latent_sample_value, base[name], c)
        if self.ngb_lat is not None and "ngbars" in base:
            v = np.asarray(base["ngbars"], dtype=np.float64)
            v = np.broadcast_to(v, v.shape[:-1] + (self.n_rbins,)) if v.ndim else np.full(self.n_rbins, float(v))
            x = np.empty(v.shape)
            for i in range(self.n_rbins):
                x[..., i] = _elementwise(latent_sample_value, v[..., i], self._ngb_elem(i))
            out["ngbars_"] = x
        if "white_mesh" in base:
            w = nbody._c64(base["white_mesh"])
            if tuple(w.shape[-3:]) != r2chshape(self.fwd.init_shape) or w.ndim not in (3, 4):
                raise ValueError(f"white_mesh must be a half-spectrum at init_shape {r2chshape(self.fwd.init_shape)}, got {tuple(w.shape)}")
            tr = self.transfer
            if torch.is_tensor(tr):
                w = torch.where(tr != 0, w / torch.where(tr != 0, tr, torch.ones_like(tr)), torch.zeros_like(w))      # safe_div
            else:
                w = w / tr
            inv = nbody.irfftn if self.precond == "real" else cgh2rg
            out["white_mesh_"] = inv(w) if w.ndim == 3 else torch.stack([inv(w[b].contiguous()) for b in range(w.shape[0])])
        return out

    def count2delta(self):
        """The observed contrast on the final mesh under the global integral constraint (model.py:1271-1285): unobserved cells of the counts
        set to 0; the selection brought to final_shape and zeroed outside the mask when its shape differs from the final mesh, used as given
        when the shapes agree, and a scalar without a selection mesh."""
        obs = self.count_obs if self.mask is None else torch.where(self.mask, self.count_obs, torch.zeros_like(self.count_obs))
        if self.selec_mesh is None:
            return bricks.count2delta(obs, 1.0)
        selec = self.selec_mesh
        if tuple(selec.shape) != self.final_shape:
            selec = self.sel_down if self.mask is None else torch.where(self.mask, self.sel_down, torch.zeros_like(self.sel_down))
        return bricks.count2delta(obs, selec)

    def kaiser_post(self, seed, base=False, temp=1., scale_field=1., n_chains=None, noise=None):
        """Start values for every sampled latent (model.py:1444-1477): the scalars at their fiducial values and the initial field drawn from
        its posterior under the fiducial flat-sky Kaiser model given the observed counts,
            white_mesh = scale_field * lin2white(sqrt(temp) stds rg2cgh(noise) + means),   (means, stds) = bricks.kaiser_posterior(delta_obs, ...)
        with delta_obs = chreshape(rfftn(count2delta()), init_shape), b1E = 1 + b1_fid, var_noise = s_e_fid / (mean count per cell * selec_fid)
        and a_fid, the cell line of sight and the fiducial cosmology of the 'kaiser' preconditioning -- whatever `evolution` is.  `noise`: unit
        normal real mesh(es), init_shape or (n_chains, *init_shape); default: drawn on the device from `seed`.  base=True: base space
        ('white_mesh', a half-spectrum); else through `sample_params` ('white_mesh_').  With `n_chains` every value has a leading chain axis.
        HIP: one call of mcpm_kaiser_post_c64 for all chains (no reduction: the same seed gives the same bits)."""
        fwd = self.fwd
        dev, shape = self.count_obs.device, tuple(fwd.init_shape)
        nc = 1 if n_chains is None else int(n_chains)
        if nc < 1:
            raise ValueError("n_chains must be at least 1")
        if noise is None:
            gen = torch.Generator(device=dev).manual_seed(int(seed))
            noise = torch.randn((nc,) + shape, dtype=torch.float32, device=dev, generator=gen)
        else:
            noise = nbody._f32(noise)
            if tuple(noise.shape) == shape:
                noise = noise.expand((nc,) + shape)
            if tuple(noise.shape) != (nc,) + shape:
                raise ValueError(f"noise must have shape {shape} or {(nc,) + shape}, got {tuple(noise.shape)}")
        noise_k = torch.stack([rg2cgh(noise[b].contiguous()) for b in range(nc)])
        k = self._kaiser_fiducial()
        delta_obs = chreshape(nbody.rfftn(self.count2delta()), r2chshape(shape))
        white, _, _ = bricks.kaiser_post_white(delta_obs, noise_k, k.cosmo, k.a, fwd.box_size, k.var_noise, k.b1E, los=k.los, kpow=fwd.lin_kpow,
                                               temp=temp, scale_field=scale_field)
        k.cosmo._workspace = {}
        start = {name: (k.fid[name] if n_chains is None else np.full(nc, k.fid[name])) for name in self.latents}
        if self.ngb_lat is not None:
            start["ngbars"] = k.fid["ngbars"] if n_chains is None else np.tile(k.fid["ngbars"], (nc, 1))
        start["white_mesh"] = white[0] if n_chains is None else white
        return start if base else self.sample_params(start)

    def condition(self, values):
        """A new log density in which the latents named in `values` are fixed at those BASE values (moved from `latents` to `fixed`); the
        observation, selection, mask, shells, preconditioning and likelihood are shared with this one.  Conditioning on every scalar leaves
        the field alone: the target of the reference's field-only warm-up (script.py:46-49).  The scalar priors of the conditioned latents
        drop out of the value (constants)."""
        import copy
        unknown = set(values) - set(self.latents) - ({"ngbars"} if self.ngb_lat is not None else set())
        if unknown:
            raise ValueError(f"cannot condition on {sorted(unknown)}: not sampled latents of this log density")
        new = copy.copy(self)
        new.latents = {name: c for name, c in self.latents.items() if name not in values}
        new.fixed = dict(self.fixed)
        for name, v in values.items():
            if name == "ngbars":
                v = np.asarray(v, dtype=np.float64)
                new.fixed[name] = np.broadcast_to(v, (self.n_rbins,)).copy()
                new.ngb_lat = new._ngb_conf = None
            else:
                new.fixed[name] = float(v)
        return new

    def _white_prior(self, w):
        """white_mesh_ ~ Normal(0, scale) per cell (model.py:666-672; scale None = 1)."""
        if self.scale is None:
            return float(-0.5 * LOG2PI * w.numel() - 0.5 * (w.double() ** 2).sum())
        return float(-0.5 * LOG2PI * w.numel() - self.scale.double().log().sum() - 0.5 * ((w / self.scale).double() ** 2).sum())

    # ---- stage 2: forward model up to the mean counts --------------------------------------------------------------------------------
    def _forward(self, base, white_mesh_, need_ctx=False, need_phi=False):
        """What every likelihood is evaluated on (model.py:850-870): gxy (the galaxy mesh of `evolve`; ctx: its context when `need_ctx`),
        rc (per-cell count multiplier from the shells' mean densities), dn (gxy times the selection mesh, brought to the final mesh),
        cm = dn rc (the mean counts), selec (a mesh with a selection mesh, else the float mean(rcounts)) and, with `need_phi`, phi on the
        final mesh where the likelihood reads it (a real-space family, png_type set, s_ep sampled or fixed away from 0), else None."""
        fwd = self.fwd
        w = nbody._f32(white_mesh_, fwd.init_shape)
        white = (nbody.rfftn(w) if self.precond == "real" else rg2cgh(w)) * self.transfer
        kw = {"png": {k: float(base.get(k, 0.0)) for k in bricks.PNG_KEYS}} if fwd.png_type is not None else {}
        if fwd.ap_auto is False:
            kw["ap"] = {k: float(base.get(k, 1.0)) for k in bricks.AP_KEYS}
        if need_ctx:
            # Omega_m sampled: the forward model makes the two evaluations of the growth-table Jacobian as soon as it has queued its kernels
            fwd.cosmo_fd_params = ("Omega_m",) if "Omega_m" in self.latents else None
        need_phi = need_phi and self.reads_phi and ("s_ep" in self.latents or float(base.get("s_ep", 0.)) != 0.)
        out = fwd.evolve(self.make_cosmo(base), {k: base[k] for k in bricks.BIAS_KEYS}, white, return_ctx=need_ctx or need_phi, **kw)
        gxy, ctx = out if (need_ctx or need_phi) else (out, None)
        rcounts = np.atleast_1d(np.asarray(base["ngbars"], dtype=np.float64)) * fwd.cell_length ** 3
        rc = torch.from_numpy(np.append(rcounts, 1.0).astype(np.float32)).to(gxy.device)[self.shell]
        selec = float(rcounts.mean()) if self.sel_down is None else (self.sel_down * rc).abs()
        dn = self._down(gxy if self.selec_mesh is None else gxy * self.selec_mesh)
        phi = fwd.phi_final(ctx.phi).contiguous() if need_phi else None      # model.py:868-869
        return SimpleNamespace(gxy=gxy, ctx=ctx, rc=rc, dn=dn, cm=dn * rc, selec=selec, phi=phi, phi_bar=None, temp=1.)

    def mean_counts(self, sample):
        """(count, selec) of the likelihood at `sample` (model.py:850-866): the mean counts on the final mesh, and the selection there (a mesh
        with a selection mesh, else the float mean(rcounts))."""
        f = self._forward(self.base_params(sample), sample["white_mesh_"])
        return f.cm, f.selec

    # ---- stage 3: likelihoods.  Each: (base, f = _forward's result with f.temp = temp_lik, need_grad) -> (lp, cm_bar = d lp / d cm at fixed selec, the
    # cotangents of the stochastic parameters, rcounts_bar = d lp / d rcounts per shell through count AND selec, or None with fixed ngbars),
    # and f.phi_bar = d lp / d f.phi where there is a phi; with need_grad = False only lp is formed and the rest is None -----------------
    def _per_shell(self, cell_bar):
        """A per-cell cotangent summed over each radial shell (float64 device tensor; the cells in no shell are dropped)."""
        return torch.bincount(self.shell.reshape(-1), weights=cell_bar.double().reshape(-1), minlength=self.n_rbins + 1)[:self.n_rbins]

    def _lik_hip(self, base, f, need_grad):
        """'shash', 'two_quad_gauss', 'poisson' or 'fourier_gauss': value, mesh cotangents and float64 sums from one kernel
        (csrc/likelihood.hip).  The kernel gives count_bar at fixed selec and sqsel_bar = d lp / d sqrt(selec) at fixed count (per cell for the
        real-space families, its sum in sums[4]); the shells get both.  The temperature is applied inside the kernels."""
        plan = nbody.get_plan(self.final_shape)
        cm, selec, want_sqsel = f.cm.contiguous(), f.selec, self.ngb_lat is not None
        sums = torch.empty(6, dtype=torch.float64, device=cm.device)
        mesh_sel, qb = torch.is_tensor(selec), None
        if self.lik_type == "fourier_gauss":
            Y = nbody.rfftn(cm)
            Yb = torch.empty_like(Y)
            box, los = [float(v) for v in self.fwd.box_size], [float(v) for v in self.los_fid]
            plan.call("mcpm_lik_fourier_temp_f32", Y, self.obs_rg, *box, *los, float(selec), float(base["s_e"]), float(base["s_k2e"]),
                      float(base["s_kmu2e"]), float(f.temp), Yb, sums)
            keys = ("s_e", "s_k2e", "s_kmu2e")
        else:
            if mesh_sel:      # the selection made safe outside the mask
                selec = (selec if self.mask is None else torch.where(self.mask, selec, torch.ones_like(selec))).contiguous()
            family = {"shash": _lib.LIK_SHASH, "poisson": _lib.LIK_POISSON, "two_quad_gauss": _lib.LIK_TWO_QUAD}[self.lik_type]
            keys = self.LIK_STOCH[self.lik_type]
            cm_bar = torch.empty_like(cm)
            qb = torch.empty_like(cm) if (want_sqsel and mesh_sel) else None
            st = [float(base[k]) if keys else 0.0 for k in self.STOCH]
            quad = (self.quad[0], self.quad[1], self.N_QUAD) if family == _lib.LIK_TWO_QUAD else (None, None, 0)
            if f.phi is not None:
                f.phi_bar = torch.empty_like(f.phi)
                keys = keys + ("s_ep",)
            plan.call("mcpm_lik_real_phi_f32", family, C.c_int64(cm.numel()), self.count_obs, cm, selec if mesh_sel else None,
                      1.0 if mesh_sel else float(selec), self.mask, f.phi, *st, float(base.get("s_ep", 0.)), float(f.temp), *quad, cm_bar,
                      f.phi_bar, qb, sums)
        v = sums.cpu().numpy()
        if not need_grad:
            return float(v[0]), None, None, None
        if self.lik_type == "fourier_gauss":
            cm_bar = nbody.rfftn_vjp(Yb, overwrite=True)
        stoch_bar = {k: float(v[5 if k == "s_ep" else 1 + i]) for i, k in enumerate(keys)}
        if not want_sqsel:
            return float(v[0]), cm_bar, stoch_bar, None
        per = self._per_shell(cm_bar * f.dn)      # count = dn rc at fixed selec
        if mesh_sel:      # selec = |S rc| per cell
            per = per + self._per_shell(qb * 0.5 * selec ** -.5 * self.sel_down.abs() * torch.sign(f.rc))
            return float(v[0]), cm_bar, stoch_bar, per.cpu().numpy()
        return float(v[0]), cm_bar, stoch_bar, per.cpu().numpy() + float(v[4]) * 0.5 * selec ** -.5 / self.n_rbins      # selec = mean(rcounts)

    def _lik_quad_gauss(self, base, f, need_grad):
        """'quad_gauss' on its torch path (model.py:852-866, :893-908).
        Only the observed cells carry a likelihood term: the reference extracts them first (mesh2masked, model.py:856-863).
        Here every cell is evaluated, so the unobserved ones are given safe inputs (selection 1, count 0 -- a cut-sky
        selection is exactly 0 there and count / selec would be NaN) and are removed with `where`, never by multiplying."""
        obs, cmu, selec = self.count_obs, f.cm, f.selec
        if self.mask is not None:
            if torch.is_tensor(selec):
                selec = torch.where(self.mask, selec, torch.ones_like(selec))
            cmu = torch.where(self.mask, f.cm, torch.zeros_like(f.cm))
            obs = torch.where(self.mask, obs, torch.zeros_like(obs))
        delta = cmu / selec - 1.0
        lin = base["s_e"] + base["s_ed"] * delta
        s_ep, st = float(base.get("s_ep", 0.)), float(f.temp) ** .5
        if f.phi is not None:
            phi = f.phi if self.mask is None else torch.where(self.mask, f.phi, torch.zeros_like(f.phi))
            lin = lin + s_ep * phi
        b = (lin.abs() + 1e-9) * selec ** .5
        if st != 1.0:
            b = b * st
        a = 0.0 if abs(float(base["s_e2"])) < 1e-10 else float(base["s_e2"]) * selec ** .5
        lpe, g_loc, g_b, g_a = quad_gaussian_log_prob_and_grad(obs, cmu, b, a)
        if self.mask is not None:
            zero = torch.zeros_like(lpe)
            lpe, g_loc, g_b = torch.where(self.mask, lpe, zero), torch.where(self.mask, g_loc, zero), torch.where(self.mask, g_b, zero)
            g_a = torch.where(self.mask, g_a, zero) if torch.is_tensor(g_a) else g_a
        lp = float(lpe.double().sum())
        if not need_grad:
            return lp, None, None, None
        sgn = torch.sign(lin) * selec ** .5
        if st != 1.0:
            sgn = sgn * st
        cm_bar = g_loc + g_b * sgn * (base["s_ed"] / selec)
        stoch_bar = {"s_e": float((g_b * sgn).double().sum()), "s_ed": float((g_b * sgn * delta).double().sum()),
                     "s_e2": float((g_a * selec ** .5).double().sum())}
        if f.phi is not None:
            f.phi_bar = g_b * sgn * s_ep
            stoch_bar["s_ep"] = float((g_b * sgn * phi).double().sum())
        if self.ngb_lat is None:
            return lp, cm_bar, stoch_bar, None
        # d/d rcounts: through count = dn rc and through selec (|S rc| per cell, or mean(rcounts)), each in its closed form
        wsel = g_b * (lin.abs() + 1e-9) * st + (g_a * float(base["s_e2"]) if torch.is_tensor(g_a) else 0.0)   # d lp / d sqrt(selec)
        if self.sel_down is not None:
            # delta = count / selec does not move with rc; selec = |S| |rc|
            rc_bar = g_loc * f.dn + wsel * 0.5 * selec ** -.5 * self.sel_down.abs() * torch.sign(f.rc)
            return lp, cm_bar, stoch_bar, self._per_shell(rc_bar).cpu().numpy()
        per = self._per_shell(cm_bar * f.dn)
        common = float((-(g_b * sgn * base["s_ed"]) * cmu / selec ** 2 + wsel * 0.5 * selec ** -.5).double().sum())
        return lp, cm_bar, stoch_bar, per.cpu().numpy() + common / self.n_rbins

    def draw_counts(self, sample, seed=0):
        """One observed count mesh drawn from the likelihood at `sample` (model.py:873, :886, :901, :909, :929; temp = 1): float32 device tensor, final_shape,
        zero in the unobserved cells.  Host float64 draws on the mean counts of the HIP forward model; not on the hot path."""
        fwd, rng = self.fwd, np.random.default_rng(seed)
        base = self.base_params(sample)
        f = self._forward(base, sample["white_mesh_"], need_phi=True)
        cm, selec = f.cm, f.selec
        cm = cm.double().cpu().numpy()
        sel_mean = selec if not torch.is_tensor(selec) else None
        selec = selec.double().cpu().numpy() if torch.is_tensor(selec) else np.full(self.final_shape, selec)
        mask = np.ones(self.final_shape, bool) if self.mask is None else self.mask.cpu().numpy()
        cm, selec = np.where(mask, cm, 0.), np.where(mask, selec, 1.)
        eps = rng.standard_normal(self.final_shape)
        if self.lik_type == "poisson":
            obs = rng.poisson(np.abs(cm)).astype(np.float64)
        elif self.lik_type == "fourier_gauss":
            kvec = nbody.rfftk(self.final_shape, fwd.box_size)
            k2 = sum(ki ** 2 for ki in kvec)
            kl2 = sum(ki * li for ki, li in zip(kvec, self.los_fid)) ** 2      # (k mu)^2 = (k . los)^2, 0 at k = 0
            amp = np.abs(base["s_e"] + base["s_k2e"] * k2 + base["s_kmu2e"] * kl2) * sel_mean ** .5
            amp = np.broadcast_to(amp, r2chshape(self.final_shape))
            sigma = cgh2rg(torch.from_numpy(amp.astype(np.complex64)), norm="amp")
            obs_rg = cgh2rg(nbody.rfftn(cm.astype(np.float32))) + sigma * torch.from_numpy(eps.astype(np.float32)).to(sigma.device)
            return nbody.irfftn(rg2cgh(obs_rg))
        else:
            phi = 0. if f.phi is None else np.where(mask, f.phi.double().cpu().numpy(), 0.)
            b = (np.abs(base["s_e"] + base["s_ed"] * (cm / selec - 1.0) + float(base.get("s_ep", 0.)) * phi) + 1e-9) * selec ** .5
            a = float(base["s_e2"]) * selec ** .5
            if self.lik_type == "quad_gauss":      # utils.py:492-494
                obs = cm + b * eps + a * (eps ** 2 - 1.0)
            elif self.lik_type == "two_quad_gauss":      # two independent normals, utils.py:595-600
                obs = cm + b * eps + a * (rng.standard_normal(self.final_shape) ** 2 - 1.0)
            else:      # 'shash', utils.py:431-435
                from numpy.polynomial.hermite_e import hermegauss
                x, wq = hermegauss(20)
                wq = (wq / np.sqrt(2 * np.pi)).reshape(-1, 1, 1, 1)
                skew, tail = 3.540 * a / b, 1.0 + 5.884 * (a / b) ** 2
                Zq = np.sinh((np.arcsinh(x).reshape(-1, 1, 1, 1) + skew) * tail)
                m = (wq * Zq).sum(0)
                sd = np.sqrt((wq * Zq ** 2).sum(0) - m ** 2)
                obs = cm + np.sqrt(b ** 2 + 2 * a ** 2) * (np.sinh((np.arcsinh(eps) + skew) * tail) - m) / sd
        return nbody._f32(np.where(mask, obs, 0.), self.final_shape)

    def names(self):
        """Sample-space parameter names: scalars (in a fixed order) then 'white_mesh_'."""
        return [k + "_" for k in self.latents] + (["ngbars_"] if self.ngb_lat is not None else []) + ["white_mesh_"]

    def __call__(self, sample):
        return self.logdensity_and_grad(sample)[0]

    def _zero_grad(self, sample):
        """The gradient's full structure, all zeros."""
        zgrad = {name + "_": 0.0 for name in self.latents}
        if self.ngb_lat is not None:
            zgrad["ngbars_"] = np.zeros(self.n_rbins)
        w0 = sample["white_mesh_"]
        zgrad["white_mesh_"] = (torch.zeros_like(w0) if torch.is_tensor(w0)
                                else torch.zeros(self.fwd.init_shape, dtype=torch.float32, device=nbody._device()))
        return zgrad

    def _base_bar(self, f, g, stoch_bar):
        """Cotangents of the scalar base parameters from those of `evolve_vjp` (g) and of the likelihood; 0 for one that is not read."""
        base_bar = {k: 0.0 for k in bricks.PNG_KEYS}      # (without png_type the model does not read them)
        base_bar.update(g.get("png", {}))
        base_bar.update({k: 0.0 for k in bricks.AP_KEYS})      # (read only with ap_auto = False)
        base_bar.update(g.get("ap", {}))
        base_bar.update(g["bias"])
        base_bar.update({k: 0.0 for k in self.ALL_STOCH})      # (a stochastic parameter the likelihood does not read)
        base_bar.update(stoch_bar)
        base_bar["sigma8"] = g["sigma8"]
        if "Omega_m" in self.latents:
            base_bar["Omega_m"] = self.fwd.cosmo_vjp(f.ctx, g, params=("Omega_m",))["Omega_m"]
        return base_bar

    def logdensity_and_grad(self, sample, need_grad=True, temp_lik=1.):
        """sample: dict with the scalars `name_` (floats) and 'white_mesh_' (real tensor, fwd.init_shape).
        Returns (log density, dict of gradients with the same keys).  `temp_lik`: the temperature of the likelihood (model.py:840, `temp` of
        `_model(temp_prior, temp_lik)`): the noise scale of the Gaussian-like families times sqrt(temp_lik), the Poisson rate to the power
        1 / temp_lik; the priors are not tempered (`temp_prior` is not built)."""
        if not temp_lik > 0:
            raise ValueError("temp_lik must be positive")
        fwd = self.fwd
        lp, base, grad, dbase = self._prior(sample)
        if lp == -math.inf:      # a latent sits in a saturated tail: zero density whatever the field (no forward model needed)
            # the gradient keeps its full structure (zeros), so that callers which index it before looking at the value --
            # jax_bridge.logdensity_fn builds a tuple over all names -- get a rejected proposal, not a KeyError
            return -math.inf, (self._zero_grad(sample) if need_grad else None)
        w = nbody._f32(sample["white_mesh_"], fwd.init_shape)
        lp += self._white_prior(w)
        f = self._forward(base, w, need_ctx=True, need_phi=True)
        lik = self._lik_quad_gauss if self.lik_type == "quad_gauss" else self._lik_hip
        f.temp = float(temp_lik)
        lpl, cm_bar, stoch_bar, rcounts_bar = lik(base, f, need_grad)
        lp += lpl
        if not need_grad:
            return lp, None
        gxy_bar = self._down_vjp(cm_bar * f.rc, f.gxy.shape)
        if self.selec_mesh is not None:
            gxy_bar = gxy_bar * self.selec_mesh
        g = fwd.evolve_vjp(f.ctx, gxy_bar) if f.phi_bar is None else fwd.evolve_vjp(f.ctx, gxy_bar, phi_bar=f.phi_bar)
        wb = g["white_mesh"] * self.transfer
        wbar = nbody.rfftn_vjp(wb, overwrite=True) if self.precond == "real" else rg2cgh_vjp(wb)
        grad["white_mesh_"] = wbar - (w if self.scale is None else w / self.scale ** 2)
        if rcounts_bar is not None:
            grad["ngbars_"] = grad.pop("ngbars_") + rcounts_bar * fwd.cell_length ** 3 * dbase["ngbars"]
        base_bar = self._base_bar(f, g, stoch_bar)
        for name in self.latents:
            grad[name + "_"] += base_bar[name] * dbase[name]
        return lp, grad
