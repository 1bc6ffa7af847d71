"""Float64 numpy restatement of the real-space likelihoods of montecosmo/model.py:850-932 with the primordial stochastic term and the
temperature: 'quad_gauss', 'two_quad_gauss', 'shash' with
    scale1 = (|s_e + s_ed delta + s_ep phi| + 1e-9) sqrt(selec) sqrt(temp),   scale2 = s_e2 sqrt(selec),   delta = count / selec - 1
and 'poisson' with the rate |count|^(1 / temp); the checker of tests/test_likelihood_phi_host.py and tests/test_gpu_likelihood_phi.py.
TwoQuadGaussian.log_prob (utils.py:541-616) is restated twice: by the 64-node Gauss-Hermite rule the reference uses, and by brute-force
integration of N(obs; loc + s2 (eps^2 - 1), s1) N(eps; 0, 1) over eps.  Value and hand-written gradient per cell for the three families the
HIP kernel serves ('shash', 'two_quad_gauss', 'poisson'); `dtype=np.float32` runs the same arithmetic in single precision on the CPU,
sums over cells always in float64 (as tests/_lik_f64.py, whose SinhArcsinh pieces are imported).  `log_density` composes the families
with the oracle's prior + evolve and the PNG-enabled evolve of tests/_png_f64.py."""
import numpy as np
from numpy.polynomial.hermite_e import hermegauss
from scipy.special import gammaln

import _lik_f64 as L
import _png_f64 as pf
from oracle import pm_oracle as o, bias_oracle as bo, power_oracle as po

LOG2PI = np.log(2 * np.pi)
N_QUAD = 64
FAMILIES = ("shash", "two_quad_gauss", "poisson")


def quad_rule(n_quad=N_QUAD):
    """utils.py:589-591: nodes z_i and log wn_i = log w_i - log(2 pi) / 2 of E_{N(0,1)}[f] ~ sum wn_i f(z_i)."""
    z, w = hermegauss(n_quad)
    return z, np.log(w) - 0.5 * LOG2PI


def two_quad_log_prob(value, loc, s1, s2, n_quad=N_QUAD, dtype=np.float64):
    """utils.py:611-616: logsumexp_i [log wn_i + Normal(loc + s2 (z_i^2 - 1), s1).log_prob(value)]."""
    return two_quad_term(value, loc, s1, s2, n_quad, dtype)[0]


def two_quad_term(value, loc, s1, s2, n_quad=N_QUAD, dtype=np.float64):
    """(lp, d/d loc, d/d s1, d/d s2) of TwoQuadGaussian(loc, s1, s2).log_prob(value) by the n_quad-node rule, with the softmax weights
    p_i: sum p_i r_i / s1, sum p_i (r_i^2 - 1) / s1, sum p_i r_i (z_i^2 - 1) / s1,  r_i = (value - loc - s2 (z_i^2 - 1)) / s1."""
    value, loc, s1, s2 = np.broadcast_arrays(*(np.asarray(v, dtype=dtype) for v in (value, loc, s1, s2)))
    z, lw = quad_rule(n_quad)
    sh = (-1,) + (1,) * value.ndim
    q, lw = (z.astype(dtype) ** 2 - dtype(1)).reshape(sh), lw.astype(dtype).reshape(sh)
    r = (value - loc - s2 * q) / s1
    e = lw - dtype(0.5) * r * r
    m = e.max(0)
    p = np.exp(e - m)
    s0 = p.sum(0)
    lp = m + np.log(s0) - np.log(s1) - dtype(0.5 * LOG2PI)
    p = p / s0
    return lp, (p * r).sum(0) / s1, ((p * r * r).sum(0) - dtype(1)) / s1, (p * r * q).sum(0) / s1


def two_quad_density_brute(value, loc, s1, s2):
    """The density by adaptive quadrature of N(value; loc + s2 (eps^2 - 1), s1) N(eps; 0, 1) over eps (scalars, float64).  The
    integrand is even in eps; break points at the eps where the inner mean crosses `value` help the adaptive rule find the peaks."""
    from scipy.integrate import quad
    f = lambda e: np.exp(-0.5 * ((value - loc - s2 * (e * e - 1.)) / s1) ** 2 - 0.5 * e * e) / (2 * np.pi * s1)
    pts = None
    if s2 != 0. and (value - loc) / s2 + 1. > 0.:
        e0 = np.sqrt((value - loc) / s2 + 1.)
        pts = [e0] if e0 < 12. else None
    v, err = quad(f, 0., 12., points=pts, epsabs=0., epsrel=1e-12, limit=400)
    return 2. * v, 2. * err


def shash_term(value, loc, b, a, dtype=np.float64):
    """(lp, d/d loc, d/d b, d/d a) of the SinhArcsinh moment-matched to (b, a) (model.py:922-932): the arithmetic of
    tests/_lik_f64.py::shash_cells in terms of the two scales."""
    value, loc, b, a = (np.asarray(v, dtype=dtype) for v in (value, loc, b, a))
    rho = a / b
    sig, skew, tail = np.sqrt(b * b + dtype(2) * a * a), dtype(3.540) * rho, dtype(1) + dtype(5.884) * rho * rho
    m, s, m_sk, m_tl, s_sk, s_tl = L.shash_standardiser(skew, tail, dtype, derivs=True)
    d = (value - loc) / sig
    Z = m + s * d
    A = np.arcsinh(Z)
    eps = np.sinh(A / tail - skew)
    lp = (dtype(-0.5 * LOG2PI) - dtype(0.5) * eps ** 2 + dtype(0.5) * np.log1p(eps ** 2) - np.log(tail) - dtype(0.5) * np.log1p(Z ** 2)
          + np.log(s) - np.log(sig))
    gt = -eps ** 3 / np.sqrt(1 + eps ** 2)
    gZ = gt / (tail * np.sqrt(1 + Z * Z)) - Z / (1 + Z * Z)
    gs = 1 / s + gZ * d
    g_skew = -gt + gZ * m_sk + gs * s_sk
    g_tail = -gt * A / tail ** 2 - 1 / tail + gZ * m_tl + gs * s_tl
    g_sig = -(1 + gZ * s * d) / sig
    g_rho = dtype(3.540) * g_skew + dtype(2 * 5.884) * rho * g_tail
    return lp, -gZ * s / sig, g_sig * b / sig - g_rho * rho / b, g_sig * 2 * a / sig + g_rho / b


def scales(count, selec, phi, s_e, s_ed, s_e2, s_ep, temp, dtype=np.float64):
    """model.py:889-897 (the same lines for the three families): q = sqrt(selec), delta, lin, scale1 = b, scale2 = a."""
    count, selec, phi = (np.asarray(v, dtype=dtype) for v in (count, selec, phi))
    q = np.sqrt(selec)
    delta = count / selec - dtype(1)
    lin = dtype(s_e) + dtype(s_ed) * delta + dtype(s_ep) * phi
    st = np.sqrt(dtype(temp))
    return dict(q=q, delta=delta, lin=lin, st=st, b=(np.abs(lin) + dtype(1e-9)) * q * st, a=dtype(s_e2) * q * np.ones_like(lin))


def family_log_prob(family, obs, count, selec, phi, s_e=0., s_ed=0., s_e2=0., s_ep=0., temp=1.):
    """Per-cell log-probability of the four real-space families (float64), as model.py:872-873, :888-932 write them."""
    obs, count = np.asarray(obs, dtype=np.float64), np.asarray(count, dtype=np.float64)
    if family == "poisson":
        return poisson_cells(obs, count, temp)["lp"]
    P = scales(count, selec, phi, s_e, s_ed, s_e2, s_ep, temp)
    if family == "quad_gauss":
        return bo.quad_gaussian_log_prob(obs, count, P["b"], P["a"])
    if family == "two_quad_gauss":
        return two_quad_log_prob(obs, count, P["b"], P["a"])
    if family == "shash":
        r = P["a"] / P["b"]
        return L.shash_log_prob(obs, count, np.sqrt(P["b"] ** 2 + 2 * P["a"] ** 2), 3.540 * r, 1 + 5.884 * r ** 2)
    raise ValueError(family)


def poisson_cells(obs, count, temp=1., dtype=np.float64):
    """model.py:873: Poisson(|count|^(1 / temp)).log_prob(obs) and d/d count; rate 0: -inf (obs > 0) or 0, zero gradient."""
    obs, count = np.asarray(obs, dtype=dtype), np.asarray(count, dtype=dtype)
    ac = np.abs(count)
    pos = ac > 0
    acs = np.where(pos, ac, dtype(1))
    ll = np.log(acs) / dtype(temp)
    lam = np.exp(ll)
    with np.errstate(all="ignore"):
        lp = np.where(obs == 0, dtype(0), obs * ll) - lam - gammaln(obs + dtype(1)).astype(dtype)
        lp = np.where(pos, lp, np.where(obs > 0, dtype(-np.inf), dtype(0)))
    z = np.zeros_like(lp)
    return dict(lp=lp, count_bar=np.where(pos, np.sign(count) * (obs - lam) / (dtype(temp) * acs), z), phi_bar=z, sqsel_bar=z, s_e=z, s_ed=z,
                s_e2=z, s_ep=z)


def cells(family, obs, count, selec, phi, s_e, s_ed, s_e2, s_ep, temp, dtype=np.float64):
    """Per cell: lp, d lp / d count (fixed selec), d lp / d phi, d lp / d sqrt(selec) (fixed count) and the integrands of
    d/d s_e, s_ed, s_e2, s_ep -- the term's (d/d loc, d/d scale1, d/d scale2) chained as the kernel chains them."""
    if family == "poisson":
        return poisson_cells(obs, count, temp, dtype)
    obs, count = np.asarray(obs, dtype=dtype), np.asarray(count, dtype=dtype)
    P = scales(count, selec, phi, s_e, s_ed, s_e2, s_ep, temp, dtype)
    selec = np.asarray(selec, dtype=dtype) * np.ones_like(P["b"])
    term = shash_term if family == "shash" else two_quad_term
    lp, g_loc, g_b, g_a = term(obs, count, P["b"], P["a"], dtype=dtype)
    q, st = P["q"], P["st"]
    gl = g_b * np.sign(P["lin"]) * q * st      # d lp / d lin
    return dict(lp=lp, count_bar=g_loc + gl * dtype(s_ed) / selec, phi_bar=gl * dtype(s_ep),
                sqsel_bar=g_b * (np.abs(P["lin"]) + dtype(1e-9)) * st + g_a * dtype(s_e2) - 2 * gl * dtype(s_ed) * count / (selec * q),
                s_e=gl, s_ed=gl * P["delta"], s_e2=g_a * q, s_ep=gl * np.asarray(phi, dtype=dtype))


SUM_KEYS = ("lp", "s_e", "s_ed", "s_e2", "sqsel_bar", "s_ep")


def real_terms(family, obs, count, selec, mask, phi, s_e=0., s_ed=0., s_e2=0., s_ep=0., temp=1., dtype=np.float64):
    """What mcpm_lik_real_phi_f32 returns: the three meshes and the six float64 sums (lp, d s_e, d s_ed, d s_e2, sum sqsel_bar, d s_ep),
    plus `cells`, the per-cell integrands of the sums.  phi None: 0.  Unobserved cells are extracted first (mesh2masked)."""
    shape = np.shape(count)
    mask = np.ones(shape, bool) if mask is None else np.asarray(mask, bool)
    sel = np.broadcast_to(np.asarray(selec, dtype=np.float64), shape)
    ph = np.zeros(shape) if phi is None else np.asarray(phi, dtype=np.float64)
    c = cells(family, np.asarray(obs)[mask], np.asarray(count)[mask], sel[mask], ph[mask], s_e, s_ed, s_e2, s_ep, temp, dtype)
    full = lambda v: L._unmask(np.asarray(v), mask)
    return dict(count_bar=full(c["count_bar"]), phi_bar=full(c["phi_bar"]), sqsel_bar=full(c["sqsel_bar"]),
                sums=np.array([np.sum(c[k], dtype=np.float64) for k in SUM_KEYS]), cells=np.stack([c[k].astype(np.float64) for k in SUM_KEYS]))


# ---- phi out of evolve, onto the final mesh, and back (model.py:837, :869) -------------------------------------------------------------
def down(mesh, final):
    """irfftn(chreshape(rfftn(mesh), final_shape))."""
    final = tuple(final)
    if tuple(mesh.shape) == final:
        return mesh
    return o._irfftn(o.chreshape(o._rfftn(mesh), o.r2chshape(final)), s=final, axes=(0, 1, 2))


def phi_final(table, evol_mesh, box_size, final):
    """The likelihood's phi from the Gaussian evolution mesh: irfftn(safe_div(evol_mesh, t)) (what `lagrangian_bias` returns,
    bricks.py:415) brought to the final mesh (model.py:869)."""
    return down(pf.png_fields(table, evol_mesh, box_size)[0], final)


def evol_mesh(cfg, cosmo, white):
    """The Gaussian evolution mesh of evolve (model.py:745-749): white2lin, then chreshape to evol_shape."""
    kpow = cfg["lin_kpow"] if cfg["lin_kpow"] is not None else po.lin_power_table(cosmo)
    init = bo.white2lin(cosmo.sigma8, white, cfg["init_shape"], cfg["box_size"], kpow)
    return o.chreshape(init, o.r2chshape(cfg["evol_shape"]))


def log_density(cfg, latents, fixed, sample, count_obs, make_cosmo, lik_type, png_type, temp=1., info=None):
    """Single-feature restatement; the composed form is tests/_model_f64.py.  The patch of `bo.evolve` below puts the PNG-enabled evolve
    (and no other feature) under the oracle's log density; it stays as the composed oracle's independent witness.
    log p(sample, count_obs) with the likelihood `lik_type`, the term s_ep phi and the temperature `temp` of the likelihood: the
    oracle's prior + (PNG-enabled, tests/_png_f64.py) evolve + 'quad_gauss' term, minus that term recomputed from the intermediates it
    leaves in `aux` (evaluated at value = loc, see tests/_lik_f64.py::_CountAsObs), plus the family's term on the same mean counts.
    `make_cosmo(base)` must put the PNG parameters of the base point on the cosmology as `png_params`.  `info` (a dict) receives
    'phi', 's_ep_phi', 'count', 'selec', 'mask', 'base' and, for 'quad_gauss', 'D' = b^2 + 4 a (obs - loc + a) over the observed cells (the support is D > 0)."""
    aux, fx = {}, dict(fixed)
    for k, v in (("s_e", 1.0), ("s_ed", 0.0), ("s_e2", 0.0)):
        if k not in fx and k not in latents:
            fx[k] = v
    saved = bo.evolve
    if png_type is not None:
        bo.evolve = lambda cfg_, cosmo, bias, white: (pf.evolve(cfg_, cosmo, bias, white, cosmo.png_params, png_type), None)
    try:
        lp = bo.log_density(cfg, latents, fx, sample, L._CountAsObs(aux), make_cosmo, aux=aux)
    finally:
        bo.evolve = saved
    base, cm = aux["base"], aux["count"]
    final = tuple(cfg["final_shape"])
    mask = np.ones(final, bool) if cfg.get("mask_mesh") is None else np.asarray(cfg["mask_mesh"], bool)
    rcounts = np.atleast_1d(np.asarray(base["ngbars"], float)) * cfg["cell_length"] ** 3
    sel = cfg.get("selec_mesh")
    if sel is None:
        selec = np.mean(rcounts) * np.ones(final)
    else:
        redges = cfg.get("redges")
        redges = bo.radial_edges(cfg, len(rcounts)) if redges is None else redges
        selec = np.abs(bo.set_radial_count(down(np.asarray(sel, float), final), bo.radius_mesh(cfg, final), redges, rcounts))
    delta = cm / selec - 1
    scale1 = (np.abs(base["s_e"] + base["s_ed"] * delta) + 1e-9) * selec ** .5
    scale2 = base["s_e2"] * selec ** .5
    lp -= float(np.sum(bo.quad_gaussian_log_prob(cm[mask], cm[mask], scale1[mask], scale2[mask])))
    phi, s_ep = np.zeros(final), float(base.get("s_ep", 0.))
    if png_type is not None and cfg["evolution"] != "kaiser":
        cosmo = make_cosmo(base)
        phi = phi_final(pf.trans_table(cosmo), evol_mesh(cfg, cosmo, aux["white"]), cfg["box_size"], final)
        cosmo._workspace = {}
    obs = np.asarray(count_obs, dtype=np.float64)
    st = [base.get(k, 0.) for k in ("s_e", "s_ed", "s_e2")]
    if info is not None:
        info.update(phi=phi, s_ep_phi=s_ep * phi[mask], count=cm, selec=selec, mask=mask, base=base)
        if lik_type == "quad_gauss":
            P = scales(cm[mask], selec[mask], phi[mask], *st, s_ep, temp)
            info["D"] = P["b"] ** 2 + 4 * P["a"] * (obs[mask] - cm[mask] + P["a"])
    return lp + float(np.sum(family_log_prob(lik_type, obs[mask], cm[mask], selec[mask], phi[mask], *st, s_ep, temp)))


# ---- the phi path of evolve_vjp, restated (float64): phi_final is linear in the evolution mesh, its adjoint is written by hand ----------
def rfftn_adj(spec_bar, shape):
    """Adjoint of rfftn in the real-pair convention: half-spectrum cotangent -> real mesh."""
    s = np.array(spec_bar, dtype=np.complex128)
    s[..., 1:(shape[-1] + 1) // 2] *= 0.5
    return o._irfftn(s, s=tuple(shape), axes=(0, 1, 2)) * np.prod(shape)


def irfftn_adj(mesh_bar):
    """Adjoint of irfftn in the real-pair convention: real cotangent -> half-spectrum."""
    k = o._rfftn(mesh_bar) / mesh_bar.size
    k[..., 1:(mesh_bar.shape[-1] + 1) // 2] *= 2.
    return k


def chreshape_adj(out_bar, in_shape):
    """Adjoint of chreshape (real-linear in (Re, Im)) from half-shape `in_shape`, column by column through the oracle (small shapes)."""
    res = np.zeros(in_shape, dtype=np.complex128)
    e = np.zeros(in_shape, dtype=np.complex128)
    pair = lambda a, b: float((a.real * b.real + a.imag * b.imag).sum())
    for idx in np.ndindex(*in_shape):
        e[idx] = 1.
        re = pair(o.chreshape(e, out_bar.shape), out_bar)
        e[idx] = 1j
        im = pair(o.chreshape(e, out_bar.shape), out_bar)
        e[idx] = 0.
        res[idx] = re + 1j * im
    return res


def phi_final_vjp(table, phi_bar, evol_shape, box_size):
    """Cotangent of the final-mesh phi -> cotangent of the Gaussian evolution mesh (real-pair convention):
    irfftn_adj -> chreshape_adj -> rfftn_adj (to the evolution-mesh phi), then irfftn_adj and the divide by t (safe_div)."""
    evol_shape = tuple(evol_shape)
    pb = np.asarray(phi_bar, dtype=np.float64)
    if pb.shape != evol_shape:
        pb = rfftn_adj(chreshape_adj(irfftn_adj(pb), o.r2chshape(evol_shape)), evol_shape)
    return o.safe_div(irfftn_adj(pb), pf.trans_mesh(table, evol_shape, box_size))


def self_check():
    """The restated gradients against float64 central differences (1e-7)."""
    rng = np.random.default_rng(5)
    n = 40
    count, selec, obs = rng.uniform(40., 90., n), rng.uniform(50., 80., n), rng.uniform(30., 100., n)
    phi = 3e-5 * rng.standard_normal(n)
    worst = 0.
    for family in FAMILIES:
        for s_e2, temp in ((0.08, 1.), (-0.08, 2.5), (0., 2.5)):
            pr = (0.9, 0.4, s_e2, 4e3)
            c = cells(family, obs, count, selec, phi, *pr, temp)
            f = lambda **kw: cells(family, obs, kw.get("count", count), kw.get("selec", selec), kw.get("phi", phi), *kw.get("pr", pr), temp)["lp"]
            # relative to the largest entry, with a floor of one unit of lp per unit of the argument: d/d s_e2 at s_e2 = 0 is exactly 0
            # for 'two_quad_gauss' (sum p_i (z_i^2 - 1) = 0) and its central difference is round-off
            close = lambda got, fd, floor=1.: np.abs(got - fd).max() / max(np.abs(fd).max(), floor)
            h = 1e-5
            errs = [close(c["count_bar"], (f(count=count + h) - f(count=count - h)) / (2 * h)),
                    close(c["sqsel_bar"], (f(selec=(selec ** .5 + h) ** 2) - f(selec=(selec ** .5 - h) ** 2)) / (2 * h))]
            if family != "poisson":
                hp = 1e-9
                errs.append(close(c["phi_bar"], (f(phi=phi + hp) - f(phi=phi - hp)) / (2 * hp)))
                for i, k in enumerate(("s_e", "s_ed", "s_e2", "s_ep")):
                    hh = h * (1e4 if k == "s_ep" else 1.)
                    e = np.eye(4)[i] * hh
                    errs.append(close(c[k], (f(pr=tuple(np.add(pr, e))) - f(pr=tuple(np.subtract(pr, e)))) / (2 * hh),
                                      np.abs(phi).max() if k == "s_ep" else 1.))
            else:
                errs = errs[:1]
            worst = max(worst, max(errs))
    return worst
