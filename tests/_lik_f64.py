"""Float64 numpy restatement of the 'shash', 'poisson' and 'fourier_gauss' likelihoods of montecosmo/model.py:872-886, :911-932
(SinhArcsinh: utils.py:386-450), the checker of tests/test_likelihood_host.py and tests/test_gpu_likelihood.py.  Value and hand-written
gradient per cell, the gradient itself checked against float64 central differences by `self_check`.  `dtype=np.float32` runs the same
arithmetic in single precision on the CPU: the measure of what float32 can deliver.  Sums over cells are always float64, as on the
device, so a deviation measures the per-cell arithmetic and not a summation order.  Wavevectors, cgh2rg and the prior + evolve part of
the log density come from the oracle (read-only)."""
import numpy as np
from numpy.polynomial.hermite_e import hermegauss
from scipy.special import gammaln

from oracle import pm_oracle as o, bias_oracle as bo

_X, _W = hermegauss(20)
_W = _W / np.sqrt(2 * np.pi)
_A = np.arcsinh(_X)
LOG2PI = np.log(2 * np.pi)


def _nodes(dtype, ndim):
    sh = (-1,) + (1,) * ndim
    return _A.astype(dtype).reshape(sh), _W.astype(dtype).reshape(sh)


def shash_standardiser(skew, tail, dtype=np.float64, derivs=False):
    """utils.py:416-429: mean and std of Z = sinh((asinh(eps) + skew) tail), eps ~ N(0, 1), by the 20-node rule; with `derivs` also
    (dm/dskew, dm/dtail, ds/dskew, ds/dtail) from the same nodes."""
    skew, tail = np.asarray(skew, dtype=dtype), np.asarray(tail, dtype=dtype)
    a, w = _nodes(dtype, max(skew.ndim, tail.ndim))
    u = (a + skew) * tail
    Z, Cc = np.sinh(u), np.cosh(u)
    m = (w * Z).sum(0)
    s = np.sqrt((w * Z * Z).sum(0) - m * m)
    if not derivs:
        return m, s
    m_sk, m_tl = tail * (w * Cc).sum(0), (w * Cc * (a + skew)).sum(0)
    s_sk = (tail * (w * Z * Cc).sum(0) - m * m_sk) / s
    s_tl = ((w * Z * Cc * (a + skew)).sum(0) - m * m_tl) / s
    return m, s, m_sk, m_tl, s_sk, s_tl


def shash_log_prob(value, loc, scale, skew, tail, dtype=np.float64):
    """SinhArcsinh(mean, std, skewness, tailweight).log_prob(value), utils.py:437-450."""
    value, loc, scale, skew, tail = (np.asarray(v, dtype=dtype) for v in (value, loc, scale, skew, tail))
    m, s = shash_standardiser(skew, tail, dtype)
    Z = m + s * (value - loc) / scale
    eps = np.sinh(np.arcsinh(Z) / tail - skew)
    return (dtype(-0.5 * LOG2PI) - dtype(0.5) * eps ** 2 + dtype(0.5) * np.log1p(eps ** 2) - np.log(tail) - dtype(0.5) * np.log1p(Z ** 2)
            + np.log(s) - np.log(scale))


def shash_sample(rng, loc, scale, skew, tail):
    """utils.py:431-435."""
    m, s = shash_standardiser(skew, tail)
    eps = rng.standard_normal(np.broadcast(loc, scale, skew, tail).shape)
    return loc + scale * (np.sinh((np.arcsinh(eps) + skew) * tail) - m) / s


def shash_params(count, selec, s_e, s_ed, s_e2, dtype=np.float64):
    """model.py:912-932: (mean, std, skewness, tailweight) of the SinhArcsinh and the intermediates the gradient needs."""
    count, selec = np.asarray(count, dtype=dtype), np.asarray(selec, dtype=dtype)
    q = np.sqrt(selec)
    delta = count / selec - dtype(1)
    lin = dtype(s_e) + dtype(s_ed) * delta
    b = (np.abs(lin) + dtype(1e-9)) * q
    a = dtype(s_e2) * q * np.ones_like(b)
    rho = a / b
    return dict(q=q, delta=delta, lin=lin, b=b, a=a, rho=rho, std=np.sqrt(b * b + dtype(2) * a * a), skew=dtype(3.540) * rho,
                tail=dtype(1) + dtype(5.884) * rho * rho)


def shash_cells(obs, count, selec, s_e, s_ed, s_e2, dtype=np.float64):
    """Per cell: lp, d lp / d count (fixed selec), d lp / d sqrt(selec) (fixed count) and the integrands of d/d s_e, s_ed, s_e2."""
    obs = np.asarray(obs, dtype=dtype)
    P = shash_params(count, selec, s_e, s_ed, s_e2, dtype)
    count, selec = np.asarray(count, dtype=dtype), np.asarray(selec, dtype=dtype) * np.ones_like(P["b"])
    b, a, rho, sig, skew, tail, q = P["b"], P["a"], P["rho"], P["std"], P["skew"], P["tail"], P["q"]
    m, s, m_sk, m_tl, s_sk, s_tl = shash_standardiser(skew, tail, dtype, derivs=True)
    d = (obs - count) / sig
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
    g_loc = -gZ * s / sig
    g_b = g_sig * b / sig - g_rho * rho / b
    g_a = g_sig * 2 * a / sig + g_rho / b
    gl = g_b * np.sign(P["lin"]) * q
    return dict(lp=lp, count_bar=g_loc + gl * dtype(s_ed) / selec,
                sqsel_bar=g_b * (np.abs(P["lin"]) + dtype(1e-9)) + g_a * dtype(s_e2) - 2 * gl * dtype(s_ed) * count / (selec * q),
                s_e=gl, s_ed=gl * P["delta"], s_e2=g_a * q)


def poisson_cells(obs, count, dtype=np.float64):
    """model.py:873 at temp = 1: Poisson(|count|).log_prob(obs) and d/d count; lambda = 0: -inf (obs > 0) or 0, zero gradient."""
    obs, count = np.asarray(obs, dtype=dtype), np.asarray(count, dtype=dtype)
    lam = np.abs(count)
    pos = lam > 0
    ls = np.where(pos, lam, dtype(1))
    with np.errstate(all="ignore"):
        lp = np.where(obs == 0, dtype(0), obs * np.log(ls)) - ls - gammaln(obs + dtype(1)).astype(dtype)
        lp = np.where(pos, lp, np.where(obs > 0, dtype(-np.inf), dtype(0)))
    z = np.zeros_like(lp)
    return dict(lp=lp, count_bar=np.where(pos, np.sign(count) * (obs / ls - 1), z), sqsel_bar=z, s_e=z, s_ed=z, s_e2=z)


def real_terms(family, obs, count, selec, mask, s_e=0., s_ed=0., s_e2=0., dtype=np.float64):
    """What mcpm_lik_real_f32 returns: the two meshes and the five float64 sums (lp, d s_e, d s_ed, d s_e2, sum sqsel_bar), plus `cells`,
    the per-cell integrands of the sums.  Unobserved cells are extracted first, as the reference does (mesh2masked, model.py:856-863)."""
    shape = np.shape(count)
    mask = np.ones(shape, bool) if mask is None else np.asarray(mask, bool)
    sel = np.broadcast_to(np.asarray(selec, dtype=np.float64), shape)
    args = (np.asarray(obs)[mask], np.asarray(count)[mask])
    c = shash_cells(*args, sel[mask], s_e, s_ed, s_e2, dtype) if family == "shash" else poisson_cells(*args, dtype)
    full = lambda v: _unmask(v, mask)
    keys = ("lp", "s_e", "s_ed", "s_e2", "sqsel_bar")
    return dict(count_bar=full(c["count_bar"]), sqsel_bar=full(c["sqsel_bar"]),
                sums=np.array([np.sum(c[k], dtype=np.float64) for k in keys]), cells=np.stack([c[k].astype(np.float64) for k in keys]))


def _unmask(v, mask):
    out = np.zeros(mask.shape, dtype=v.dtype)
    out[mask] = v
    return out


def fourier_sigma_terms(shape, box_size, los, dtype=np.float64):
    """k^2 and (k mu)^2 on the half-spectrum (model.py:877-880), laid out like the real tensor by cgh2rg(norm='amp')."""
    kvec = o.rfftk(tuple(shape), np.asarray(box_size, dtype=np.float64))
    kmesh = sum(ki ** 2 for ki in kvec) ** .5
    mu = o.safe_div(sum(ki * li for ki, li in zip(kvec, los)), kmesh)
    amp = lambda x: o.cgh2rg((x * np.ones(o.r2chshape(tuple(shape)))).astype(complex), norm="amp").astype(dtype)
    return amp(kmesh ** 2), amp((kmesh * mu) ** 2)


def cgh2rg_adjoint(g):
    """Adjoint of the real-linear map (Re Y, Im Y) -> cgh2rg(Y), column by column through the oracle (small shapes only): the cotangent of the
    half-spectrum in the real-pair convention."""
    shape = g.shape
    hs = o.r2chshape(shape)
    out = np.zeros(hs, dtype=complex)
    e = np.zeros(hs, dtype=complex)
    for idx in np.ndindex(*hs):
        e[idx] = 1.
        re = float((o.cgh2rg(e) * g).sum())
        e[idx] = 1j
        im = float((o.cgh2rg(e) * g).sum())
        e[idx] = 0.
        out[idx] = re + 1j * im
    return out


def fourier_terms(Y, obs_rg, box_size, los, selec, s_e, s_k2e, s_kmu2e, dtype=np.float64, adjoint=True):
    """What mcpm_lik_fourier_f32 returns: Y_bar (real-pair cotangent of the half-spectrum) and the five sums (lp, d s_e, d s_k2e, d s_kmu2e,
    d sqrt(selec)); model.py:875-886 with Y = rfftn(count_mesh), obs_rg = cgh2rg(rfftn(count_obs))."""
    shape = o.ch2rshape(np.shape(Y))
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    loc = o.cgh2rg(np.asarray(Y).astype(cdt).astype(complex)).astype(dtype)      # the inputs rounded to `dtype`; the permutation is exact
    k2, kmu2 = fourier_sigma_terms(shape, box_size, los, dtype)
    q = dtype(np.sqrt(dtype(selec)))
    lin = dtype(s_e) + dtype(s_k2e) * k2 + dtype(s_kmu2e) * kmu2
    sigma = np.abs(lin) * q
    z = (np.asarray(obs_rg, dtype=dtype) - loc) / sigma
    lp = dtype(-0.5 * LOG2PI) - np.log(sigma) - dtype(0.5) * z * z
    gs = (z * z - 1) / sigma
    sg = np.sign(lin) * q
    cells = np.stack([lp, gs * sg, gs * sg * k2, gs * sg * kmu2, gs * np.abs(lin)]).astype(np.float64)
    out = dict(sums=cells.reshape(5, -1).sum(1), cells=cells, loc_bar=(z / sigma).astype(np.float64))
    if adjoint:
        out["Y_bar"] = cgh2rg_adjoint(out["loc_bar"])
    return out


class _CountAsObs:
    """Stands in for count_obs in the oracle's log density: converts to the model's own mean counts, which the oracle has put into
    `aux` by the time it reads the observation.  The oracle's 'quad_gauss' term is then evaluated at value = loc, inside the support
    for every scale2, so it is finite and can be subtracted exactly."""

    def __init__(self, aux):
        self.aux = aux

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self.aux["count"], dtype=dtype)


def log_density(cfg, latents, fixed, sample, count_obs, make_cosmo, lik_type, los_fid=None):
    """log p(sample, count_obs) with the likelihood `lik_type`: the oracle's prior + evolve + 'quad_gauss' term, minus that term
    recomputed from the intermediates it leaves in `aux`, plus the new family's term on the same mean counts."""
    aux = {}
    fx = dict(fixed)
    for k, v in (("s_e", 1.0), ("s_ed", 0.0), ("s_e2", 0.0)):      # parameters the family does not read: any value, the term is removed
        if k not in fx and k not in latents:
            fx[k] = v
    lp = bo.log_density(cfg, latents, fx, sample, _CountAsObs(aux), make_cosmo, aux=aux)
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
        down = o._irfftn(o.chreshape(o._rfftn(np.asarray(sel, float)), o.r2chshape(final)), s=final, axes=(0, 1, 2))
        selec = np.abs(bo.set_radial_count(down, bo.radius_mesh(cfg, final), redges, rcounts))
    delta = cm / selec - 1
    scale1 = (np.abs(base["s_e"] + base["s_ed"] * delta) + 1e-9) * selec ** .5
    scale2 = base["s_e2"] * selec ** .5
    lp -= float(np.sum(bo.quad_gaussian_log_prob(cm[mask], cm[mask], scale1[mask], scale2[mask])))
    obs = np.asarray(count_obs, dtype=np.float64)
    if lik_type == "shash":
        P = shash_params(cm[mask], selec[mask], base["s_e"], base["s_ed"], base["s_e2"])
        return lp + float(np.sum(shash_log_prob(obs[mask], cm[mask], P["std"], P["skew"], P["tail"])))
    if lik_type == "poisson":
        return lp + float(np.sum(poisson_cells(obs[mask], cm[mask])["lp"]))
    if lik_type == "fourier_gauss":
        assert cfg.get("mask_mesh") is None and sel is None
        t = fourier_terms(o._rfftn(cm), o.cgh2rg(o._rfftn(obs)), cfg["box_size"], los_fid, float(np.mean(rcounts)), base["s_e"],
                          base["s_k2e"], base["s_kmu2e"], adjoint=False)
        return lp + float(t["sums"][0])
    raise ValueError(lik_type)


def self_check():
    """The restatement against what is known without it."""
    rng = np.random.default_rng(5)
    x = rng.normal(3., 2., 50)
    normal = -0.5 * LOG2PI - np.log(1.7) - 0.5 * ((x - 2.5) / 1.7) ** 2
    assert np.allclose(shash_log_prob(x, 2.5, 1.7, 0., 1.), normal, rtol=0, atol=1e-12)      # skewness 0, tailweight 1: Normal
    # a density; its mean and standard deviation are loc and scale as far as the 20-node rule integrates sinh: the rule's own error at
    # these shapes is ~1e-5 of the scale (against a 200-node rule: 7e-6 in m, 6e-6 in s, times scale / s = 2), hence 1e-4
    for skew in (0.35, -0.35):
        t = np.linspace(-60., 60., 1200001)
        p = np.exp(shash_log_prob(t, 1.5, 2.0, skew, 1.06))
        dt = t[1] - t[0]
        n0, n1 = p.sum() * dt, (p * t).sum() * dt
        n2 = (p * (t - n1) ** 2).sum() * dt
        assert abs(n0 - 1) < 1e-8 and abs(n1 - 1.5) < 1e-4 and abs(n2 ** .5 - 2.0) < 1e-4, (skew, n0, n1, n2 ** .5)
    y = rng.standard_normal((4, 6, 8))
    assert abs(np.linalg.norm(o.cgh2rg(np.fft.rfftn(y))) - np.linalg.norm(y)) < 1e-12 * np.linalg.norm(y)      # the map is orthogonal
    # the hand-written gradients against central differences
    n = 40
    count, selec, obs = rng.uniform(40., 90., n), rng.uniform(50., 80., n), rng.uniform(30., 100., n)
    for s_e2 in (0.08, -0.08, 0.):
        pr = (0.9, 0.4, s_e2)
        c = shash_cells(obs, count, selec, *pr)
        f = lambda **kw: shash_cells(obs, kw.get("count", count), kw.get("selec", selec), *kw.get("pr", pr))["lp"]
        h = 1e-5
        fd = (f(count=count + h) - f(count=count - h)) / (2 * h)
        assert np.allclose(c["count_bar"], fd, rtol=1e-6, atol=1e-8), np.abs(c["count_bar"] - fd).max()
        fd = (f(selec=(selec ** .5 + h) ** 2) - f(selec=(selec ** .5 - h) ** 2)) / (2 * h)
        assert np.allclose(c["sqsel_bar"], fd, rtol=1e-6, atol=1e-8), np.abs(c["sqsel_bar"] - fd).max()
        for i, k in enumerate(("s_e", "s_ed", "s_e2")):
            e = np.eye(3)[i] * h
            fd = (f(pr=tuple(np.add(pr, e))) - f(pr=tuple(np.subtract(pr, e)))) / (2 * h)
            assert np.allclose(c[k], fd, rtol=1e-6, atol=1e-7), (k, np.abs(c[k] - fd).max())
    pc = poisson_cells(np.array([3., 0., 2., 5.]), np.array([2.5, 0., 0., -4.]))
    assert pc["lp"][1] == 0. and pc["lp"][2] == -np.inf and pc["count_bar"][2] == 0. and abs(pc["count_bar"][3] + (5 / 4 - 1)) < 1e-15
    assert abs(pc["lp"][0] - (3 * np.log(2.5) - 2.5 - np.log(6.))) < 1e-14
    # fourier_gauss: sums and Y_bar against central differences
    shape, box, los = (4, 6, 8), (100., 150., 200.), np.array([0.3, -0.5, 0.81])
    cnt, ob = rng.uniform(40., 90., shape), rng.uniform(40., 90., shape)
    Y, org = np.fft.rfftn(cnt), o.cgh2rg(np.fft.rfftn(ob))
    pr = (60., 1.1, -40., 900.)      # selec, s_e, s_k2e, s_kmu2e
    t = fourier_terms(Y, org, box, los, *pr)
    f = lambda Y_=Y, pr_=pr: fourier_terms(Y_, org, box, los, *pr_, adjoint=False)["sums"][0]
    for i in range(1, 4):
        h = 1e-5 * abs(pr[i])
        e = np.eye(4)[i] * h
        fd = (f(pr_=tuple(np.add(pr, e))) - f(pr_=tuple(np.subtract(pr, e)))) / (2 * h)
        assert abs(fd - t["sums"][i]) < 1e-6 * abs(fd) + 1e-9, (i, fd, t["sums"][i])
    h = 1e-5
    fd = (f(pr_=((pr[0] ** .5 + h) ** 2,) + pr[1:]) - f(pr_=((pr[0] ** .5 - h) ** 2,) + pr[1:])) / (2 * h)
    assert abs(fd - t["sums"][4]) < 1e-6 * abs(fd), (fd, t["sums"][4])
    dc = rng.standard_normal(shape)      # a real perturbation of the counts: dlp = <Y_bar, rfftn(dc)> over the stored modes
    fd = (f(Y_=np.fft.rfftn(cnt + 1e-4 * dc)) - f(Y_=np.fft.rfftn(cnt - 1e-4 * dc))) / 2e-4
    dY = np.fft.rfftn(dc)
    an = float((t["Y_bar"].real * dY.real + t["Y_bar"].imag * dY.imag).sum())
    assert abs(fd - an) < 1e-6 * abs(fd) + 1e-9, (fd, an)
    return True
