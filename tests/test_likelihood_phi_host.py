"""Host checks of tests/_lik_phi_f64.py, the float64 restatement behind tests/test_gpu_likelihood_phi.py: 'two_quad_gauss' (the 64-node
rule against brute-force integration, the Gaussian limit, the moments of its draws), the hand-written gradients of the three kernel
families with the term s_ep phi and a temperature against central differences, the phi path of evolve_vjp as a dot-product identity,
and the argument checks that run before any device work.

Measured here: the 64-node density against the adaptive integral over s2 / s1 in {0, 0.1, 1/3} and (obs - loc) / s1 in [-4, 6] is off by
at most 1.66e-6 relative, at s2 / s1 = 1/3 (1e-5 allowed; the reference's docstring claims ~1e-5 at 32 nodes for s2 <= s1 / 3); the restated gradients are
within 2.0e-8 of central differences, relative to the largest entry (1e-7 allowed)."""
import numpy as np
import pytest

import _lik_phi_f64 as P
import _png_f64 as pf
from oracle import pm_oracle as o, background as obg


def test_two_quad_rule_against_brute_force_integral():
    """The 64-node value of TwoQuadGaussian.log_prob against quad() of N(obs; loc + s2 (eps^2 - 1), s1) N(eps): 1e-5 relative on the
    density over s2 / s1 in {0, 0.1, 1/3} (both signs of s2) and (obs - loc) / s1 in [-4, 6]."""
    loc, s1, worst = 3., 1.7, 0.
    for ratio in (0., 0.1, -0.1, 1 / 3, -1 / 3):
        for x in np.linspace(-4., 6., 41):
            obs = loc + x * s1
            rule = float(np.exp(P.two_quad_log_prob(obs, loc, s1, ratio * s1)))
            brute, err = P.two_quad_density_brute(obs, loc, s1, ratio * s1)
            assert err < 1e-9 * brute, (ratio, x, brute, err)      # the adaptive integral knows its value far better than the gate
            worst = max(worst, abs(rule - brute) / brute)
            assert abs(rule - brute) < 1e-5 * brute, (ratio, x, rule, brute)
    print(f"\n64-node rule against the adaptive integral: largest relative difference of the density {worst:.3e}")


def test_two_quad_gaussian_limit():
    rng = np.random.default_rng(3)
    x, loc, s1 = rng.normal(3., 4., 200), rng.normal(3., 1., 200), rng.uniform(0.5, 3., 200)
    normal = -0.5 * P.LOG2PI - np.log(s1) - 0.5 * ((x - loc) / s1) ** 2
    assert np.abs(P.two_quad_log_prob(x, loc, s1, 0.) - normal).max() < 1e-12
    lp, g_loc, g_b, g_a = P.two_quad_term(x, loc, s1, 0.)
    z = (x - loc) / s1
    assert np.allclose(g_loc, z / s1, rtol=1e-12, atol=1e-13) and np.allclose(g_b, (z * z - 1) / s1, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("s2", [0.6, -0.6])
def test_two_quad_draws_have_the_mean_and_variance(s2):
    """obs = loc + s1 eps1 + s2 (eps2^2 - 1) with two independent normals (utils.py:595-600, the draw of `draw_counts`): the sample mean
    within 5 standard errors of loc, the sample variance within 5 standard errors of s1^2 + 2 s2^2 (the standard error of a variance from
    the fourth central moment mu4 = 3 s1^4 + 12 s1^2 s2^2 + 60 s2^4: Var[s^2] = (mu4 - var^2) / n)."""
    rng = np.random.default_rng(17)
    n, loc, s1 = 400000, 12., 1.7
    obs = loc + s1 * rng.standard_normal(n) + s2 * (rng.standard_normal(n) ** 2 - 1.)
    var = s1 ** 2 + 2 * s2 ** 2
    mu4 = 3 * s1 ** 4 + 12 * s1 ** 2 * s2 ** 2 + 60 * s2 ** 4
    assert abs(obs.mean() - loc) < 5 * np.sqrt(var / n)
    assert abs(obs.var() - var) < 5 * np.sqrt((mu4 - var ** 2) / n)
    # and the density the rule gives has these moments: it is the density of these draws
    t = np.linspace(loc - 40., loc + 60., 400001)
    p = np.exp(P.two_quad_log_prob(t, loc, s1, s2))
    dt = t[1] - t[0]
    m0, m1 = p.sum() * dt, (p * t).sum() * dt
    assert abs(m0 - 1) < 1e-8 and abs(m1 - loc) < 1e-6 and abs((p * (t - m1) ** 2).sum() * dt - var) < 1e-5


def test_restated_gradients_against_central_differences():
    worst = P.self_check()
    print(f"\nrestated gradients against central differences: largest relative difference {worst:.3e}")
    assert worst < 1e-7


def test_family_log_prob_agrees_with_cells_and_with_the_plain_restatement():
    """The value route (`family_log_prob`, what `log_density` adds up) and the gradient route (`cells`) are the same numbers; with
    s_ep = 0 and temp = 1 they are tests/_lik_f64.py's; temp enters scale1 as sqrt(temp) and the Poisson rate as a power."""
    import _lik_f64 as L
    rng = np.random.default_rng(8)
    n = 60
    count, selec, obs, phi = rng.uniform(40., 90., n), rng.uniform(50., 80., n), np.rint(rng.uniform(30., 100., n)), 3e-5 * rng.standard_normal(n)
    pr = (0.9, 0.4, 0.08, 4e3)
    for fam in P.FAMILIES:
        a = P.family_log_prob(fam, obs, count, selec, phi, *pr, temp=2.5)
        b = P.cells(fam, obs, count, selec, phi, *pr, 2.5)["lp"]
        assert np.abs(a - b).max() < 1e-11, fam
    plain = L.shash_cells(obs, count, selec, *pr[:3])
    mine = P.cells("shash", obs, count, selec, phi, *pr[:3], 0., 1.)
    for k in ("lp", "count_bar", "sqsel_bar", "s_e", "s_ed", "s_e2"):
        assert np.abs(plain[k] - mine[k]).max() <= 1e-12 * np.abs(plain[k]).max(), k
    assert np.abs(L.poisson_cells(obs, count)["lp"] - P.poisson_cells(obs, count, 1.)["lp"]).max() < 1e-11
    lam = np.abs(count) ** (1 / 2.5)
    from scipy.special import gammaln
    assert np.abs(P.poisson_cells(obs, count, 2.5)["lp"] - (obs * np.log(lam) - lam - gammaln(obs + 1))).max() < 1e-11
    # quad_gauss: scale1 carries sqrt(temp) and the phi term
    from oracle import bias_oracle as bo
    q = P.family_log_prob("quad_gauss", obs, count, selec, phi, *pr, temp=2.5)
    b1 = (np.abs(pr[0] + pr[1] * (count / selec - 1) + pr[3] * phi) + 1e-9) * np.sqrt(selec) * np.sqrt(2.5)
    assert np.array_equal(q, bo.quad_gaussian_log_prob(obs, count, b1, pr[2] * np.sqrt(selec)))


def test_phi_path_dot_product_identity():
    """phi on the final mesh is linear in the Gaussian evolution mesh X: <phi_bar, phi_final(dX)> = <phi_final_vjp(phi_bar), dX> in the
    real-pair convention, for a Hermitian direction and for one interior mode with an arbitrary complex value.  14^3 -> 8^3: the
    chreshape between them aggregates the Nyquist planes."""
    rng = np.random.default_rng(21)
    evol, final, box = (14, 14, 14), (8, 8, 8), (320., 320., 320.)
    cosmo = obg.Planck18()
    table = pf.trans_table(cosmo)
    pb = rng.standard_normal(final)
    vjp = P.phi_final_vjp(table, pb, evol, box)
    dH = np.fft.rfftn(rng.standard_normal(evol))
    d1 = np.zeros_like(dH)
    d1[2, 3, 1] = 0.7 - 1.3j
    for tag, d in (("hermitian", dH), ("single mode", d1)):
        lhs = float((pb * P.phi_final(table, d, box, final)).sum())
        rhs = float((vjp.real * d.real + vjp.imag * d.imag).sum())
        print(f"\nphi path, {tag}: {lhs:.15e} {rhs:.15e}")
        assert abs(lhs - rhs) < 1e-12 * max(abs(lhs), np.linalg.norm(vjp) * np.linalg.norm(d) * 1e-3), (tag, lhs, rhs)
    # same shapes: no reshape on the way
    pb = rng.standard_normal(evol)
    vjp = P.phi_final_vjp(table, pb, evol, box)
    lhs, rhs = float((pb * P.phi_final(table, dH, box, evol)).sum()), float((vjp.real * dH.real + vjp.imag * dH.imag).sum())
    assert abs(lhs - rhs) < 1e-12 * abs(lhs)


# ---- argument checks of the package (before any geometry or device work) -----------------------------------------------------------
class _Fwd:
    final_shape = init_shape = (8, 8, 8)
    png_type = "fNL"
    evolution = "kaiser"


_FIXED = dict(Omega_m=0.3, sigma8=0.8, b1=1., b2=0., bs2=0., b3=0., bds2=0., bs3=0., bn2=0., bnpar=0., ngbars=1e-3, s_e=1., s_ed=0., s_e2=0.)


@pytest.mark.parametrize("lik_type", ["quad_gauss", "shash", "two_quad_gauss"])
def test_s_ep_with_the_kaiser_model_raises(lik_type):
    from montecosmo_amd import logdensity
    with pytest.raises(ValueError, match="s_ep"):
        logdensity.FieldLevelLogDensity(_Fwd(), np.zeros((8, 8, 8)), {"s_ep": {}}, _FIXED, lik_type=lik_type)
    with pytest.raises(ValueError, match="s_ep"):
        logdensity.FieldLevelLogDensity(_Fwd(), np.zeros((8, 8, 8)), {}, dict(_FIXED, s_ep=10.), lik_type=lik_type)


def test_two_quad_gauss_is_a_likelihood_and_needs_its_scalars():
    from montecosmo_amd import logdensity
    LD = logdensity.FieldLevelLogDensity
    assert LD.LIK_STOCH["two_quad_gauss"] == ("s_e", "s_ed", "s_e2") and "s_ep" in LD.ALL_STOCH
    assert LD.S_EP_LATENT == dict(loc=0., scale=1e5, loc_fid=0., scale_fid=1e2)      # model.py:248-253
    fixed = {k: v for k, v in _FIXED.items() if k != "s_e2"}
    with pytest.raises(ValueError, match="s_e2"):
        LD(_Fwd(), np.zeros((8, 8, 8)), {}, fixed, lik_type="two_quad_gauss")


def test_model_arguments_pass_two_quad_gauss_on():
    from montecosmo_amd import register
    rng = np.random.default_rng(5)
    reg = dict(cell_length=25., box_center=np.array([10., -20., 1500.]), box_rotvec=np.array([0.1, 0., -0.2]), init_oversamp=1.5,
               paint_oversamp=1.75, cosmo_fid=dict(Omega_m=0.3137721, sigma8=0.8076354), count_mesh=rng.poisson(3.0, (8, 6, 10)).astype(np.float64),
               a_obs=0.6, curved_sky=False, png_type="fNL")
    assert register.model_arguments(reg, lik_type="two_quad_gauss")["density"]["lik_type"] == "two_quad_gauss"
