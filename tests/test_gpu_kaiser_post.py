"""GPU checks of the chain start: `FieldLevelLogDensity.kaiser_post` / `sample_params` / `count2delta` / `condition` and
`bricks.kaiser_posterior` (mcpm_kaiser_post_c64) against the float64 restatement tests/_kaiser_post_f64.py, which
tests/test_kaiser_post_host.py pins.  Gate of the forward outputs: 1e-5 relative L2, the project's float32 gate."""
import math

import numpy as np
import pytest

import _kaiser_post_f64 as kp
from oracle import background as obg, bias_oracle as bo, pm_oracle as o

pytestmark = pytest.mark.gpu

GATE = 1e-5
BIAS0 = dict(b2=0., bs2=0., bn2=0., bnpar=0., b3=0., bds2=0., bs3=0.)


def _kpow(init_shape, box_size):
    """A power table that ends at 0.8 of the corner |k| of the init mesh: modes with P = 0 besides k = 0, whatever the mesh."""
    corner = float(np.sqrt(sum((np.pi * n / b) ** 2 for n, b in zip(init_shape, box_size))))
    ks = np.logspace(-3, np.log10(0.8 * corner), 128)
    return ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6)


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _np(t):
    t = t.cpu().numpy()
    return t.astype(np.complex128 if np.iscomplexobj(t) else np.float64)


def _make_cosmo(base):
    return obg.Planck18(Omega_c=base["Omega_m"] - obg.Planck18().Omega_b, sigma8=base["sigma8"])


def _survey(final_shape, oversamp, precond, seed=3):
    """The hard case: oblique box centre, rotated box, a selection mesh, a spherical-cap mask, fixed per-shell ngbars."""
    from montecosmo_amd import model, logdensity
    rng = np.random.default_rng(seed)
    init_shape = tuple(int(2 * np.rint(n * oversamp / 2)) for n in final_shape)
    KPOW = _kpow(init_shape, np.multiply(final_shape, 40.))
    fwd = model.FieldLevelForward(final_shape=final_shape, cell_length=40., box_center=(300., -200., 1500.), box_rotvec=(0.1, 0.2, -0.1),
                                  evolution="lpt", init_oversamp=oversamp, evol_oversamp=oversamp, ptcl_oversamp=oversamp,
                                  paint_oversamp=2. if oversamp != 1 else 1., a_obs=0.65, curved_sky=True, lin_kpow=KPOW)
    g = np.indices(fwd.paint_shape).astype(float)
    selec = 0.7 + 0.3 * np.cos(2 * np.pi * g[0] / fwd.paint_shape[0]) * np.sin(2 * np.pi * g[2] / fwd.paint_shape[2]) \
        + 0.1 * rng.uniform(size=fwd.paint_shape)
    pos = bo.cell2phys_pos(o.regular_pos(fwd.final_shape), fwd.box_center, bo.rotvec_matrix(fwd.box_rotvec), fwd.box_size, fwd.final_shape)
    cosang = (pos @ (fwd.box_center / np.linalg.norm(fwd.box_center))) / np.linalg.norm(pos, axis=-1)
    mask = (cosang > np.quantile(cosang, 0.3)).reshape(fwd.final_shape)      # a cap about the box centre's direction: 70 % of the cells
    lat = {"sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2, low=0., high=np.inf),
           "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2), "s_e": dict(loc=1., scale=10., loc_fid=1., scale_fid=1e-2)}
    fixed = dict(BIAS0, Omega_m=0.3111, b2=0.2, ngbars=np.array([1e-4, 1.4e-4]), s_ed=0., s_e2=0.)
    obs = np.where(mask, rng.poisson(8., fwd.final_shape), 0).astype(np.float64)
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond=precond, selec_mesh=selec, mask_mesh=mask)
    cfg = dict(fwd.config(), final_shape=fwd.final_shape, cell_length=fwd.cell_length, precond=precond, selec_mesh=selec, mask_mesh=mask)
    assert fwd.init_shape == init_shape
    return dict(fwd=fwd, ld=ld, cfg=cfg, lat=lat, fixed=fixed, obs=obs, rng=rng, kpow=KPOW)


@pytest.mark.parametrize("final_shape,oversamp,precond", [((8, 8, 8), 1.5, "kaiser"), ((16, 12, 8), 1., "fourier"), ((10, 6, 14), 1., "real")])
def test_parity_with_the_restatement(gpu, final_shape, oversamp, precond):
    s = _survey(final_shape, oversamp, precond)
    ld, fwd, cfg, KPOW = s["ld"], s["fwd"], s["cfg"], s["kpow"]
    if final_shape == (8, 8, 8):
        assert fwd.init_shape == (12, 12, 12) and fwd.paint_shape != fwd.final_shape
    nc, temp, sf = 3, 0.5, 7 / 8
    noise = s["rng"].standard_normal((nc,) + fwd.init_shape)
    got_b = ld.kaiser_post(0, base=True, temp=temp, scale_field=sf, n_chains=nc, noise=noise.astype(np.float32))
    got_s = ld.kaiser_post(0, base=False, temp=temp, scale_field=sf, n_chains=nc, noise=noise.astype(np.float32))
    assert set(got_b) == {"sigma8", "b1", "s_e", "white_mesh"} and set(got_s) == set(ld.names())
    pmesh = bo.lin_power_mesh(0.8102, fwd.init_shape, fwd.box_size, KPOW)
    assert (pmesh == 0).sum() > 1
    # the observed contrast first: what everything else is made from
    d_got, d_want = _np(ld.count2delta()), kp.observed_delta(cfg, s["obs"])
    print(f"\n{final_shape} {precond}: count2delta rel L2 {rel_l2(d_got, d_want):.2e}")
    assert rel_l2(d_got, d_want) < GATE
    for b in range(nc):
        want_b = kp.kaiser_post(cfg, s["lat"], s["fixed"], s["obs"], noise[b].astype(np.float32), _make_cosmo, temp=temp, scale_field=sf, base=True)
        want_s = kp.kaiser_post(cfg, s["lat"], s["fixed"], s["obs"], noise[b].astype(np.float32), _make_cosmo, temp=temp, scale_field=sf)
        wb, ws = _np(got_b["white_mesh"][b]), _np(got_s["white_mesh_"][b])
        eb, es = rel_l2(wb, want_b["white_mesh"]), rel_l2(ws, want_s["white_mesh_"])
        print(f"  chain {b}: white_mesh rel L2 {eb:.2e}, white_mesh_ rel L2 {es:.2e}")
        assert eb < GATE and es < GATE
        assert np.all(wb[pmesh == 0] == 0)      # exactly
        for k in s["lat"]:
            assert got_b[k].shape == (nc,) and got_b[k][b] == want_b[k]
            assert abs(got_s[k + "_"][b] - want_s[k + "_"]) < 1e-9
    # the posterior moments alone, on the restatement's own delta_obs
    from montecosmo_amd import bricks
    means64, stds64, fid, cosmo64 = kp.posterior_moments(cfg, s["lat"], s["fixed"], s["obs"], _make_cosmo)
    delta_obs = o.chreshape(o._rfftn(d_want), o.r2chshape(fwd.init_shape))
    k = ld._kaiser_fiducial()
    means, stds = bricks.kaiser_posterior(delta_obs.astype(np.complex64), k.cosmo, k.a, fwd.box_size, k.var_noise, k.b1E, los=k.los, kpow=KPOW)
    print(f"  means rel L2 {rel_l2(_np(means), means64):.2e}, stds rel L2 {rel_l2(_np(stds), stds64):.2e}")
    assert rel_l2(_np(means), means64) < GATE and rel_l2(_np(stds), stds64) < GATE
    assert np.all(_np(stds)[pmesh == 0] == 0) and np.all(_np(means)[pmesh == 0] == 0)
    # lin2white against its restatement, zeros included
    x = o.rg2cgh(noise[0])
    lw = _np(bricks.lin2white(k.cosmo, x.astype(np.complex64), fwd.init_shape, fwd.box_size, kpow=KPOW))
    assert rel_l2(lw, kp.lin2white(0.8102, x, fwd.init_shape, fwd.box_size, KPOW)) < GATE and np.all(lw[pmesh == 0] == 0)


def test_bitwise(gpu):
    import torch
    s = _survey((8, 8, 8), 1.5, "kaiser")
    ld = s["ld"]
    a = ld.kaiser_post(7, temp=0.5, scale_field=7 / 8, n_chains=3)
    b = ld.kaiser_post(7, temp=0.5, scale_field=7 / 8, n_chains=3)
    c = ld.kaiser_post(8, temp=0.5, scale_field=7 / 8, n_chains=3)
    assert torch.equal(a["white_mesh_"], b["white_mesh_"]) and not torch.equal(a["white_mesh_"], c["white_mesh_"])
    assert a["white_mesh_"].shape == (3,) + ld.fwd.init_shape and np.array_equal(a["sigma8_"], b["sigma8_"])
    noise = torch.randn((3,) + ld.fwd.init_shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    all3 = ld.kaiser_post(0, base=True, temp=0.5, n_chains=3, noise=noise)
    for i in range(3):
        one = ld.kaiser_post(0, base=True, temp=0.5, noise=noise[i])
        assert one["white_mesh"].shape == all3["white_mesh"].shape[1:] and torch.equal(one["white_mesh"], all3["white_mesh"][i])
        assert isinstance(one["sigma8"], float)


# ---- exactness on the device: the configuration of tests/test_kaiser_post_host.py on the HIP log density -----------------------------------
def test_device_mean_is_the_peak_of_the_hip_log_density(gpu):
    """m = kaiser_post(temp = 0) against the float64 restatement's mean cast to float32, both fed to the same HIP log density: |grad lp(m)| is
    no more than 10x the restatement's (both are round-off: hence the factor), and both are <= 1e-3 |grad lp(0)| (three orders above float32
    cancellation error; this only keeps two bad means from passing).  The same for lp(m + z) - lp(m) + |z|^2 / 2 against |z|^2 / 2."""
    import torch
    import test_kaiser_post_host as H
    from montecosmo_amd import model, logdensity
    fwd = model.FieldLevelForward(final_shape=H.SHAPE, cell_length=H.CELL, box_center=(0., 0., 1500.), evolution="kaiser", init_oversamp=1.,
                                  evol_oversamp=1., ptcl_oversamp=1., paint_oversamp=1., a_obs=0.7, curved_sky=False, lin_kpow=H.KPOW)
    obs, _ = H._observation()
    ld = logdensity.FieldLevelLogDensity(fwd, obs, {}, dict(BIAS0, **H.FIXED), precond="kaiser", make_cosmo=H._make_cosmo)
    m = ld.kaiser_post(0, temp=0.)["white_mesh_"]
    m64 = torch.from_numpy(H._restated_mean("kaiser", obs).astype(np.float32)).cuda()
    print(f"\nmean: device vs restatement rel L2 {rel_l2(_np(m), _np(m64)):.2e}")
    gnorm = lambda w: float(torch.linalg.vector_norm(ld.logdensity_and_grad({"white_mesh_": w})[1]["white_mesh_"].double()))
    g0, gm, gm64 = gnorm(torch.zeros_like(m)), gnorm(m), gnorm(m64)
    print(f"|grad(m)| / |grad(0)|: device mean {gm / g0:.3e}, restated mean {gm64 / g0:.3e}")
    assert gm <= 10 * gm64 and gm <= 1e-3 * g0 and gm64 <= 1e-3 * g0
    z = torch.randn(H.SHAPE, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    half = 0.5 * float((z.double() ** 2).sum())
    quad = lambda w: abs(ld({"white_mesh_": w + z}) - ld({"white_mesh_": w}) + half)
    qm, qm64 = quad(m), quad(m64)
    print(f"|lp(m + z) - lp(m) + |z|^2 / 2| / (|z|^2 / 2): device mean {qm / half:.3e}, restated mean {qm64 / half:.3e}")
    assert qm <= 10 * qm64 and qm <= 1e-3 * half and qm64 <= 1e-3 * half


# ---- conditioning -----------------------------------------------------------------------------------------------------------------------
def test_conditioning_on_every_scalar(gpu):
    import torch
    from montecosmo_amd import logdensity, samplers
    s = _survey((8, 8, 8), 1.5, "kaiser")
    ld, rng = s["ld"], s["rng"]
    sample = {k + "_": float(rng.normal(0, 1.0)) for k in s["lat"]}
    sample["white_mesh_"] = torch.from_numpy((rng.standard_normal(ld.fwd.init_shape) * _np(ld.scale)).astype(np.float32)).cuda()
    v = {k: ld.base_params(sample)[k] for k in s["lat"]}
    cond = ld.condition(v)
    assert cond.names() == ["white_mesh_"] and set(ld.names()) == {"sigma8_", "b1_", "s_e_", "white_mesh_"}      # the original is untouched
    assert cond.transfer is ld.transfer and cond.scale is ld.scale and cond.count_obs is ld.count_obs
    back = ld.sample_params(v)
    prior = sum(logdensity.latent_log_prob_and_grad(back[k + "_"], ld.latents[k])[0] for k in s["lat"])
    lp_c, g_c = cond.logdensity_and_grad({"white_mesh_": sample["white_mesh_"]})
    lp_j, g_j = ld.logdensity_and_grad(sample)
    print(f"\nconditioned {lp_c:.6f} + priors {prior:.6f} vs joint {lp_j:.6f}; field gradient rel L2 "
          f"{rel_l2(_np(g_c['white_mesh_']), _np(g_j['white_mesh_'])):.2e}")
    assert math.isfinite(lp_j) and abs(lp_c + prior - lp_j) <= 1e-6 * abs(lp_j)
    assert set(g_c) == {"white_mesh_"} and rel_l2(_np(g_c["white_mesh_"]), _np(g_j["white_mesh_"])) <= 1e-6
    flat = samplers.FlatLogDensity(cond)
    q = flat.pack({"white_mesh_": sample["white_mesh_"]})
    assert flat.ns == 0 and q.numel() == int(np.prod(ld.fwd.init_shape))
    lp_f, g_f = flat(q)
    assert lp_f == lp_c and g_f.shape == q.shape
    with pytest.raises(ValueError):
        ld.condition({"Omega_m": 0.3})      # fixed already: not a latent


# ---- it is a better start ---------------------------------------------------------------------------------------------------------------
def test_kaiser_post_is_a_better_start(gpu):
    """lpt at (16, 16, 16), 8 galaxies per cell: lp at the Kaiser posterior draw (scale_field = 7/8) exceeds lp at the zero field and at the
    tools' 0.3 randn prior_std start, scalars at fiducial in all three.  Float64 composition (oracle + this file's restatement) for this
    seed: see profiles/kaiser_post.txt."""
    import torch
    from montecosmo_amd import model, logdensity, utils
    ks = np.logspace(-3, 1, 128)
    kpow = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))
    fwd = model.FieldLevelForward(final_shape=(16, 16, 16), cell_length=20., box_center=(0., 0., 2000.), evolution="lpt", a_obs=0.7, lin_kpow=kpow)
    lat = {"sigma8": dict(loc=0.8102, scale=0.03, loc_fid=0.8102, scale_fid=1e-2, low=0., high=np.inf),
           "b1": dict(loc=1., scale=0.03, loc_fid=1., scale_fid=1e-2), "b2": dict(loc=0., scale=0.09, loc_fid=0., scale_fid=3e-2)}
    fixed = dict(BIAS0, Omega_m=0.3111, ngbars=8. / 20. ** 3, s_e=1.0, s_ed=0., s_e2=0.)
    fixed.pop("b2")
    ld0 = logdensity.FieldLevelLogDensity(fwd, torch.zeros(fwd.final_shape), lat, fixed, precond="kaiser")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rng = np.random.default_rng(0)
    truth = {k + "_": float(rng.normal(0., c["scale"] / c["scale_fid"])) for k, c in lat.items()}      # a prior draw
    truth["white_mesh_"] = torch.randn(fwd.init_shape, device="cuda", generator=gen) * ld0.scale
    obs = ld0.draw_counts(truth, seed=1)
    print(f"\nmean count per cell {float(obs.mean()):.2f}")
    assert 6. < float(obs.mean()) < 10.
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="kaiser")
    start = ld.kaiser_post(3, scale_field=7 / 8)
    fid = {k + "_": 0.0 for k in lat}
    assert all(abs(start[k]) < 1e-9 for k in fid)
    g = torch.Generator(device="cuda").manual_seed(100)
    lp_k = ld(start)
    lp_0 = ld(dict(fid, white_mesh_=torch.zeros(fwd.init_shape, device="cuda")))
    lp_p = ld(dict(fid, white_mesh_=0.3 * torch.randn(fwd.init_shape, device="cuda", generator=g) * ld.scale))
    print(f"lp: kaiser_post {lp_k:.1f}, zero field {lp_0:.1f}, 0.3 randn prior_std {lp_p:.1f}, truth {ld(truth):.1f}")
    assert lp_k > lp_0 and lp_k > lp_p
    # the batched start against the truth: coherence of the white fields (recorded, not gated)
    batch = ld.kaiser_post(3, base=True, scale_field=7 / 8, n_chains=2)["white_mesh"]
    truth_white = utils.rg2cgh(truth["white_mesh_"]) * ld.transfer
    k, pow1, trans, coh = fwd.powtranscoh(truth_white, batch)
    print(f"lowest bin k = {np.ravel(k)[0]:.4f}: coherence {coh[:, 0]}, transfer {trans[:, 0]}")
    assert coh.shape[0] == 2 and np.all(np.isfinite(coh[:, 0]))
