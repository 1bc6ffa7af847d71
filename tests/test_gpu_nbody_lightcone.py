"""N-body evolution on the light cone (mcpm_nbody_lightcone_f32, mcpm_nbody_bf_lc_vjp_f32; nbody.nbody_bf with a per-particle a1,
FieldLevelForward(evolution='nbody', a_obs=None)) against the float64 restatement tests/_nbody_lc_f64.py."""
import numpy as np
import pytest

import _model_cases as C
import _nbody_lc_f64 as lc
from oracle import pm_oracle as o, background as obg

pytestmark = pytest.mark.gpu

K, A0, A_END = 4, 0.2, 0.8
LATTICES = [((16, 16, 16), (16, 16, 16)), ((16, 16, 16), (8, 8, 8)), ((12, 16, 20), (12, 16, 20)), ((12, 16, 20), (6, 8, 10))]
IDS = ["16c", "16c-ptcl8c", "12x16x20", "12x16x20-ptcl6x8x10"]


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    dt = np.complex128 if (np.iscomplexobj(a) or np.iscomplexobj(b)) else np.float64
    a, b = a.astype(dt), b.astype(dt)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def to_np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def nb(gpu):
    from montecosmo_amd import nbody
    return nbody


_CASES = {}


def case(nb, mesh, ptcl):
    """One run per lattice, shared and left unchanged: inputs, the library's forward state and context, the float64 step states."""
    key = (mesh, ptcl)
    if key in _CASES:
        return _CASES[key]
    from montecosmo_amd import bricks, synth
    rng = np.random.default_rng(17)
    spec = synth.init_mesh(mesh, seed=8, rms_disp=1.0)
    pos = bricks.regular_pos(mesh, ptcl)
    N = len(pos)
    a_p = rng.uniform(0.1, 0.95, N)
    cos_o, cos_g = obg.Planck18(), bricks.Planck18()
    (lp, vel), ctx = nb.nbody_bf(cos_g, spec, pos, a0=A0, a1=a_p, a_end=A_END, n_steps=K, return_ctx=True, lattice_out=True)
    traj, g0, dg = lc.run(cos_o, spec.astype(np.complex128), pos, A0, A_END, K)
    g_p = to_np(ctx.g_p).astype(np.float64)      # the growth factors the library selected with (float32 of a2g(a_p))
    assert np.abs(g_p - o.a2g(cos_o, a_p)).max() < 1e-7 and abs(g0 - ctx.lpt_s[0]) < 1e-9 and abs(dg - ctx.dg) < 1e-9      # the same run
    i, th, inside = lc.locate(g_p, float(ctx.lpt_s[0]), float(ctx.dg), K)      # with the host scalars the library selected with
    # on the host: every interval holds particles, and both clamps occur
    assert all((i == j).sum() > 0 for j in range(K)) and (g_p < g0).any() and (g_p > g0 + K * dg).any()
    xb, vb = rng.standard_normal((N, 3)).astype(np.float32), rng.standard_normal((N, 3)).astype(np.float32)
    _CASES[key] = dict(spec=spec, pos=pos, N=N, a_p=a_p, cos_o=cos_o, cos_g=cos_g, lp=lp, vel=vel, ctx=ctx, traj=traj, g0=g0, dg=dg,
                       g_p=g_p, sel=(i, th, inside), xb=xb, vb=vb, rng=rng)
    return _CASES[key]


@pytest.mark.parametrize("mesh,ptcl", LATTICES, ids=IDS)
def test_select_pass_against_f64_interpolation_of_the_same_checkpoints(nb, mesh, ptcl):
    """The select pass alone: float64 interpolation of the library's own float32 checkpoints.  Per component the kernel rounds the
    half-drift removal x' - v dg/2 (one fma, with dg/2 itself rounded to float32), theta and 1 - theta, two products and their sum: seven
    roundings of at most half an ulp of the largest operand each, so 4 ulp = 4 * 2^-23 of it bounds the difference (velocities: five)."""
    c = case(nb, mesh, ptcl)
    ctx, (i, th, _), N = c["ctx"], c["sel"], c["N"]
    hd = ctx.dg / 2
    X, V = [], []
    for j in range(K):
        x, v = (to_np(t).astype(np.float64) for t in ctx.state(j))
        X.append(x - v * hd)
        V.append(v)
    X.append(to_np(ctx.final[0]).astype(np.float64))
    V.append(to_np(ctx.final[1]).astype(np.float64))
    X, V, n, t = np.stack(X), np.stack(V), np.arange(N), th[:, None]
    want_x, want_v = (1 - t) * X[i, n] + t * X[i + 1, n], (1 - t) * V[i, n] + t * V[i + 1, n]
    mag_x = np.maximum(np.abs(X[i, n]) + np.abs(V[i, n]) * hd, np.abs(X[i + 1, n]) + np.abs(V[i + 1, n]) * hd)
    mag_v = np.maximum(np.abs(V[i, n]), np.abs(V[i + 1, n]))
    ex, ev = np.abs(to_np(c["lp"].disp) - want_x), np.abs(to_np(c["vel"]) - want_v)
    print(f"\nselect: worst |dx| / ulp(operand) {np.max(ex / (2.0 ** -23 * mag_x)):.2f}, |dv| {np.max(ev / (2.0 ** -23 * mag_v)):.2f} (bound 4)")
    assert np.all(ex <= 4 * 2.0 ** -23 * mag_x) and np.all(ev <= 4 * 2.0 ** -23 * mag_v)
    # the clamped particles carry a state bit for bit
    lo, hi = c["g_p"] < c["g0"], c["g_p"] > c["g0"] + K * c["dg"]
    assert np.array_equal(to_np(c["lp"].disp)[hi], to_np(ctx.final[0])[hi]) and np.array_equal(to_np(c["vel"])[hi], to_np(ctx.final[1])[hi])
    assert np.array_equal(to_np(c["vel"])[lo], to_np(ctx.state(0)[1])[lo])


@pytest.mark.parametrize("mesh,ptcl", LATTICES, ids=IDS)
def test_state_against_the_restatement(nb, mesh, ptcl):
    """The whole light-cone state against float64: the gate tests/test_gpu_parity.py::test_nbody_bf_edge_configurations applies to the
    fixed-time state on these meshes (2e-5 relative L2)."""
    c = case(nb, mesh, ptcl)
    p_o, v_o = lc.select(c["traj"], o.a2g(c["cos_o"], c["a_p"]), c["g0"], c["dg"])
    ex, ev = rel_l2(to_np(c["lp"].disp), p_o - c["pos"]), rel_l2(to_np(c["vel"]), v_o)
    print(f"\nlight-cone state: displacement {ex:.2e}, velocity {ev:.2e} (gate 2e-5)")
    assert ex < 2e-5 and ev < 2e-5
    # the default return structure: absolute positions with a leading axis of 1, as with a scalar a1
    p1, v1 = nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a0=A0, a1=c["a_p"].reshape(-1, 1), a_end=A_END, n_steps=K)
    assert tuple(p1.shape) == (1, c["N"], 3) and tuple(v1.shape) == (1, c["N"], 3)
    assert rel_l2(to_np(p1[0]) - c["pos"], p_o - c["pos"]) < 2e-5


@pytest.mark.parametrize("integrator", ["bullfrog", "fastpm"])
def test_all_particles_after_the_end_is_the_fixed_time_run_bit_for_bit(nb, integrator):
    c = case(nb, *LATTICES[0])
    kw = dict(a0=A0, n_steps=K, return_ctx=True, lattice_out=True, integrator=integrator)
    (lp0, v0), ctx0 = nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a1=A_END, **kw)
    (lp1, v1), ctx1 = nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a1=np.full(c["N"], 1.0), a_end=A_END, **kw)
    assert np.array_equal(to_np(lp0.disp), to_np(lp1.disp)) and np.array_equal(to_np(v0), to_np(v1))
    m0, s0 = nb.nbody_bf_vjp(ctx0, c["xb"], c["vb"])
    m1, s1 = nb.nbody_bf_vjp(ctx1, c["xb"], c["vb"])
    assert np.array_equal(to_np(m0), to_np(m1)) and not to_np(s1["g_lc"]).any()
    assert all(np.array_equal(s0[k], s1[k]) for k in s0), (s0, s1)


def test_refusals(nb):
    c = case(nb, *LATTICES[0])
    for kw in (dict(snapshots=3), dict(snapshots=[0.5]), dict(paint_deconv=True), dict(grad_fd=2), dict(lap_fd=4)):
        with pytest.raises(ValueError):
            nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a0=A0, a1=c["a_p"], a_end=A_END, n_steps=K, **kw)
    with pytest.raises(ValueError):
        nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a0=A0, a1=c["a_p"][:-1], a_end=A_END, n_steps=K)
    with pytest.raises(ValueError):
        nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a0=A0, a1=0.7, a_end=A_END, n_steps=K)


@pytest.mark.parametrize("mesh,ptcl,integrator", [(*LATTICES[0], "bullfrog"), (*LATTICES[1], "bullfrog"), (*LATTICES[2], "fastpm"),
                                                  (*LATTICES[3], "bullfrog")], ids=IDS)
def test_reverse_sweep_against_the_restatement(nb, mesh, ptcl, integrator):
    """Gates of tests/test_gpu_parity.py::test_nbody_bf_vjp for the same quantities: init_mesh_bar 1e-4 (relative L2 and along a random
    direction), alpha / beta rtol 2e-4 + 1e-3 of the largest, the growth scalars rtol 1e-3 + 1e-3 |g_bar|.  dg_bar and g_lc have no gate there:
    dg_bar takes the growth scalars' (the same kind of sum), g_lc the gate of init_mesh_bar."""
    c = case(nb, mesh, ptcl)
    alpha_fn = o.alpha_bf if integrator == "bullfrog" else o.alpha_fpm
    ctx = c["ctx"]
    if integrator != "bullfrog":
        _, ctx = nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a0=A0, a1=c["a_p"], a_end=A_END, n_steps=K, return_ctx=True, lattice_out=True,
                             integrator=integrator)
    mb_g, sb_g = nb.nbody_bf_vjp(ctx, c["xb"], c["vb"])
    mb_g, g_lc = to_np(mb_g), to_np(sb_g["g_lc"]).astype(np.float64)
    mb_o, sb_o, gb_o = lc.nbody_lc_vjp(c["cos_o"], c["spec"].astype(np.complex128), c["pos"], c["xb"].astype(np.float64),
                                       c["vb"].astype(np.float64), A0, None, A_END, K, alpha_fn=alpha_fn, g_p=c["g_p"])
    rng = np.random.default_rng(2)
    d = np.fft.rfftn(rng.standard_normal(mesh))
    dg_p = rng.standard_normal(c["N"])
    print(f"\ninit_mesh_bar {rel_l2(mb_g, mb_o):.2e}  g_lc {rel_l2(g_lc, gb_o):.2e}  "
          + "  ".join(f"{k} {sb_g[k]:.6g}/{sb_o[k]:.6g}" for k in ("g", "g2", "dg2dg", "dg")) + f"  theta terms {sb_o['g0_theta']:.4g} {sb_o['dg_theta']:.4g}")
    assert rel_l2(mb_g, mb_o) < 1e-4
    assert np.isclose(np.sum((np.conj(mb_g) * d).real), np.sum((np.conj(mb_o) * d).real), rtol=1e-4)
    assert np.allclose(sb_g["alpha"], sb_o["alpha"], rtol=2e-4, atol=1e-3 * np.abs(sb_o["alpha"]).max())
    assert np.allclose(sb_g["beta"], sb_o["beta"], rtol=2e-4, atol=1e-3 * np.abs(sb_o["beta"]).max())
    for k in ("g", "g2", "dg2dg", "dg"):
        assert np.isclose(sb_g[k], sb_o[k], rtol=1e-3, atol=1e-3 * abs(sb_o["g"])), k
    assert rel_l2(g_lc, gb_o) < 1e-4 and np.isclose((g_lc * dg_p).sum(), (gb_o * dg_p).sum(), rtol=1e-4, atol=1e-4 * np.linalg.norm(gb_o))
    assert not g_lc[~c["sel"][2]].any() and str(sb_g["g_lc"].dtype) == "torch.float32" and tuple(sb_g["g_lc"].shape) == (c["N"],)


@pytest.mark.parametrize("mesh,ptcl", [LATTICES[0], LATTICES[3]], ids=[IDS[0], IDS[3]])
def test_repeatable_independent_of_neighbours_and_of_the_pitch(nb, mesh, ptcl):
    c = case(nb, mesh, ptcl)
    N = c["N"]

    def run(a_p):
        (lp, vel), ctx = nb.nbody_bf(c["cos_g"], c["spec"], c["pos"], a0=A0, a1=a_p, a_end=A_END, n_steps=K, return_ctx=True, lattice_out=True)
        mb, sb = nb.nbody_bf_vjp(ctx, c["xb"], c["vb"])
        return dict(disp=to_np(lp.disp), vel=to_np(vel), mb=to_np(mb), g_lc=to_np(sb["g_lc"]),
                    **{k: np.asarray(sb[k]) for k in ("alpha", "beta", "g", "g2", "dg2dg", "dg")})

    first = run(c["a_p"])
    for _ in range(4):      # five calls in all
        again = run(c["a_p"])
        assert all(np.array_equal(first[k], again[k]) for k in first)
    # the same particles among OTHER scale factors: what one particle receives (state, cotangent of its g_p) depends on no neighbour's time
    other = c["a_p"].copy()
    other[1::2] = np.random.default_rng(3).uniform(0.1, 0.95, N)[1::2]
    mixed = run(other)
    for k in ("disp", "vel", "g_lc"):
        assert np.array_equal(first[k][0::2], mixed[k][0::2]), k
    assert not np.array_equal(first["disp"][1::2], mixed["disp"][1::2])
    # another pitch between the particle arrays of the checkpoint and of the running cotangents
    plan = nb.get_plan(mesh, ptcl)
    try:
        plan._pitch_probed = True
        plan.call("mcpm_plan_set_particle_pitch", 3 * N + 1088)
        pitched = run(c["a_p"])
    finally:
        plan.call("mcpm_plan_set_particle_pitch", 0)
    assert all(np.array_equal(first[k], pitched[k]) for k in first)


# ---- the model ------------------------------------------------------------------------------------------------------------------
BIAS = dict(b1=0.8, b2=0.2, bs2=-0.15, b3=0.1, bds2=0.1, bs3=-0.05, bn2=20.0, bnpar=5.0)
FWD = dict(final_shape=(8, 8, 8), cell_length=40., box_center=(60., -40., 1400.), box_rotvec=(0.1, 0.2, -0.1), evolution='nbody',
           nbody_n_steps=4, lpt_order=2, init_oversamp=1.5, evol_oversamp=2., paint_oversamp=2., a_obs=None, nbody_a_start=0.6)


def _intervals(cfg, cosmo):
    """Intervals of the run that the lattice's g_p fall in, from the host tables."""
    a, a_end = lc.lattice_a(cfg, cosmo)
    g0, g1 = float(o.a2g(cosmo, cfg["nbody_a_start"])), float(o.a2g(cosmo, a_end))
    return np.unique(lc.locate(o.a2g(cosmo, a.reshape(-1)), g0, (g1 - g0) / cfg["nbody_n_steps"], cfg["nbody_n_steps"])[0])


def _with_s8(c, s8):
    c.sigma8 = s8
    return c


@pytest.mark.parametrize("curved,ptcl", [(True, 2.), (False, 2.), (True, 1.5), (False, 1.5)])
def test_evolve_forward_and_vjp_on_the_light_cone(gpu, curved, ptcl):
    """tests/test_gpu_model.py::test_evolve_forward_and_vjp with evolution='nbody', a_obs=None and its gates: gxy 2e-4; white_mesh, b1, bs2,
    bnpar, sigma8 3e-3 and Omega_m 1e-2 against central differences of the restatement."""
    from montecosmo_amd import bricks, model
    rng = np.random.default_rng(31)
    fwd = model.FieldLevelForward(ptcl_oversamp=ptcl, curved_sky=curved, lin_kpow=C.kpow(), **FWD)
    cfg = fwd.config()
    assert cfg["init_shape"] == (12, 12, 12) and cfg["evol_shape"] == (16, 16, 16)
    cosmo, cosmo_o = bricks.Planck18(), obg.Planck18()
    cosmo_o.sigma8 = cosmo.sigma8
    assert len(_intervals(cfg, cosmo_o)) >= 3
    white = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * (12 ** 3 / np.prod(cfg["box_size"])) ** .5
    gxy, ctx = fwd.evolve(cosmo, BIAS, white.astype(np.complex64), return_ctx=True)
    ref, aux = lc.evolve(cfg, cosmo_o, BIAS, white)
    assert gxy.shape == (16, 16, 16)
    print(f"\ngxy {rel_l2(gxy.cpu().numpy(), ref):.2e} (gate 2e-4)")
    assert rel_l2(gxy.cpu().numpy(), ref) < 2e-4
    gb = rng.standard_normal((16, 16, 16))
    grads = fwd.evolve_vjp(ctx, gb.astype(np.float32))
    L = lambda wh, bias_, s8: float((gb * lc.evolve(cfg, _with_s8(cosmo_o, s8), bias_, wh)[0]).sum())
    eps = 1e-5
    dW = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * np.abs(white).mean() / 40.
    fd = (L(white + eps * dW, BIAS, cosmo.sigma8) - L(white - eps * dW, BIAS, cosmo.sigma8)) / (2 * eps)
    an = float(np.sum(np.conj(grads["white_mesh"].cpu().numpy().astype(np.complex128)) * dW).real)
    print(f"white_mesh fd {fd:.6g} got {an:.6g}")
    assert abs(fd - an) < 3e-3 * abs(fd), ("white_mesh", fd, an)
    for k in ("b1", "bs2", "bnpar"):
        h = 1e-4 * max(1.0, abs(BIAS[k]))
        fdk = (L(white, dict(BIAS, **{k: BIAS[k] + h}), cosmo.sigma8) - L(white, dict(BIAS, **{k: BIAS[k] - h}), cosmo.sigma8)) / (2 * h)
        print(f"{k} fd {fdk:.6g} got {grads['bias'][k]:.6g}")
        assert abs(fdk - grads["bias"][k]) < 3e-3 * max(abs(fdk), 1e-3 * abs(fd)), (k, fdk, grads["bias"][k])
    h = 1e-4
    fds = (L(white, BIAS, cosmo.sigma8 + h) - L(white, BIAS, cosmo.sigma8 - h)) / (2 * h)
    print(f"sigma8 fd {fds:.6g} got {grads['sigma8']:.6g}")
    assert abs(fds - grads["sigma8"]) < 3e-3 * abs(fds), ("sigma8", fds, grads["sigma8"])
    got = fwd.cosmo_vjp(ctx, grads, params=("Omega_m",))["Omega_m"]

    def L_om(dom):
        cc = obg.Planck18(Omega_c=cosmo.Omega_c + dom)
        cc.sigma8 = cosmo.sigma8
        return float((gb * lc.evolve(cfg, cc, BIAS, white)[0]).sum())
    fdo = (L_om(h) - L_om(-h)) / (2 * h)
    print(f"Omega_m fd {fdo:.6g} got {got:.6g}")
    assert abs(fdo - got) < 1e-2 * abs(fdo), ("Omega_m", fdo, got)


def test_log_density_and_gradient_on_the_light_cone(gpu):
    """FieldLevelLogDensity with evolution='nbody' on the light cone: precond='kaiser', Omega_m, sigma8, b1, b2 sampled, a selection mesh, a
    mask and two shells, png_type='fNL'; the gates of tests/test_gpu_model.py::test_log_density_and_gradient, the steps of tests/_model_cases.py."""
    import torch
    from montecosmo_amd import logdensity, model
    rng = np.random.default_rng(41)
    fwd = model.FieldLevelForward(ptcl_oversamp=2., curved_sky=True, lin_kpow=C.kpow(), png_type='fNL', **FWD)
    cfg = dict(fwd.config(), final_shape=(8, 8, 8), cell_length=40., precond="kaiser")
    g = np.indices(fwd.paint_shape).astype(float)
    extra = dict(selec_mesh=0.7 + 0.3 * np.cos(2 * np.pi * g[0] / 16) * np.sin(2 * np.pi * g[2] / 16) + 0.1 * rng.uniform(size=fwd.paint_shape),
                 mask_mesh=rng.uniform(size=(8, 8, 8)) < 0.8)
    cfg.update(extra)
    lat = {"Omega_m": dict(loc=0.3111, scale=0.1, loc_fid=0.3111, scale_fid=1e-2, low=0.05, high=1.), "sigma8": C.TN(0.8102, 1e-2),
           "b1": C.N(1., 1e-2), "b2": C.N(0., 3e-2)}
    fixed = dict(bs2=-0.15, bn2=20., bnpar=5., b3=0.1, bds2=0.1, bs3=-0.05, ngbars=np.array([1e-3, 1.4e-3]), s_e=1.0, s_ed=0.3, s_e2=0.03,
                 fNL=200., fNL_bpd2=-20., fNL_bps2=30., fNL_bn2p=2.0e3)
    sample = {k + "_": float(rng.normal(0, 1.0)) for k in lat}
    sample["white_mesh_"] = rng.standard_normal((12, 12, 12))
    assert len(_intervals(cfg, C.make_cosmo(dict(Omega_m=0.3111, sigma8=0.81)))) >= 3
    ref = lambda s, obs_, info=None: lc.log_density(cfg, lat, fixed, s, obs_, C.make_cosmo, png_type='fNL', info=info)
    truth = dict(sample, white_mesh_=0.98 * sample["white_mesh_"] + 0.2 * rng.standard_normal((12, 12, 12)))
    info = {}
    ref(truth, np.zeros((8, 8, 8)), info=info)
    cm = info["count"]
    obs = cm + np.sqrt(np.abs(cm)) * rng.standard_normal((8, 8, 8))
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="kaiser", **extra)
    s32 = {k: (v if np.ndim(v) == 0 else v.astype(np.float32)) for k, v in sample.items()}
    lp, grad = ld.logdensity_and_grad(s32)
    lp2, grad2 = ld.logdensity_and_grad(s32)
    same = lambda a, b: torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b)
    assert lp == lp2 and set(grad) == set(grad2) and all(same(grad[k], grad2[k]) for k in grad)      # bitwise repeatable, scalars included
    lp_o = ref(sample, obs)
    print(f"\nlp {lp:.6f} float64 {lp_o:.6f}")
    assert np.isfinite(lp_o) and abs(lp - lp_o) < 2e-4 * abs(lp_o) + 0.05, (lp, lp_o)
    steps = dict(Omega_m=1e-3, sigma8=1e-3, b1=1e-4, b2=1e-4)
    for k in lat:
        h = steps[k]
        fd = (ref(dict(sample, **{k + "_": sample[k + "_"] + h}), obs) - ref(dict(sample, **{k + "_": sample[k + "_"] - h}), obs)) / (2 * h)
        print(f"  {k}: fd {fd:.6f} got {float(grad[k + '_']):.6f}")
        assert abs(fd - grad[k + "_"]) < 1e-2 * abs(fd) + 1e-3, (k, fd, grad[k + "_"])
    d, h = rng.standard_normal((12, 12, 12)), 3e-5
    fd = (ref(dict(sample, white_mesh_=sample["white_mesh_"] + h * d), obs) - ref(dict(sample, white_mesh_=sample["white_mesh_"] - h * d), obs)) / (2 * h)
    gw = grad["white_mesh_"].double().cpu().numpy()
    an = float((gw * d).sum())
    typical = np.linalg.norm(gw) * np.linalg.norm(d) / np.sqrt(d.size)
    print(f"  white_mesh_: fd {fd:.6f} got {an:.6f} typical {typical:.4f}")
    assert abs(fd - an) < 5e-3 * max(abs(fd), typical), ("white_mesh_", fd, an, typical)
