"""The fused isokinetic integrator kernels (csrc/mclmc.hip) against the float64 restatement `_mclmc_f64`, and the preconditioned MCLMC / MAMS
samplers on them: one transition against the 'torch' back end, short chains over the HIP log density of an 8^3 model."""
import math

import numpy as np
import pytest

import _mclmc_f64 as ref
from oracle import bias_oracle as bo, background as obg  # checker only

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 63, 64, 65, 1025, 65537, 1000003, 2 ** 22 + 3)
# Tolerance of u' and q', per unit of the largest operand (|u'| for u'; the larger of |q| and |eps_drift s u'| for q').  On the host the same
# expressions (gt = s g; u' = ca gt + cb u; q' = q + eps_drift (s u')) were evaluated in numpy float32, with ca and cb rounded to float32,
# against float64 from the same float32 inputs, at every size of SIZES and every variant of `_case`: the largest absolute error over the
# largest operand was 9.78e-8 (u') and 6.79e-8 (q', against the drift of the rounded u').  Four times the larger of the two, 3.91e-7, is
# allowed, because the device fuses multiply-adds differently.  (The kernel forms both in float64 and rounds once, so it sits well inside.)
HOST_F32_ERROR = 9.78e-8
TOL = 4 * HOST_F32_ERROR
DELTA = 0.3      # eps_kick gamma / (d - 1) of the cases: dK = (d - 1)(delta - ln 2 + ln D) ~ (d - 1) c delta, far from the cancellation at delta -> 0


def _case(d, with_s, unit, seed=0, delta=DELTA, zero_g=False):
    """float32 inputs of one kick: u (unit, or 2.5 times that), g correlated with u (c about 0.3, so that sum u gt is no small difference of
    large terms), s in [0.5, 2), q, and the eps_kick that makes delta what is asked."""
    rng = np.random.default_rng(1000 * seed + d % 997 + 2 * with_s + unit)
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    g = np.zeros(d) if zero_g else 4. * (0.3 * math.sqrt(d) * u + rng.standard_normal(d))
    u = (u if unit else 2.5 * u).astype(np.float32)
    g = g.astype(np.float32)
    s = rng.uniform(0.5, 2., d).astype(np.float32) if with_s else None
    q = (3. * rng.standard_normal(d)).astype(np.float32)
    gg = ref.sums(u, g, s)[0]
    eps_kick = delta * (d - 1) / math.sqrt(gg) if gg > 0 else 0.5
    return u, q, g, s, eps_kick, 0.37


def _dev(x, offset=False):
    import torch
    if x is None:
        return None
    if not offset:
        return torch.from_numpy(x).cuda()
    buf = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda()
    return buf[1:]      # contiguous, 4 bytes past a 16-byte boundary


def _plan():
    from montecosmo_amd import nbody
    return nbody.get_plan((8, 8, 8))


def _run_kernel(u, q, g, s, eps_kick, eps_drift, offset=False, dK0=0.25):
    import torch
    ud, qd, gd, sd = _dev(u, offset), _dev(q, offset), _dev(g, offset), _dev(s, offset)
    stats = torch.tensor([7., 7., 7., dK0], dtype=torch.float64, device="cuda")
    _plan().call("mcpm_mclmc_kick_drift_f32", ud, qd, gd, sd, u.size, float(eps_kick), float(eps_drift), stats)
    return ud.cpu().numpy(), None if qd is None else qd.cpu().numpy(), stats.cpu().numpy()


def _check(got, u, q, g, s, eps_kick, eps_drift, want=None, dK0=0.25):
    un, qn, stats = got
    u_ref, q_ref, dK, st = want if want is not None else ref.kick_drift(u, q, g, eps_kick, eps_drift, s)
    for a, b in zip(stats[:3], st):
        assert abs(a - b) <= 1e-12 * abs(b), (stats, st)
    assert abs((stats[3] - dK0) - dK) <= 1e-12 * abs(dK) + 1e-15 * abs(dK0), (stats[3] - dK0, dK)      # (added to what was there)
    assert np.abs(un - u_ref).max() <= TOL * np.abs(u_ref).max()
    assert abs(np.linalg.norm(un.astype(np.float64)) - 1.) < 1e-6
    if q is not None:
        sv = 1. if s is None else s.astype(np.float64)
        scale = max(np.abs(q).max(), np.abs(eps_drift * sv * u_ref).max())
        assert np.abs(qn - q_ref).max() <= TOL * scale
    else:
        assert qn is None


@pytest.mark.parametrize("d", SIZES)
def test_kick_drift_against_float64(gpu, d):
    """Every size (one lane, the wave edge, the block edge, ragged tails, more than one grid stride), with and without s, with and
    without q, unit and un-normalised u.  The reference of a (d, s, u) is computed once and serves both q variants.  The sums and dK are
    held to a relative 1e-12; u' and q' to TOL = 3.91e-7 of the largest operand, four times the 9.78e-8 that a float32 evaluation of the same
    expressions loses on the host (see TOL above); |u'| to 1e-6 of 1."""
    for with_s in (False, True):
        for unit in (True, False):
            u, q, g, s, ek, ed = _case(d, with_s, unit)
            want = ref.kick_drift(u, q, g, ek, ed, s)
            _check(_run_kernel(u, q, g, s, ek, ed), u, q, g, s, ek, ed, want)
            _check(_run_kernel(u, None, g, s, ek, ed), u, None, g, s, ek, ed, (want[0], None) + want[2:])


@pytest.mark.parametrize("d", [3, 65, 1000003])
def test_kick_drift_with_every_pointer_offset_by_one_float(gpu, d):
    u, q, g, s, ek, ed = _case(d, True, False, seed=1)
    got = _run_kernel(u, q, g, s, ek, ed, offset=True)
    _check(got, u, q, g, s, ek, ed)
    aligned = _run_kernel(u, q, g, s, ek, ed)
    assert np.array_equal(got[0], aligned[0]) and np.array_equal(got[1], aligned[1])      # elementwise work is the same on both paths


def test_kick_drift_zero_force_and_huge_delta(gpu):
    d = 1025
    u, q, g, s, ek, ed = _case(d, True, False, seed=2, zero_g=True)
    un, qn, stats = _run_kernel(u, q, g, s, ek, ed)
    _check((un, qn, stats), u, q, g, s, ek, ed)
    assert stats[0] == 0. and stats[3] == 0.25      # dK = 0
    assert np.abs(un - u / np.linalg.norm(u.astype(np.float64))).max() <= TOL * np.abs(un).max()
    u, q, g, s, ek, ed = _case(d, True, True, seed=3, delta=200.)      # |s g| eps / (d - 1) = 200
    got = _run_kernel(u, q, g, s, ek, ed)
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    _check(got, u, q, g, s, ek, ed)


@pytest.mark.parametrize("d", [65, 1000003])
def test_moments_against_float64(gpu, d):
    import torch
    rng = np.random.default_rng(d)
    q = rng.standard_normal(d).astype(np.float32)
    xa, x2a = rng.standard_normal(d), rng.uniform(0., 2., d)
    xd, x2d = torch.from_numpy(xa).cuda(), torch.from_numpy(x2a).cuda()
    _plan().call("mcpm_mclmc_moments_f64", torch.from_numpy(q).cuda(), d, 0.9867, 0.73, xd, x2d)
    xr, x2r = ref.moments(q, 0.9867, 0.73, xa, x2a)
    assert np.abs(xd.cpu().numpy() - xr).max() <= 1e-14 * np.abs(xr).max()
    assert np.all(np.abs(xd.cpu().numpy() - xr) <= 1e-14 * np.abs(xr)) and np.all(np.abs(x2d.cpu().numpy() - x2r) <= 1e-14 * np.abs(x2r))
    # offset q (the scalar path) gives the same
    xo, x2o = torch.from_numpy(xa).cuda(), torch.from_numpy(x2a).cuda()
    _plan().call("mcpm_mclmc_moments_f64", _dev(q, offset=True), d, 0.9867, 0.73, xo, x2o)
    assert torch.equal(xo, xd) and torch.equal(x2o, x2d)


def test_kick_drift_repeats_bitwise(gpu):
    for d in (65537, 2 ** 22 + 3):
        u, q, g, s, ek, ed = _case(d, True, False, seed=4)
        a, b = _run_kernel(u, q, g, s, ek, ed), _run_kernel(u, q, g, s, ek, ed)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_argument_errors(gpu):
    import torch
    from montecosmo_amd._lib import McpmError
    x = torch.ones(8, device="cuda")
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    keep = x.clone()
    with pytest.raises(McpmError):
        _plan().call("mcpm_mclmc_kick_drift_f32", x, None, x.clone(), None, 1, 0.1, 0.1, stats)      # d = 1
    with pytest.raises(McpmError):
        _plan().call("mcpm_mclmc_kick_drift_f32", x, None, None, None, 8, 0.1, 0.1, stats)           # no gradient
    with pytest.raises(McpmError):
        _plan().call("mcpm_mclmc_kick_drift_f32", x, None, x.clone(), None, 8, 0.1, 0.1, None)       # no stats
    with pytest.raises(McpmError):
        _plan().call("mcpm_mclmc_moments_f64", x, 8, 0.9, 1., None, stats)
    assert torch.equal(x, keep) and float(stats.abs().sum()) == 0.      # nothing was launched


def _device_gauss(sd):
    def logdf(q):
        r = q.double() / sd
        return float(-0.5 * (r * r).sum()), (-(q.double() / (sd * sd))).float()
    return logdf


def test_one_transition_hip_against_torch(gpu):
    """The same state, z and s on a device Gaussian: one MCLMC transition through each back end."""
    import torch
    from montecosmo_amd import samplers
    d = 65537
    rng = np.random.default_rng(9)
    sd = torch.from_numpy(np.exp(rng.uniform(-1., 1., d))).cuda()
    logdf = _device_gauss(sd)
    q0 = (sd * torch.from_numpy(rng.standard_normal(d)).cuda()).float()
    u0 = torch.from_numpy(rng.standard_normal(d)).cuda().float()
    u0 /= torch.linalg.vector_norm(u0)
    inverse_mass = (sd * sd).float() * torch.from_numpy(rng.uniform(0.7, 1.4, d)).cuda().float()
    lp, g = logdf(q0)
    out = {}
    for backend in ("torch", "hip"):
        integ = samplers.make_integrator(q0, inverse_mass, backend)
        assert integ.backend == backend
        st = {"q": q0.clone(), "u": u0.clone(), "lp": lp, "g": g}
        dE = samplers._mclmc_transition(integ, logdf, st, 6., math.sqrt(d), samplers._Rng(3))
        out[backend] = (st["q"].double().cpu().numpy(), st["u"].double().cpu().numpy(), dE, st["lp"])
    (qt, ut, dEt, lpt), (qh, uh, dEh, lph) = out["torch"], out["hip"]
    assert np.abs(qt - q0.double().cpu().numpy()).max() > 0.01 and math.isfinite(dEh)
    assert np.abs(qh - qt).max() <= TOL * np.abs(qt).max() and np.abs(uh - ut).max() <= TOL * np.abs(ut).max()
    assert abs(dEh - dEt) <= TOL * max(abs(lpt), abs(lp)), (dEh, dEt)      # the energy change is a difference of log densities of this size
    assert samplers.make_integrator(q0, None, "auto").backend == "hip"


# ---- on the model: _setup("lpt") of test_gpu_samplers.py (8^3, d about 1.7e3) ----
def _setup(evolution="lpt"):
    import torch
    from montecosmo_amd import model, logdensity, samplers
    rng = np.random.default_rng(7)
    ks = np.logspace(-3, 1, 128)
    kpow = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))
    fwd = model.FieldLevelForward(final_shape=(8, 8, 8), cell_length=40., box_center=(60., -40., 1400.), box_rotvec=(0.1, 0.2, -0.1),
                                  evolution=evolution, nbody_n_steps=3, lpt_order=2, init_oversamp=1.5, evol_oversamp=2.,
                                  ptcl_oversamp=2., paint_oversamp=2., a_obs=0.65, curved_sky=True, lin_kpow=kpow, nbody_a_start=0.1)
    cfg = dict(fwd.config(), final_shape=(8, 8, 8), cell_length=40., precond="kaiser")
    lat = {"sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2, low=0., high=np.inf),
           "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2), "b2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=3e-2)}
    fixed = dict(Omega_m=0.3111, bs2=0., bn2=0., b3=0., bds2=0., bs3=0., bnpar=0., ngbars=1e-3, s_e=1.0, s_ed=0., s_e2=0.)
    make_cosmo = lambda base: _cos(obg.Planck18(Omega_c=base["Omega_m"] - 0.0490), base["sigma8"])
    obs = 64. + 8. * rng.standard_normal((8, 8, 8))
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="kaiser")
    flat = samplers.FlatLogDensity(ld)
    start = {k + "_": 0.0 for k in lat}
    start["white_mesh_"] = (0.3 * rng.standard_normal(fwd.init_shape)).astype(np.float32)
    q0 = flat.pack(start)
    ref_lp = lambda q: bo.log_density(cfg, lat, fixed, {k: (np.asarray(v.cpu(), np.float64) if torch.is_tensor(v) else v)
                                                        for k, v in flat.unpack(q).items()}, obs, make_cosmo)
    return samplers, flat, q0, ref_lp


def _cos(c, s8):
    c.sigma8 = s8
    return c


@pytest.fixture(scope="module")
def problem(gpu):
    return _setup("lpt")


def test_preconditioned_mclmc_over_the_hip_log_density(problem):
    samplers, flat, q0, ref_lp = problem
    d = q0.numel()

    def run():
        state, config = samplers.mclmc_warmup(flat, q0, 60, diagonal_preconditioning=True, seed=5)
        return config, samplers.mclmc_run(flat, state, config, 10, thinning=2)
    c1, r1 = run()
    assert r1["backend"] == "hip" and len(r1["samples"]) == 10 and c1["inverse_mass"] is not None
    assert bool(torch_isfinite(c1["inverse_mass"])) and math.isfinite(c1["step_size"]) and c1["L"] == math.sqrt(d)
    de = np.array([i["energy_change"] for i in r1["infos"]])
    assert np.all(np.isfinite(de)) and all(math.isfinite(i["logdensity"]) and i["n_evals"] == 4 for i in r1["infos"])
    assert np.mean(de ** 2) / d < 20 * 5e-4                                 # energy-error variance per dimension near its target
    lp, lp_o = flat(r1["samples"][-1])[0], ref_lp(r1["samples"][-1])
    assert abs(lp - lp_o) < 2e-4 * abs(lp_o) + 0.05, (lp, lp_o)
    c2, r2 = run()
    assert np.array_equal(r2["samples"][-1].cpu().numpy(), r1["samples"][-1].cpu().numpy())      # bit for bit
    assert c2["step_size"] == c1["step_size"] and np.array_equal(c2["inverse_mass"].cpu().numpy(), c1["inverse_mass"].cpu().numpy())


def torch_isfinite(t):
    import torch
    return torch.isfinite(t).all()


def test_mams_over_the_hip_log_density(problem):
    samplers, flat, q0, ref_lp = problem

    def run():
        state, config = samplers.mams_warmup(flat, q0, 40, seed=6)
        return config, samplers.mams_run(flat, state, config, 10)
    c1, r1 = run()
    assert r1["backend"] == "hip" and len(r1["samples"]) == 10
    assert all(math.isfinite(i["logdensity"]) and math.isfinite(i["acceptance_rate"]) for i in r1["infos"])
    assert all(bool(torch_isfinite(s)) for s in r1["samples"])
    assert np.mean([i["acceptance_rate"] for i in r1["infos"]]) > 0.2
    c2, r2 = run()
    assert np.array_equal(r2["samples"][-1].cpu().numpy(), r1["samples"][-1].cpu().numpy()) and c2["step_size"] == c1["step_size"]
