"""Preconditioned MCLMC and MAMS, host side (no GPU): the 'torch' back end of the integrator in float64 against `_mclmc_B` and
the numpy restatement, the samplers on Gaussians, thinning, save / resume, `collapse_configs`, and the two exported symbols."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _mclmc_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _gauss(sd):
    sd = torch.as_tensor(sd, dtype=F64)

    def logdf(q):
        return float(-0.5 * ((q / sd) ** 2).sum()), -q / sd ** 2
    return logdf


def _unit(rng, d):
    u = rng.standard_normal(d)
    return u / np.linalg.norm(u)


def _with_c(rng, d, c):
    """A unit u and a unit e with u . e = c."""
    u = _unit(rng, d)
    v = rng.standard_normal(d)
    v -= v.dot(u) * u
    v /= np.linalg.norm(v)
    return u, c * u + math.sqrt(max(1. - c * c, 0.)) * v


# c near +-1 stops at 1 - 1e-3: dK depends on c through ln D, d ln D / dc = (1 - zeta^2) / D, and D -> 1 + c at large delta, so a last-bit
# difference in c (1e-16: the two codes measure it differently) moves dK by (d - 1) 1e-16 / (1 + c) -- 5e-12 at c = -0.999, d = 50, against
# |dK| of several hundred there; closer to -1 the comparison would measure the conditioning of the formula, not the code.
@pytest.mark.parametrize("delta", [1e-6, 1e-3, 0.1, 1., 5., 25.])
@pytest.mark.parametrize("c", [-0.999, -0.5, 0., 0.7, 0.999])
def test_kick_equals_mclmc_B(delta, c):
    from montecosmo_amd import samplers
    d = 50
    rng = np.random.default_rng(int(delta * 1e6) % 1000 + int(c * 1000) + 2000)
    u, e = _with_c(rng, d, c)
    gn = 3.7
    eps = delta * (d - 1) / gn
    ut, gt = torch.from_numpy(u), torch.from_numpy(gn * e)
    u_old, dK_old = samplers._mclmc_B(ut, gt, eps, d)
    integ = samplers.make_integrator(ut, None, "torch")
    u_new = ut.clone()
    integ.zero_dK()
    integ.kick_drift(u_new, None, gt, eps, 0.)
    dK_new = integ.read_dK()
    assert float((u_new - u_old).abs().max()) <= 1e-12
    assert abs(dK_new - dK_old) <= 1e-12 * max(1., abs(dK_old)), (dK_new, dK_old)
    u_ref, dK_ref, _ = ref.kick(u, gn * e, eps)
    assert np.abs(u_new.numpy() - u_ref).max() <= 1e-14 and abs(dK_new - dK_ref) <= 1e-12 * max(1., abs(dK_ref))
    assert abs(float(torch.linalg.vector_norm(u_new)) - 1.) < 1e-12      # (the same 1 / (1 + c) on a few 1e-16)


def test_kick_zero_force_huge_delta_and_unnormalised_u():
    from montecosmo_amd import samplers
    d = 50
    rng = np.random.default_rng(5)
    u = torch.from_numpy(_unit(rng, d))
    integ = samplers.make_integrator(u, None, "torch")
    # g = 0: u only normalised, no energy change, the drift still happens
    u1, q1 = 3. * u.clone(), torch.zeros(d, dtype=F64)
    integ.zero_dK()
    integ.kick_drift(u1, q1, torch.zeros(d, dtype=F64), 0.3, 0.5)
    assert float((u1 - u).abs().max()) < 1e-15 and integ.read_dK() == 0. and float((q1 - 0.5 * u).abs().max()) < 1e-15
    assert samplers._mclmc_B(u, torch.zeros(d, dtype=F64), 0.3, d)[1] == 0.
    # delta = 1e3: finite, u' -> e, dK = (d - 1)(delta - ln 2 + ln(1 + c))
    g = torch.from_numpy(rng.standard_normal(d))
    gn = float(torch.linalg.vector_norm(g))
    u2 = u.clone()
    integ.zero_dK()
    integ.kick_drift(u2, None, g, 1e3 * (d - 1) / gn, 0.)
    dK = integ.read_dK()
    c = float(torch.dot(u, g)) / gn
    assert torch.isfinite(u2).all() and math.isfinite(dK)
    assert float((u2 - g / gn).abs().max()) < 1e-14 and abs(dK - (d - 1) * (1e3 - math.log(2.) + math.log1p(c))) < 1e-9 * dK
    # an un-normalised u gives what the normalised one gives
    s = torch.from_numpy(rng.uniform(0.5, 2., d))
    integ_s = samplers.make_integrator(u, s * s, "torch")
    ua, ub = u.clone(), 2.5 * u.clone()
    integ_s.kick_drift(ua, None, g, 0.7, 0.)
    integ_s.kick_drift(ub, None, g, 0.7, 0.)
    assert float((ua - ub).abs().max()) < 1e-15
    u_ref, _, _ = ref.kick(u.numpy(), g.numpy(), 0.7, s.numpy())
    assert np.abs(ua.numpy() - u_ref).max() < 1e-14


@pytest.mark.parametrize("precond", [False, True])
def test_step_matches_restatement_and_is_reversible(precond):
    from montecosmo_amd import samplers
    d, n, eps = 50, 20, 0.4
    rng = np.random.default_rng(11)
    sd = np.exp(rng.uniform(-1., 1., d))
    s = sd.copy() if precond else None
    logdf = _gauss(sd)
    np_logdf = lambda q: (float(-0.5 * np.sum((q / sd) ** 2)), -q / sd ** 2)
    q0, u0 = torch.from_numpy(sd * rng.standard_normal(d)), torch.from_numpy(_unit(rng, d))
    integ = samplers.make_integrator(q0, None if s is None else torch.from_numpy(s * s), "torch")
    q, u = q0.clone(), u0.clone()
    lp, g = logdf(q)
    qr, ur, lpr, gr, dEr = ref.mclachlan_step(np_logdf, q0.numpy(), u0.numpy(), lp, g.numpy(), eps, s)
    lp, g, dE = samplers.mclachlan_step(integ, logdf, q, u, lp, g, eps)
    assert np.abs(q.numpy() - qr).max() < 1e-13 and np.abs(u.numpy() - ur).max() < 1e-13 and abs(dE - dEr) < 1e-11
    for _ in range(n - 1):
        lp, g, _ = samplers.mclachlan_step(integ, logdf, q, u, lp, g, eps)
    assert float((q - q0).abs().max()) > 0.1      # it went somewhere
    u.neg_()
    for _ in range(n):
        lp, g, _ = samplers.mclachlan_step(integ, logdf, q, u, lp, g, eps)
    assert float((q - q0).abs().max()) < 1e-9 and float((u + u0).abs().max()) < 1e-9


def test_energy_error_is_second_order():
    from montecosmo_amd import samplers
    d, T = 50, 2.4
    rng = np.random.default_rng(12)
    sd = np.exp(rng.uniform(-0.5, 0.5, d))
    logdf = _gauss(sd)
    starts = [(torch.from_numpy(sd * rng.standard_normal(d)), torch.from_numpy(_unit(rng, d))) for _ in range(16)]
    integ = samplers.make_integrator(starts[0][0], None, "torch")

    def rms(eps):
        out = []
        for q0, u0 in starts:
            q, u = q0.clone(), u0.clone()
            lp, g = logdf(q)
            tot = 0.
            for _ in range(int(round(T / eps))):
                lp, g, dE = samplers.mclachlan_step(integ, logdf, q, u, lp, g, eps)
                tot += dE
            out.append(tot)
        return float(np.sqrt(np.mean(np.square(out))))
    ratio = rms(0.2) / rms(0.1)
    assert 3. < ratio < 5., ratio


def _moments(samples):
    x = torch.stack(samples).numpy()
    return x.mean(0), x.std(0)


def test_diagonal_preconditioning_on_an_anisotropic_gaussian():
    """d = 100, sd log-spaced over 0.1 .. 10.  Seeds 0 .. 4 were all run before seed 0 was fixed: tuned step size 1.97 .. 2.06
    (identity) and 12.1 .. 13.3 (diagonal, ratio 6.1 .. 6.6), corr(log inverse_mass, log sd^2) 0.966 .. 0.974, std ratio under the
    diagonal metric 0.958 .. 1.018, |mean| / sd at most 0.09 (identity metric: 0.88 .. 1.20 and up to 0.35)."""
    from montecosmo_amd import samplers
    d = 100
    sd = np.logspace(-1, 1, d)
    logdf = _gauss(sd)
    q0 = torch.from_numpy(sd * np.random.default_rng(0).standard_normal(d))
    out = {}
    for precond in (False, True):
        state, config = samplers.mclmc_warmup(logdf, q0, 4000, diagonal_preconditioning=precond, seed=0, backend="torch")
        out[precond] = (config, samplers.mclmc_run(logdf, state, config, 20000, backend="torch"))
    (c_id, _), (c_di, run) = out[False], out[True]
    assert c_id["inverse_mass"] is None and c_di["L"] == math.sqrt(d)
    print("step sizes", c_id["step_size"], c_di["step_size"])
    assert c_di["step_size"] / c_id["step_size"] >= 3.
    corr = np.corrcoef(np.log(c_di["inverse_mass"].numpy()), np.log(sd ** 2))[0, 1]
    mean, std = _moments(run["samples"])
    print("corr", corr, "std ratio", (std / sd).min(), (std / sd).max(), "mean", np.abs(mean / sd).max())
    assert corr >= 0.9
    assert np.all(np.abs(std / sd - 1.) < 0.25) and np.all(np.abs(mean) / sd < 0.5)
    assert run["last_state"]["inverse_mass"] is not None and run["last_state"]["sampler"] == "mclmc"


def test_mams_on_a_gaussian():
    from montecosmo_amd import samplers
    d = 100
    sd = np.linspace(0.5, 2., d)
    logdf = _gauss(sd)
    q0 = torch.from_numpy(sd * np.random.default_rng(1).standard_normal(d))
    state, config = samplers.mams_warmup(logdf, q0, 1000, seed=0, backend="torch")
    run = samplers.mams_run(logdf, state, config, 4000, backend="torch")
    acc = np.mean([i["acceptance_rate"] for i in run["infos"]])
    mean, std = _moments(run["samples"])
    print("acceptance", acc, "std ratio", (std / sd).min(), (std / sd).max(), "mean", np.abs(mean / sd).max(), config["step_size"], config["L"])
    assert 0.5 <= acc <= 0.85
    assert np.all(np.abs(std / sd - 1.) < 0.25) and np.all(np.abs(mean) / sd < 0.5)
    assert all(i["n_evals"] == 2 * i["n_steps"] and i["n_steps"] >= 1 for i in run["infos"])


def test_mams_rejection_leaves_the_state_untouched():
    from montecosmo_amd import samplers
    d = 20
    logdf = _gauss(0.1 * np.ones(d))
    q = torch.from_numpy(0.1 * np.random.default_rng(2).standard_normal(d))
    lp, g = logdf(q)
    rng = samplers._Rng(0)
    integ = samplers.make_integrator(q, None, "torch")
    n_rej = 0
    for _ in range(30):      # a step size far too large: almost every proposal is rejected
        st = {"q": q, "u": None, "lp": lp, "g": g}
        keep = (q.clone(), g.clone())
        acc, n = samplers._mams_transition(integ, logdf, st, 3., 6., rng)
        if st["q"] is q:
            n_rej += 1
            assert st["lp"] == lp and st["g"] is g and torch.equal(q, keep[0]) and torch.equal(g, keep[1])
        q, lp, g = st["q"], st["lp"], st["g"]
    assert n_rej >= 5
    # a non-finite energy change is a rejection
    bad = lambda x: (float("nan"), torch.zeros_like(x))
    st = {"q": q, "u": None, "lp": lp, "g": g}
    acc, _ = samplers._mams_transition(integ, bad, st, 0.5, 2., rng)
    assert acc == 0. and st["q"] is q and st["lp"] == lp and st["g"] is g


def test_thinning_keeps_every_kth_state():
    from montecosmo_amd import samplers
    d = 30
    sd = np.linspace(0.5, 2., d)
    logdf = _gauss(sd)
    q0 = torch.from_numpy(sd * np.random.default_rng(3).standard_normal(d))
    state, config = samplers.mclmc_warmup(logdf, q0, 200, diagonal_preconditioning=True, seed=4, backend="torch")
    one = samplers.mclmc_run(logdf, state, config, 40, thinning=1, backend="torch")
    four = samplers.mclmc_run(logdf, state, config, 10, thinning=4, backend="torch")
    assert all(torch.equal(four["samples"][i], one["samples"][4 * i + 3]) for i in range(10))
    de = np.array([i["energy_change"] for i in one["infos"]]).reshape(10, 4)
    for i, info in enumerate(four["infos"]):
        assert info["energy_change"] == pytest.approx(math.sqrt(np.mean(de[i] ** 2)), rel=1e-14)
        assert info["mse_per_dim"] == pytest.approx(info["energy_change"] ** 2 / d, rel=1e-14) and info["n_evals"] == 8
    assert torch.equal(four["last_state"]["q"], one["last_state"]["q"]) and torch.equal(four["last_state"]["u"], one["last_state"]["u"])
    # MAMS: acceptance averaged, steps and evaluations summed
    state, config = samplers.mams_warmup(logdf, q0, 100, seed=4, backend="torch")
    one = samplers.mams_run(logdf, state, config, 12, backend="torch")
    three = samplers.mams_run(logdf, state, config, 4, thinning=3, backend="torch")
    assert all(torch.equal(three["samples"][i], one["samples"][3 * i + 2]) for i in range(4))
    for i, info in enumerate(three["infos"]):
        blk = one["infos"][3 * i:3 * i + 3]
        assert info["acceptance_rate"] == pytest.approx(np.mean([b["acceptance_rate"] for b in blk]), rel=1e-14)
        assert info["n_steps"] == sum(b["n_steps"] for b in blk) and info["n_evals"] == 2 * info["n_steps"]


def test_collapse_configs():
    from montecosmo_amd import samplers
    rng = np.random.default_rng(6)
    for n in (3, 4):
        cfgs = [{"L": 1., "step_size": float(rng.uniform(0.5, 2.)), "inverse_mass": torch.from_numpy(rng.uniform(0.1, 3., 7))} for _ in range(n)]
        got = samplers.collapse_configs(cfgs, eval_per_ess=800.)
        want = ref.collapse_configs([dict(c, inverse_mass=c["inverse_mass"].numpy()) for c in cfgs], eval_per_ess=800.)
        assert got["step_size"] == pytest.approx(want["step_size"], rel=1e-15) and got["L"] == pytest.approx(want["L"], rel=1e-15)
        assert np.allclose(got["inverse_mass"].numpy(), want["inverse_mass"], rtol=1e-15, atol=0)
    got = samplers.collapse_configs([{"L": 1., "step_size": 0.3, "inverse_mass": None}, {"L": 2., "step_size": 0.5, "inverse_mass": None}])
    assert got["inverse_mass"] is None and got["step_size"] == pytest.approx(0.4) and got["L"] == pytest.approx(0.4 * 1e3 / 2 * 0.4)


def test_moments_match_restatement():
    from montecosmo_amd import samplers
    rng = np.random.default_rng(8)
    q = torch.from_numpy(rng.standard_normal(33))
    integ = samplers.make_integrator(q, None, "torch")
    xa, x2a = integ.new_moments()
    xr, x2r = np.zeros(33), np.zeros(33)
    for k in range(3):
        qk = q * (k + 1.)
        integ.moments(qk, 0.98, 0.7, xa, x2a)
        xr, x2r = ref.moments(qk.numpy(), 0.98, 0.7, xr, x2r)
    assert np.array_equal(xa.numpy(), xr) and np.array_equal(x2a.numpy(), x2r)


@pytest.mark.parametrize("which", ["mclmc", "mams"])
def test_new_chains_save_and_resume_exactly(tmp_path, which):
    """The pattern of test_chain_save_and_resume_continue_exactly: a chain continued from the saved state repeats the uninterrupted one."""
    from montecosmo_amd import samplers
    scale = torch.tensor([1.0, 0.5, 2.0, 1.5], dtype=F64)

    def logdf(q):
        return float(-0.5 * ((q / scale) ** 2).sum()), -q / scale ** 2

    warmup, run = (samplers.mclmc_warmup, samplers.mclmc_run) if which == "mclmc" else (samplers.mams_warmup, samplers.mams_run)
    q0 = torch.zeros(4, dtype=F64) + 0.1
    path = str(tmp_path / "chain")
    state, config = warmup(logdf, q0, 60, diagonal_preconditioning=True, seed=3, backend="torch")
    whole = run(logdf, state, config, 40, thinning=2, backend="torch")
    first = run(logdf, state, config, 15, thinning=2, backend="torch")
    samplers.save_run(first, 0, path)
    rest = run(logdf, samplers.load_state(path), None, 25, thinning=2, backend="torch")
    samplers.save_run(rest, 1, path)
    a, b = np.load(path + "_0.npz"), np.load(path + "_1.npz")
    joined = np.concatenate([a["samples"], b["samples"]])
    assert joined.shape == (40, 4) and not a["warmup"].any()
    assert np.array_equal(joined, torch.stack(whole["samples"]).numpy())
    assert "n_evals" in a.files and len(a["n_evals"]) == 15
    assert rest["last_state"]["inverse_mass"] is not None and torch.equal(rest["last_state"]["q"], whole["last_state"]["q"])
    # the driver, through the adapter: warm-up run, two more runs, then a resumed fourth run
    sampler = samplers.chain_sampler(which, diagonal_preconditioning=True)
    res = samplers.sample_and_save(sampler, logdf, q0, str(tmp_path / "drv"), start=0, end=2, n_warmup=40, n_samples=10, seed=1, thinning=2,
                                   backend="torch")
    res2 = samplers.sample_and_save(sampler, logdf, q0, str(tmp_path / "drv"), start=3, end=3, n_samples=10, resume=True, thinning=2,
                                    backend="torch")
    assert all((tmp_path / f"drv_{i}.npz").exists() for i in range(4))
    assert res2["step_size"] == res["step_size"] and res2["L"] == res["L"] and len(res2["samples"]) == 10


def test_symbols_are_declared_bound_and_exported():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("mcpm_mclmc_kick_drift_f32", "mcpm_mclmc_moments_f64"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mcpm_mclmc_kick_drift_f32"][1]) == 9 and len(_lib.SIGNATURES["mcpm_mclmc_moments_f64"][1]) == 7
    assert _lib.lib.mcpm_mclmc_kick_drift_f32(None, None, None, None, None, 8, 0.1, 0.1, None) == -6      # MCPM_E_ARG, no launch
    assert _lib.lib.mcpm_mclmc_moments_f64(None, None, 8, 0.9, 1., None, None) == -6
    assert _lib.lib.mcpm_version().decode() == "mcpm 0.12 (gfx950)"


def test_backend_selection():
    from montecosmo_amd import samplers
    q = torch.zeros(5, dtype=F64)
    assert samplers.make_integrator(q, None, "auto").backend == "torch" and not samplers.hip_backend_applies(q)
    with pytest.raises(ValueError):
        samplers.make_integrator(q, None, "hip")
    with pytest.raises(ValueError):
        samplers.make_integrator(q, None, "triton")
