"""N-body evolution on the light cone, the parts that need no GPU: the float64 restatement (tests/_nbody_lc_f64.py) against the oracle's
snapshots and against its own central differences, and the declarations of the new entry points."""
import os

import numpy as np
import pytest

import _nbody_lc_f64 as lc
from oracle import pm_oracle as o, background as obg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, K, A0, A_END = (8, 8, 8), 3, 0.2, 0.8


@pytest.fixture(scope="module")
def setup():
    rng = np.random.default_rng(5)
    spec = np.fft.rfftn(0.3 * rng.standard_normal(SHAPE))
    pos = o.regular_pos(SHAPE)
    cosmo = obg.Planck18()
    a_p = rng.uniform(0.1, 0.95, len(pos))
    return dict(rng=rng, spec=spec, pos=pos, cosmo=cosmo, a_p=a_p, traj=lc.run(cosmo, spec, pos, A0, A_END, K))


def test_one_time_for_all_particles_is_the_oracle_snapshot(setup):
    s = setup
    for a_s in (0.3, 0.5, 0.77):
        p, v = lc.nbody_lc(s["cosmo"], s["spec"], s["pos"], A0, np.full(len(s["pos"]), a_s), A_END, K)
        ps, vs = o.nbody_bf(s["cosmo"], s["spec"], s["pos"], A0, A_END, K, snapshots=[a_s])
        assert np.abs(p - ps[0]).max() < 1e-13 and np.abs(v - vs[0]).max() < 1e-13


def test_clamps(setup):
    s = setup
    traj, g0, dg = s["traj"]
    n = len(s["pos"])
    p, v = lc.nbody_lc(s["cosmo"], s["spec"], s["pos"], A0, np.full(n, 1.0), A_END, K)
    assert np.array_equal(p, traj[K][0]) and np.array_equal(v, traj[K][1])          # later than the end: the final state, exactly
    p, v = lc.nbody_lc(s["cosmo"], s["spec"], s["pos"], A0, np.full(n, A_END), A_END, K)
    assert np.array_equal(p, traj[K][0]) and np.array_equal(v, traj[K][1])
    p, v = lc.nbody_lc(s["cosmo"], s["spec"], s["pos"], A0, np.full(n, 0.05), A_END, K)
    assert np.array_equal(p, traj[0][0]) and np.array_equal(v, traj[0][1])          # earlier than the start: the LPT start state
    i, th, inside = lc.locate(o.a2g(s["cosmo"], s["a_p"]), g0, dg, K)
    assert set(i) == set(range(K)) and (~inside & (th == 0)).any() and (~inside & (th == 1)).any()      # the mixed case has everything
    assert np.allclose(lc.weights(o.a2g(s["cosmo"], s["a_p"]), g0, dg, K).sum(0), 1.0, rtol=0, atol=1e-15)


def test_reverse_sweep_against_central_differences(setup):
    """The pins of tests/test_bias_f64_host.py: eps = 1e-6, agreement to 1e-7 of max(|fd|, |bar| |d|)."""
    s = setup
    rng, cosmo, spec, pos = s["rng"], s["cosmo"], s["spec"], s["pos"]
    traj, g0, dg = s["traj"]
    g_p = o.a2g(cosmo, s["a_p"])
    Xb, Vb = rng.standard_normal((len(pos), 3)), rng.standard_normal((len(pos), 3))
    mb, sb, gb = lc.nbody_lc_vjp(cosmo, spec, pos, Xb, Vb, A0, None, A_END, K, g_p=g_p)
    assert np.all(gb[(g_p < g0) | (g_p > g0 + K * dg)] == 0) and np.count_nonzero(gb) > len(pos) // 2
    eps = 1e-6

    def loss(spec_=spec, g_p_=g_p):
        p, v = lc.nbody_lc(cosmo, spec_, pos, A0, None, A_END, K, g_p=g_p_)
        return float((Xb * p).sum() + (Vb * v).sum())

    def sel(g0_=g0, dg_=dg):      # the selection alone, the step states held: what the theta terms of g0 and dg are the derivative of
        p, v = lc.select(traj, g_p, g0_, dg_)
        return float((Xb * p).sum() + (Vb * v).sum())

    d = np.fft.rfftn(0.3 * rng.standard_normal(SHAPE))
    fd = (loss(spec_=spec + eps * d) - loss(spec_=spec - eps * d)) / (2 * eps)
    an = float((np.conj(mb) * d).real.sum())
    assert abs(fd - an) < 1e-7 * max(abs(fd), np.linalg.norm(mb) * np.linalg.norm(d)), ("init_mesh", fd, an)
    dgp = rng.standard_normal(len(pos)) * dg
    fd = (loss(g_p_=g_p + eps * dgp) - loss(g_p_=g_p - eps * dgp)) / (2 * eps)
    assert abs(fd - (gb * dgp).sum()) < 1e-7 * max(abs(fd), np.linalg.norm(gb) * np.linalg.norm(dgp)), ("g_p", fd, (gb * dgp).sum())
    h = eps * dg
    fd = (sel(g0_=g0 + h) - sel(g0_=g0 - h)) / (2 * h)
    assert abs(fd - sb["g0_theta"]) < 1e-7 * max(abs(fd), np.abs(gb).sum()), ("g0", fd, sb["g0_theta"])
    fd = (sel(dg_=dg + h) - sel(dg_=dg - h)) / (2 * h)
    assert abs(fd - sb["dg_theta"]) < 1e-7 * max(abs(fd), np.abs(gb).sum()), ("dg", fd, sb["dg_theta"])
    # with no particle inside the run the sweep is the oracle's own, for the cotangents of the final state
    mb1, sb1, gb1 = lc.nbody_lc_vjp(cosmo, spec, pos, Xb, Vb, A0, np.full(len(pos), 1.0), A_END, K)
    mb_o, sb_o = o.nbody_bf_vjp(cosmo, spec, pos, Xb, Vb, A0, A_END, K)
    assert np.array_equal(mb1, mb_o) and not gb1.any() and all(np.array_equal(sb1[k], sb_o[k]) for k in sb_o)


def test_new_symbols_are_declared_bound_and_exported():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    for name, nargs in (("mcpm_nbody_lightcone_f32", 10), ("mcpm_nbody_bf_lc_vjp_f32", 19)):
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.ABI_VERSION == "mcpm 0.12 (gfx950)" and '#define MCPM_ABI_VERSION "mcpm 0.12 (gfx950)"' in header
    makefile = open(os.path.join(ROOT, "montecosmo_amd", "csrc", "Makefile")).read()
    assert makefile.split("SRCS  :=")[1].splitlines()[0].split()[-1] == "lightcone.hip"


def test_model_constructs_on_the_light_cone():
    from montecosmo_amd import model
    fwd = model.FieldLevelForward(final_shape=(8, 8, 8), evolution='nbody')
    assert fwd.a_obs is None and fwd.evolution == 'nbody'
