"""tests/_model_f64.py, the composed float64 reference of the forward model and its log density, pinned on the CPU:
  * wherever a per-feature restatement is defined, the composition returns its mesh (relative L2 < 1e-12) and its log density (< 1e-10
    relative): both sides are the same float64 operations, possibly in another order, so the composition is a reference and not a
    second opinion;
  * the case table of tests/_model_cases.py contains every valid pair of levels of its factors, and every case mixes features;
  * at every case of the table the reference's own central differences at h and h / 2 agree (1e-3 relative, 1e-6 absolute) for every
    sampled scalar and for the white-mesh direction, the point lies inside the support of its likelihood, and the features it switches
    on move the result -- conditions on the reference alone, so that tests/test_gpu_model_combinations.py compares against a derivative.
Sizes: final 8^3, init 12^3, evolution / paint 16^3, the smallest the model tests use."""
import numpy as np
import pytest

import _ap_f64 as apo
import _eulerian_f64 as ef
import _kaiser_f64 as kf
import _lik_f64 as L
import _lik_phi_f64 as P
import _model_cases as C
import _model_f64 as M
import _png_f64 as pf
from oracle import bias_oracle as bo

BIAS = dict(b1=0.8, b2=0.2, bs2=-0.15, b3=0.1, bds2=0.1, bs3=-0.05, bn2=20.0, bnpar=5.0)
PNG = dict(fNL=300., fNL_bp=3., fNL_bpd=-1., fNL_bpd2=-20., fNL_bps2=30., fNL_bn2p=2.0e3)
AP = {"alpha_iso": 1.03, "alpha_ap": 0.97}


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _setting(evo, **kw):
    """A case-shaped dict for a single-feature setting (it need not mix features), its configuration, a cosmology and a white field."""
    c = C._case(evo, kw.pop("bias_type", "lagrangian"), kw.pop("png_type", None), kw.pop("ap_auto", None), kw.pop("lik_type", "quad_gauss"),
                kw.pop("survey", "none"), kw.pop("precond", "fourier"), kw.pop("s_ep", False), kw.pop("temp", 1.), **kw)
    cfg = C.config(c)
    rng = np.random.default_rng(31)
    white = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * (12 ** 3 / np.prod(cfg["box_size"])) ** .5
    return c, cfg, C.make_cosmo(dict(Omega_m=0.25, sigma8=0.8102)), white


# ---- agreement with the per-feature restatements: evolve ----------------------------------------------------------------------------
@pytest.mark.parametrize("evo", ["lpt", "lpt_lc", "nbody"])
def test_evolve_plain_is_the_oracles(evo):
    _, cfg, cosmo, white = _setting(evo)
    want, aux_o = bo.evolve(cfg, cosmo, BIAS, white)
    got, aux = M.evolve(cfg, cosmo, BIAS, white)
    assert rel_l2(got, want) < 1e-12
    assert rel_l2(aux["pos"], aux_o["pos"]) < 1e-12 and rel_l2(aux["weights"], aux_o["weights"]) < 1e-12
    assert rel_l2(aux["evol_mesh"], aux_o["init_mesh"]) < 1e-12 and aux["phi"] is None and aux["white"] is white


@pytest.mark.parametrize("png_type", ["fNL", "bias"])
@pytest.mark.parametrize("evo", ["lpt_lc", "nbody"])
def test_evolve_png_is_the_png_restatement(evo, png_type):
    _, cfg, cosmo, white = _setting(evo, png_type=png_type)
    got, aux = M.evolve(cfg, cosmo, BIAS, white, png=PNG, png_type=png_type)
    assert rel_l2(got, pf.evolve(cfg, cosmo, BIAS, white, PNG, png_type)) < 1e-12
    assert rel_l2(got, bo.evolve(cfg, cosmo, BIAS, white)[0]) > 1e-3      # (and PNG moves the mesh)
    assert rel_l2(aux["phi"], pf.png_fields(pf.trans_table(cosmo), aux["evol_mesh"], cfg["box_size"])[0]) < 1e-12


@pytest.mark.parametrize("png_type", [None, "fNL", "bias"])
@pytest.mark.parametrize("evo", ["lpt", "nbody"])
def test_evolve_eulerian_is_the_eulerian_restatement(evo, png_type):
    _, cfg, cosmo, white = _setting(evo, bias_type="eulerian", png_type=png_type)
    got, _ = M.evolve(cfg, cosmo, BIAS, white, png=PNG, png_type=png_type, bias_type="eulerian")
    assert rel_l2(got, ef.evolve(cfg, cosmo, BIAS, white, PNG, png_type)) < 1e-12
    assert rel_l2(got, M.evolve(cfg, cosmo, BIAS, white, png=PNG, png_type=png_type)[0]) > 1e-3      # (not the Lagrangian mesh)


@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("evo", ["lpt", "lpt_lc", "nbody"])
def test_evolve_ap_is_the_ap_restatement(evo, auto):
    _, cfg, cosmo, white = _setting(evo, ap_auto=auto)
    fid = C.cosmo_fid_oracle()
    got, _ = M.evolve(cfg, cosmo, BIAS, white, ap_auto=auto, ap=AP, cosmo_fid=fid)
    assert rel_l2(got, apo.evolve_ap(cfg, cosmo, BIAS, white, auto, AP, fid)) < 1e-12
    assert rel_l2(got, bo.evolve(cfg, cosmo, BIAS, white)[0]) > 1e-2


@pytest.mark.parametrize("flat,a_obs,png_type", [(False, None, None), (False, None, "bias"), (True, 0.65, None), (True, 0.65, "fNL")])
def test_evolve_kaiser_is_the_kaiser_restatement(flat, a_obs, png_type):
    _, cfg, cosmo, white = _setting("kaiser", flat=flat, png_type=png_type)
    cfg["a_obs"] = a_obs
    got, aux = M.evolve(cfg, cosmo, BIAS, white, png=PNG, png_type=png_type, bias_type="eulerian")      # (bias_type is ignored)
    assert rel_l2(got, kf.evolve(cfg, cosmo, BIAS, white, PNG, png_type)[0]) < 1e-12
    assert aux["phi"] is None and aux["pos"] is None
    if flat:      # the flat sky at fixed a: the oracle's and the PNG restatement's own Kaiser branches
        want = bo.evolve(cfg, cosmo, BIAS, white)[0] if png_type is None else pf.evolve(cfg, cosmo, BIAS, white, PNG, png_type)
        assert rel_l2(got, want) < 1e-12


# ---- agreement with the per-feature restatements: log density -------------------------------------------------------------------------
def _close(got, want):
    assert np.isfinite(want) and abs(got - want) < 1e-10 * abs(want), (got, want)


def _built(evo, **kw):
    return C.build(_setting(evo, **kw)[0])


@pytest.mark.parametrize("evo,survey,precond", [("lpt", "none", "fourier"), ("nbody", "survey", "kaiser"), ("lpt_lc", "ngbars", "real"),
                                                ("kaiser", "survey", "real")])
def test_log_density_plain_is_the_oracles(evo, survey, precond):
    b = _built(evo, survey=survey, precond=precond, flat=True if evo == "kaiser" else None)
    if evo == "kaiser":
        b["cfg"]["a_obs"] = 0.65      # the oracle's Kaiser branch: the flat sky at fixed a
    _close(b["ref"](b["sample"]), bo.log_density(b["cfg"], b["lat"], b["fixed"], b["sample"], b["obs"], C.make_cosmo))


@pytest.mark.parametrize("auto", [True, False])
def test_log_density_ap_is_the_ap_restatement(auto):
    b = _built("lpt", ap_auto=auto)
    want = apo.log_density_ap(b["cfg"], b["lat"], b["fixed"], b["sample"], b["obs"], C.make_cosmo, auto, C.cosmo_fid_oracle())
    _close(b["ref"](b["sample"]), want)


@pytest.mark.parametrize("survey", ["none", "survey", "ngbars"])
@pytest.mark.parametrize("lik_type,temp", [("quad_gauss", 1.), ("shash", 2.5), ("two_quad_gauss", 1.), ("poisson", 2.5)])
def test_log_density_families_are_the_phi_restatement(lik_type, temp, survey):
    """Each real-space family with PNG, the term s_ep phi (the families that read it) and a temperature, survey on and off."""
    b = _built("lpt_lc", png_type="fNL", lik_type=lik_type, survey=survey, s_ep=lik_type != "poisson", temp=temp)
    info = {}
    got = b["ref"](b["sample"], info)
    _close(got, P.log_density(b["cfg"], b["lat"], b["fixed"], b["sample"], b["obs"], C.make_cosmo, lik_type, "fNL", temp=temp))
    assert lik_type == "poisson" or np.abs(info["s_ep_phi"]).max() > 0.05      # the term is there


@pytest.mark.parametrize("lik_type", ["shash", "poisson", "fourier_gauss"])
def test_log_density_families_are_the_likelihood_restatement(lik_type):
    b = _built("lpt", lik_type=lik_type, survey="none" if lik_type == "fourier_gauss" else "survey")
    want = L.log_density(b["cfg"], b["lat"], b["fixed"], b["sample"], b["obs"], C.make_cosmo, lik_type, los_fid=M.los_fid(b["cfg"]))
    _close(b["ref"](b["sample"]), want)


def test_fourier_temperature_is_the_gaussian_law():
    """The one step no restatement composes: 'fourier_gauss' at a temperature takes the family at the selection selec * temp
    (tests/test_gpu_likelihood_phi.py::test_fourier_with_a_temperature holds the kernel to the same statement).  Every mode is a normal
    whose sigma grows by sqrt(temp), so lp(T) = lp(1) - N / 2 log T + (1 - 1 / T) Q with Q = sum z^2 / 2: Q from T = 2.5 predicts T = 4."""
    b = _built("lpt", lik_type="fourier_gauss")
    lp = {T: M.log_density(b["cfg"], b["lat"], b["fixed"], b["sample"], b["obs"], C.make_cosmo, lik_type="fourier_gauss", temp=T)
          for T in (1., 2.5, 4.)}
    n = b["obs"].size
    Q = (lp[2.5] - lp[1.] + n / 2 * np.log(2.5)) / (1 - 1 / 2.5)
    assert Q > 0
    _close(lp[4.], lp[1.] - n / 2 * np.log(4.) + (1 - 1 / 4.) * Q)


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_valid_pair():
    valid = C.valid_pairs()
    assert len(valid) > 300      # 9 factors, 27 levels
    assert all(C.valid(c) for c in C.CASES)
    seen = set().union(*(C.pairs_of(c) for c in C.CASES))
    assert not valid - seen, sorted(valid - seen, key=str)
    assert seen <= valid
    assert all(C.n_features(c) >= 2 for c in C.CASES), [C.case_id(c) for c in C.CASES if C.n_features(c) < 2]
    assert len({C.case_id(c) for c in C.CASES}) == len(C.CASES)
    # every (evolution, likelihood) pair needs a case of its own: 20 is the least a covering table can have
    assert len(C.CASES) == len(C.FACTORS["evo"]) * len(C.FACTORS["lik_type"])
    assert sum(c["evo"] == "nbody" for c in C.CASES) <= 5
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in C.CASES)
    assert has(evo="lpt_lc", bias_type="eulerian", png_type="bias", ap_auto=True, lik_type="two_quad_gauss", s_ep=True, survey="survey")
    assert has(evo="nbody", bias_type="lagrangian", png_type="fNL", ap_auto=False, lik_type="shash", survey="ngbars", temp=2.5)


def test_case_configuration_is_the_models():
    """`_model_cases.config` restates FieldLevelForward.config() by hand, so that the host tests need no library; here the two meet."""
    from montecosmo_amd import bricks, model
    for c in (C.CASES[0], C.CASES[7], C.CASES[11], C.CASES[15]):
        got, want = C.config(c), model.FieldLevelForward(cosmo_fid=bricks.Planck18() if c["ap_auto"] else None, **C.forward_kwargs(c)).config()
        assert set(want) <= set(got)
        for k, v in want.items():
            assert np.array_equal(np.asarray(got[k], dtype=object), np.asarray(v, dtype=object)) if k != "lin_kpow" else all(
                np.array_equal(a, b) for a, b in zip(got[k], v)), k


@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_reference_derivatives_are_converged(c):
    b = C.build(c)
    info = {}
    lp = b["ref"](b["sample"], info)
    assert np.isfinite(lp)
    obs, cm = b["obs"][info["mask"]], info["count"][info["mask"]]
    if c["lik_type"] == "quad_gauss":      # inside the support: a cell at -inf would show nothing
        assert info["D"].min() > 0
    if c["lik_type"] == "poisson":
        assert np.array_equal(obs, np.round(obs)) and obs.min() >= 0 and cm.min() > 0
    if c["s_ep"]:      # the term is there: scale1 moves by per cent in some cells
        assert np.abs(info["s_ep_phi"]).max() > 0.02
    if c["ap_auto"] is not None or c["png_type"] is not None or c["bias_type"] == "eulerian" and c["evo"] != "kaiser":
        plain = M.evolve(b["cfg"], C.make_cosmo(info["base"]), {k: info["base"][k] for k in bo.BIAS_KEYS}, info["aux"]["white"])[0]
        assert rel_l2(info["gxy"], plain) > 1e-3      # the forward-model features move the mesh
    for name, idx in C.scalar_names(b) + [("white_mesh", None)]:
        h = b["h"][name]
        fd, half = C.central_difference(b, name, idx, h), C.central_difference(b, name, idx, h / 2)
        assert abs(fd - half) < 1e-3 * abs(half) + 1e-6, (name, idx, h, fd, half)
