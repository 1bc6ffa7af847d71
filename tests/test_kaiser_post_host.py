"""Host checks of the chain start (kaiser_post): the ABI entry, the inverse reparametrisation, and the known answer that pins the float64
restatement tests/_kaiser_post_f64.py -- on a flat-sky Kaiser model the restated posterior mean is where the float64 log posterior peaks.
No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _kaiser_post_f64 as kp
from oracle import background as obg, bias_oracle as bo, pm_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NORMAL = dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2)
SIGMA8 = dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2, low=0., high=np.inf)      # truncated below only
OMEGA_M = dict(loc=0.3111, scale=0.1, loc_fid=0.3111, scale_fid=1e-2, low=0.05, high=1.)       # truncated on both sides
UNIF = dict(low=-1., high=1.5)
NGB = dict(loc=1e-3, scale=1e-2, loc_fid=np.array([1e-3, 1.4e-3, 0.9e-3]), scale_fid=np.array([1e-5, 2e-5, 1e-5]), low=0., high=np.inf)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_header_binding_and_version():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    assert re.search(r"\bint\s+mcpm_kaiser_post_c64\s*\(", header)
    assert "mcpm_kaiser_post_c64" in _lib.SIGNATURES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "mcpm_kaiser_post_c64")      # exported by the cross-compiled library
    version = re.search(r'#define\s+MCPM_ABI_VERSION\s+"([^"]+)"', header).group(1)
    assert version == _lib.ABI_VERSION == _lib.lib.mcpm_version().decode() == "mcpm 0.12 (gfx950)"
    # the binding has one argument per parameter of the declaration
    decl = re.search(r"int\s+mcpm_kaiser_post_c64\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["mcpm_kaiser_post_c64"][1]) == 24


# ---- latent round trips ---------------------------------------------------------------------------------------------------------------
def _host_density(latents, ngb=None, n_rbins=0):
    """A log-density object as far as `base_params` / `sample_params` read it for scalars (no device, no forward model)."""
    from montecosmo_amd import logdensity
    ld = logdensity.FieldLevelLogDensity.__new__(logdensity.FieldLevelLogDensity)
    ld.latents = {k: dict({"low": -math.inf, "high": math.inf}, **{kk: float(vv) for kk, vv in v.items()}) for k, v in latents.items()}
    for c in ld.latents.values():
        if "loc" not in c:
            c.setdefault("loc_fid", (c["low"] + c["high"]) / 2)
            c.setdefault("scale_fid", (c["high"] - c["low"]) / 12 ** .5)
    ld.fixed, ld.n_rbins = {"q": 3.}, n_rbins
    ld.ngb_lat = None if ngb is None else {k: np.broadcast_to(np.asarray(v, dtype=np.float64), (n_rbins,)).copy() for k, v in ngb.items()}
    return ld


@pytest.mark.parametrize("name,conf,values", [
    ("b1", NORMAL, (1.0, 0.93, 1.4)),
    ("sigma8", SIGMA8, (0.8102, 0.75, 0.9, 0.2)),
    ("Omega_m", OMEGA_M, (0.3111, 0.25, 0.4, 0.06)),
    ("u", UNIF, (0.25, -0.9, 1.4)),
])
def test_latent_round_trip(name, conf, values):
    ld = _host_density({name: conf})
    for v in values:
        s = ld.sample_params({name: v, "q": 7.})      # a fixed key is ignored
        assert set(s) == {name + "_"}
        assert s[name + "_"] == pytest.approx(kp.base2sample(v, conf), rel=1e-9, abs=1e-12)      # ... and is what the restatement gives
        back = ld.base_params(s)[name]
        assert abs(back - v) <= 1e-12 * abs(v), (name, v, back)
        again = ld.sample_params({name: back})[name + "_"]
        assert abs(again - s[name + "_"]) <= 1e-9 * max(1., abs(s[name + "_"]))


def test_per_shell_ngbars_round_trip():
    ld = _host_density({}, NGB, 3)
    v = np.array([1.1e-3, 1.3e-3, 0.8e-3])
    s = ld.sample_params({"ngbars": v})["ngbars_"]
    assert s.shape == (3,) and np.allclose(s, kp.base2sample(v, NGB), rtol=1e-9)
    back = ld.base_params({"ngbars_": s})["ngbars"]
    assert np.all(np.abs(back - v) <= 1e-12 * np.abs(v))
    # a leading chain axis is inverted element by element
    s2 = ld.sample_params({"ngbars": np.stack([v, v[::-1] * 1.01])})["ngbars_"]
    assert s2.shape == (2, 3) and np.array_equal(s2[0], s)


@pytest.mark.parametrize("x,low,high", [(-13., -20., 5.), (-14.5, -np.inf, 3.), (14., -3., 30.), (13.2, -5., np.inf)])
def test_tail_branches_round_trip(x, low, high):
    """Beyond 12 fiducial sigma with the bound on that side beyond 12 sigma too: the soft maximum / minimum and its inverse."""
    from montecosmo_amd import logdensity
    loc, scale = 0.3, 0.01
    lo, hi = loc + scale * low, loc + scale * high
    y = logdensity.std2trunc_and_derivs(x, loc, scale, lo, hi)[0]
    assert abs((y - loc) / scale) > 12      # the inverse takes the tail branch as well
    got = logdensity.trunc2std(y, loc, scale, lo, hi)
    assert abs(got - x) <= 1e-9 * abs(x)      # sample -> base -> sample
    assert got == pytest.approx(kp.trunc2std(y, loc, scale, lo, hi), rel=1e-12)
    assert abs(logdensity.std2trunc_and_derivs(got, loc, scale, lo, hi)[0] - y) <= 1e-12 * abs(y)      # base -> sample -> base


# ---- the restatement's own checks -----------------------------------------------------------------------------------------------------
def test_restatement_self_check():
    assert kp.self_check()


def test_count2delta_known_answers():
    rng = np.random.default_rng(3)
    mesh = rng.uniform(1., 9., (6, 4, 8))
    assert np.allclose(kp.count2delta(mesh, 1.), (mesh - mesh.mean()) / mesh.mean(), rtol=1e-14, atol=0)
    assert np.allclose(kp.count2delta(mesh, 0.37), (mesh - mesh.mean()) / mesh.mean(), rtol=1e-13, atol=0)      # any scalar selection
    sel = rng.uniform(.2, 1., mesh.shape)
    sel[0] = 0.      # cells outside the survey
    mesh = np.where(sel > 0, mesh, 0.)
    closed = (mesh / mesh.mean() - sel / sel.mean()) / ((sel / sel.mean()) ** 2).mean() ** .5      # bricks.py:931-934
    assert np.allclose(kp.count2delta(mesh, sel), closed, rtol=1e-13, atol=1e-15)
    assert np.all(kp.count2delta(mesh, sel)[0] == 0)


# ---- exactness: the restated mean is the peak of the float64 log posterior --------------------------------------------------------------
SHAPE = (16, 12, 8)
CELL = 16.
KS = np.logspace(-3, 1, 128)
KPOW = (KS, 3.0e4 * (KS / 0.02) / (1 + (KS / 0.02) ** 2.6))
FIXED = dict(Omega_m=0.3111, sigma8=0.8102, b1=0.6, ngbars=2. ** -6, s_e=1.0, s_ed=0., s_e2=0.)
RC = FIXED["ngbars"] * CELL ** 3      # 64 counts per cell, a power of two: rc (1 + d) is exact


def _cfg(precond):
    return dict(final_shape=SHAPE, init_shape=SHAPE, cell_length=CELL, box_size=np.multiply(SHAPE, CELL), box_center=np.array([0., 0., 1500.]),
                box_rotvec=np.zeros(3), a_obs=0.7, curved_sky=False, lin_kpow=KPOW, precond=precond, selec_mesh=None, mask_mesh=None)


def _make_cosmo(base):
    return obg.Planck18(Omega_c=base["Omega_m"] - obg.Planck18().Omega_b, sigma8=base["sigma8"])


def _observation():
    """rc (1 + d) with d of EXACTLY zero mean: integers / 1024 that sum to zero (every sum below is exact in float64)."""
    rng = np.random.default_rng(11)
    n = rng.integers(-200, 201, SHAPE)
    n[0, 0, 0] -= n.sum()
    d = n / 1024.
    return RC * (1. + d), d


class FlatKaiser:
    """Float64 flat-sky Kaiser model in sample space, written out: gxy = 1 + irfftn(boost sqrt(P) transfer T(w)), T = rg2cgh or rfftn; the
    'quad_gauss' likelihood with s_ed = s_e2 = 0 (a Gaussian of std s_e sqrt(rc) about rc gxy; the reference's 1e-9 regulariser of the std is
    left out: it would move the noise variance by 2e-9 relative, more than the gate below) and the prior w ~ N(0, scale).  The map is linear, so
    it is held as a dense matrix built column by column: value and gradient are then plain linear algebra, with no hand-derived adjoint."""

    def __init__(self, precond, obs):
        cfg = _cfg(precond)
        fid, cosmo = dict(FIXED), _make_cosmo(FIXED)
        self.scale, transfer = bo.precond_scale_and_transfer(cfg, fid, cosmo)
        self.scale = np.asarray(self.scale, dtype=np.float64).reshape(-1)
        boost = bo.kaiser_boost(cosmo, cfg["a_obs"], SHAPE, cfg["box_size"], 1. + FIXED["b1"], kp.los_fid(cfg))
        mult = boost * bo.lin_power_mesh(FIXED["sigma8"], SHAPE, cfg["box_size"], KPOW) ** .5 * transfer
        to_k = o._rfftn if precond == "real" else o.rg2cgh
        M = int(np.prod(SHAPE))
        self.A = np.empty((M, M))
        e = np.zeros(M)
        for j in range(M):
            e[j] = 1.
            self.A[:, j] = RC * o._irfftn(mult * to_k(e.reshape(SHAPE)), s=SHAPE, axes=(0, 1, 2)).reshape(-1)
            e[j] = 0.
        self.resid0 = (obs - RC).reshape(-1)      # obs - mean counts at w = 0
        self.var = FIXED["s_e"] ** 2 * RC

    def lp(self, w):
        w = w.reshape(-1)
        r = self.resid0 - self.A @ w
        return float(np.sum(-0.5 * np.log(2 * np.pi * self.var) - 0.5 * r ** 2 / self.var)
                     + np.sum(-0.5 * np.log(2 * np.pi) - np.log(self.scale) - 0.5 * (w / self.scale) ** 2))

    def grad(self, w):
        w = w.reshape(-1)
        return self.A.T @ ((self.resid0 - self.A @ w) / self.var) - w / self.scale ** 2

    def delta_lp(self, w, z):
        """lp(w + z) - lp(w), formed from the differences so that the constants cancel exactly."""
        w, z = w.reshape(-1), z.reshape(-1)
        r, Az = self.resid0 - self.A @ w, self.A @ z
        return float(np.sum((r * Az - 0.5 * Az ** 2) / self.var) - np.sum((w * z + 0.5 * z ** 2) / self.scale ** 2))


@pytest.fixture(scope="module")
def observation():
    return _observation()


def _restated_mean(precond, obs):
    return kp.kaiser_post(_cfg(precond), {}, FIXED, obs, np.zeros(SHAPE), _make_cosmo, temp=0.)["white_mesh_"]


def test_inputs_meet_the_conditions_of_exactness(observation):
    obs, d = observation
    cfg = _cfg("kaiser")
    los = kp.los_fid(cfg)
    assert los[0] == 0. and los[1] == 0. and los[2] == 1.      # along z: mu^2 = kz^2 / k^2 is even under k -> -k on every Nyquist plane
    assert d.sum() == 0. and obs.mean() == RC                  # the integral constraint leaves delta_obs = d
    assert np.array_equal(kp.observed_delta(cfg, obs), d)
    assert FIXED["s_e"] == 1. and cfg["selec_mesh"] is None and cfg["final_shape"] == cfg["init_shape"]


def test_restated_mean_is_the_peak_of_the_kaiser_posterior(observation):
    obs, _ = observation
    model = FlatKaiser("kaiser", obs)
    m = _restated_mean("kaiser", obs)
    g0, gm = np.linalg.norm(model.grad(np.zeros(SHAPE))), np.linalg.norm(model.grad(m))
    print(f"kaiser: |grad(mean)| / |grad(0)| = {gm / g0:.3e}")
    assert g0 > 0 and gm <= 1e-9 * g0
    # unit covariance about the mean: lp(m + z) - lp(m) = -|z|^2 / 2
    z = np.random.default_rng(5).standard_normal(SHAPE)
    half = 0.5 * float((z ** 2).sum())
    dev = abs(model.delta_lp(m, z) + half)
    print(f"kaiser: |lp(m + z) - lp(m) + |z|^2 / 2| / (|z|^2 / 2) = {dev / half:.3e}")
    assert dev <= 1e-9 * half
    assert abs((model.lp(m + z) - model.lp(m)) - model.delta_lp(m, z)) <= 1e-9 * half      # delta_lp is the difference of lp


@pytest.mark.parametrize("precond", ["fourier", "real"])
def test_restated_mean_is_the_peak_in_the_other_preconditionings(observation, precond):
    obs, _ = observation
    model = FlatKaiser(precond, obs)
    m = _restated_mean(precond, obs)
    g0, gm = np.linalg.norm(model.grad(np.zeros(SHAPE))), np.linalg.norm(model.grad(m))
    print(f"{precond}: |grad(mean)| / |grad(0)| = {gm / g0:.3e}")
    assert g0 > 0 and gm <= 1e-9 * g0
