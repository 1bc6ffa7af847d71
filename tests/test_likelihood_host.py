"""The 'shash', 'poisson' and 'fourier_gauss' likelihoods without a GPU: the ABI of the cross-compiled library, the float64 restatement
(tests/_lik_f64.py) against what is known without it, and the argument checks of FieldLevelLogDensity that come before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import _lik_f64 as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mcpm_lik_real_f32", "mcpm_lik_fourier_f32")


def test_abi_symbols_exported_and_declared():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(mcpm_plan \*plan," % name, header), name
        assert getattr(raw, name) is not None
    assert _lib.lib.mcpm_version().decode() == _lib.ABI_VERSION
    assert "MCPM_LIK_SHASH %d" % _lib.LIK_SHASH in header and "MCPM_LIK_POISSON %d" % _lib.LIK_POISSON in header


def test_restatement_self_checks():
    """SinhArcsinh(skewness 0, tailweight 1) is Normal; the density integrates to 1 with mean loc and standard deviation scale at
    (skew, tail) = (+-0.35, 1.06); |cgh2rg(rfftn x)| = |x| at (4, 6, 8); every hand-written gradient of the restatement against float64
    central differences."""
    assert L.self_check()


def test_shash_reduces_to_the_normal_of_quad_gauss():
    from oracle import bias_oracle as bo
    rng = np.random.default_rng(2)
    obs, count, selec = rng.uniform(30., 100., 64), rng.uniform(40., 90., 64), rng.uniform(50., 80., 64)
    c = L.shash_cells(obs, count, selec, 0.9, 0.4, 0.0)
    P = L.shash_params(count, selec, 0.9, 0.4, 0.0)
    assert np.allclose(c["lp"], bo.quad_gaussian_log_prob(obs, count, P["b"], 0.0), rtol=0, atol=1e-12)


def test_samples_have_the_stated_moments():
    rng = np.random.default_rng(3)
    x = L.shash_sample(rng, np.full(400000, 5.), 2., 0.35, 1.06)
    assert abs(x.mean() - 5.) < 0.02 and abs(x.std() - 2.) < 0.02      # 4 sigma of the sample mean is 0.013


class _Fwd:
    """Stands in for FieldLevelForward up to the argument checks (they run before any geometry or device work)."""
    final_shape = init_shape = (8, 8, 8)
    png_type = None


def _args():
    lat = {"b1": dict(loc=1., scale=1., loc_fid=1., scale_fid=1e-2)}
    fixed = dict(Omega_m=0.3, sigma8=0.8, b2=0., bs2=0., b3=0., bds2=0., bs3=0., bn2=0., bnpar=0., ngbars=1e-3, s_e=1., s_ed=0., s_e2=0.)
    return lat, fixed


def test_unknown_lik_type_and_fourier_with_mask_raise():
    from montecosmo_amd import logdensity
    lat, fixed = _args()
    with pytest.raises(ValueError, match="likelihood"):
        logdensity.FieldLevelLogDensity(_Fwd(), np.zeros((8, 8, 8)), lat, fixed, lik_type="student")
    with pytest.raises(ValueError, match="cut-sky"):
        logdensity.FieldLevelLogDensity(_Fwd(), np.zeros((8, 8, 8)), lat, fixed, lik_type="fourier_gauss", mask_mesh=np.ones((8, 8, 8), bool))
    with pytest.raises(ValueError, match="selection"):
        logdensity.FieldLevelLogDensity(_Fwd(), np.zeros((8, 8, 8)), lat, fixed, lik_type="fourier_gauss", selec_mesh=np.ones((8, 8, 8)))
    fixed.pop("s_e2")      # 'shash' reads it
    with pytest.raises(ValueError, match="s_e2"):
        logdensity.FieldLevelLogDensity(_Fwd(), np.zeros((8, 8, 8)), lat, fixed, lik_type="shash")


def test_register_passes_lik_type_to_the_density_arguments():
    from montecosmo_amd import register
    reg = dict(count_mesh=np.ones((8, 8, 8)), cell_length=10., box_center=(0., 0., 500.), box_rotvec=(0., 0., 0.), init_oversamp=1.,
               paint_oversamp=1., cosmo_fid=dict(Omega_m=0.3, sigma8=0.8))
    plain = register.model_arguments(dict(reg))
    assert "lik_type" not in plain["density"] and "lik_type" not in plain["forward"]
    got = register.model_arguments(dict(reg), lik_type="shash", evolution="lpt")
    assert got["density"]["lik_type"] == "shash" and "lik_type" not in got["forward"] and got["forward"]["evolution"] == "lpt"
