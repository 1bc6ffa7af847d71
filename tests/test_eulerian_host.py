"""CPU-side checks of the Eulerian bias expansion: known answers and the dot test of the float64 restatement tests/_eulerian_f64.py (the
checker of tests/test_gpu_eulerian.py), the Lagrangian -> Eulerian conversions, the `bias_type` switch of the model and of the register
files, and the two new entry points in the header and the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _eulerian_f64 as ef
from montecosmo_amd import bricks, model, register

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2E = (bricks.b1_L2E, bricks.b2_L2E, bricks.bpd_L2E)      # (the conversions this module's known answers go through)
BIAS = dict(b1=0.7, b2=-0.4, bs2=0.3, b3=0.2, bds2=-0.1, bs3=0.15, bn2=12.0, bnpar=3.0)


def pair(a, b):
    return float((a.real * b.real + a.imag * b.imag).sum())


def with_mean(X, value):
    """X with `value` added to its zero mode (which eulerian_bias must drop)."""
    X = np.array(X)
    X[0, 0, 0] += value
    return X


def test_l2e_conversions():
    b1, b2 = BIAS["b1"], BIAS["b2"]
    assert L2E[0](b1) == 1 + b1 and bricks.b1_E2L(L2E[0](b1)) == pytest.approx(b1, abs=1e-15)
    assert L2E[1](b2, b1) == b2 + 8 / 21 * b1 and bricks.b2_E2L(L2E[1](b2, b1), b1) == pytest.approx(b2, abs=1e-15)
    coef = ef.l2e(BIAS, {"fNL_bp": 3.0, "fNL_bpd": -2.0})
    assert coef == (L2E[0](b1), L2E[1](b2, b1), BIAS["bs2"], BIAS["bn2"], 3.0, L2E[2](-2.0, 3.0))
    assert L2E[1](8 / 21, -1.) == 0.0      # the bitwise known answer of the GPU test: b1E = b2E = 0 exactly


@pytest.mark.parametrize("mode", [(2, 0, 0), (0, 3, 0), (0, 0, 1), (1, 1, 1), (2, -1, 1)])
def test_plane_wave_known_answer(mode):
    """d = eps cos(k . x): the shear of a plane wave is (khat khat - 1/3) d, so s^2 = 2/3 d^2, lap d = -k^2 d, <d^2> = eps^2 / 2 and
    w = 1 + b1E d + (b2E / 2 + 2/3 bs2) (d^2 - eps^2 / 2) - bn2 k^2 d."""
    shape, box, eps = (16, 12, 8), (200., 120., 100.), 0.3
    x = np.meshgrid(*[np.arange(n) / n for n in shape], indexing="ij")
    d = eps * np.cos(2 * np.pi * sum(m * xi for m, xi in zip(mode, x)) + 0.4)
    k2 = sum((2 * np.pi * m / b) ** 2 for m, b in zip(mode, box))
    coef = ef.l2e(BIAS)
    w, (sigma2, spd) = ef.eulerian_bias(with_mean(np.fft.rfftn(d), 5.0 * d.size), None, box, coef)
    f, _ = ef.fields(np.fft.rfftn(d), None, box)
    assert np.abs(ef._shear(f, np.float64)[3] - 2 / 3 * d ** 2).max() < 1e-12
    assert np.abs(f[6] + k2 * d).max() < 1e-12 * max(1., k2)
    want = 1 + coef[0] * d + (coef[1] / 2 + 2 / 3 * coef[2]) * (d ** 2 - eps ** 2 / 2) - coef[3] * k2 * d
    assert abs(sigma2 - eps ** 2 / 2) < 1e-14 and spd == 0.
    assert np.abs(w - want).max() < 1e-12


@pytest.mark.parametrize("shape,box", [((10, 14, 6), (100., 180., 90.)), ((8, 8, 8), (80., 80., 80.))])
@pytest.mark.parametrize("with_phi", [False, True])
def test_restatement_vjp_dot(shape, box, with_phi):
    """The hand VJP against central differences of the restatement itself (w is quadratic in the spectra: the quotient is exact up to
    rounding), for a Hermitian direction and a single interior complex mode; the coefficient cotangents are the sums of the factors."""
    rng = np.random.default_rng(5)
    X = with_mean(np.fft.rfftn(0.4 * rng.standard_normal(shape)), 3.0)
    P = np.fft.rfftn(2e-5 * rng.standard_normal(shape)) if with_phi else None
    coef = ef.l2e(BIAS, {"fNL_bp": 2.0e4, "fNL_bpd": 1.0e4})
    wb = rng.standard_normal(shape)
    Xb, Pb, cb = ef.eulerian_bias_vjp(X, P, box, coef, wb)
    assert Xb[0, 0, 0] == 0 and (Pb is None) == (not with_phi)
    L = lambda X_, P_=P, c=coef: float((wb * ef.eulerian_bias(X_, P_, box, c)[0]).sum())
    d1 = np.zeros_like(X)
    d1[2, 3, 1] = 0.7 - 1.3j
    for d in (np.fft.rfftn(rng.standard_normal(shape)), d1):
        eps = 1e-3
        fd = (L(X + eps * d) - L(X - eps * d)) / (2 * eps)
        assert abs(fd - pair(Xb, d)) < 1e-7 * abs(fd), (fd, pair(Xb, d))
        if with_phi:
            dp = 1e-4 * d
            fd = (L(X, P + eps * dp) - L(X, P - eps * dp)) / (2 * eps)
            assert abs(fd - pair(Pb, dp)) < 1e-7 * abs(fd), (fd, pair(Pb, dp))
    for k in range(6 if with_phi else 4):
        e = np.zeros(6)
        e[k] = 1.
        fd = (L(X, c=tuple(np.add(coef, e))) - L(X, c=tuple(np.subtract(coef, e)))) / 2
        assert abs(fd - cb[k]) < 1e-7 * max(abs(fd), 1e-3), (k, fd, cb[k])
    # the single-precision mode is the same arithmetic: it stays within float32 rounding of the float64 run
    w64, w32 = ef.eulerian_bias(X, P, box, coef)[0], ef.eulerian_bias(X, P, box, coef, dtype=np.float32)[0]
    assert np.linalg.norm(w32 - w64) < 1e-5 * np.linalg.norm(w64)


def test_bias_type_switch_and_register(tmp_path):
    kw = dict(final_shape=(8, 8, 8), cell_length=40.)
    assert model.FieldLevelForward(**kw).bias_type == "lagrangian" and model.FieldLevelForward(**kw).config()["bias_type"] == "lagrangian"
    assert model.FieldLevelForward(bias_type="eulerian", **kw).config()["bias_type"] == "eulerian"
    assert model.FieldLevelForward(bias_type="eulerian", evolution="kaiser", **kw).bias_type == "eulerian"      # accepted, and ignored
    for bad in ("Eulerian", None, "", 1):
        with pytest.raises(ValueError, match="bias_type"):
            model.FieldLevelForward(bias_type=bad, **kw)
    with pytest.raises(ValueError, match="png_type"):
        bricks.eulerian_bias(np.zeros((4, 4, 3), np.complex64), None, (1., 1., 1.), {}, {}, png_type="fnl")
    reg = dict(cell_length=40., box_center=np.array([0., 0., 900.]), box_rotvec=np.zeros(3), init_oversamp=1.5, paint_oversamp=2.,
               cosmo_fid=dict(Omega_m=0.31, sigma8=0.81), count_mesh=np.ones((8, 8, 8)))
    assert "bias_type" not in register.model_arguments(reg)["forward"]
    assert "bias_type" not in register.model_arguments(dict(reg, bias_type=None))["forward"]
    for value in ("eulerian", "lagrangian"):
        path = register.save_register(str(tmp_path / f"reg_{value}.npz"), dict(reg, bias_type=value))
        args = register.model_arguments(register.load_register(path))
        assert args["forward"]["bias_type"] == value
        assert model.FieldLevelForward(**args["forward"]).bias_type == value
    assert model.FieldLevelForward(**register.model_arguments(register.load_register(
        register.save_register(str(tmp_path / "reg.npz"), reg)))["forward"]).bias_type == "lagrangian"
    with pytest.raises(ValueError, match="bias_type"):
        model.FieldLevelForward(**register.model_arguments(dict(reg, bias_type="euler"))["forward"])


def test_new_symbols_declared_and_exported():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("mcpm_eulerian_bias_f32", "mcpm_eulerian_bias_vjp_f32"):
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.lib.mcpm_eulerian_bias_f32(None, *([None] * 2), 1., 1., 1., *([None] * 4)) == -6      # MCPM_E_ARG, no crash
    assert _lib.lib.mcpm_version() == b"mcpm 0.12 (gfx950)"      # two symbols added, nothing changed: the ABI string stays
