"""Primordial non-Gaussianity, host side (no GPU): the phi -> delta transfer table, the bias reparametrisation and its VJP, and
two identities of the float64 restatement (tests/_png_f64.py) that the GPU tests lean on."""
import numpy as np
import pytest

import _png_f64 as pf
from oracle import pm_oracle as o, power_oracle as po


@pytest.fixture(scope="module")
def bricks():
    from montecosmo_amd import bricks
    return bricks


@pytest.mark.parametrize("tabulated", [False, True], ids=["eisenstein_hu", "lin_kpow"])
def test_transfer_table_closed_form_low_k_and_sigma8(bricks, tabulated):
    cosmo = bricks.Planck18()
    kpow = po.lin_power_table(cosmo) if tabulated else None
    a = 0.7
    ks, trans = bricks.trans_phi2delta_table(cosmo, a=a, kpow=kpow)
    assert ks.shape == trans.shape == (256,) and ks.dtype == trans.dtype == np.float64
    np.testing.assert_allclose(ks, np.logspace(-4, 1, 256), rtol=1e-14)
    # at ks[0] the normalised transfer function is 1 by construction: trans = 2 rh^2 k^2 D(a) / D_md / (3 Omega_m)
    a_md = 1. / 11.
    closed = 2. * 2997.92458 ** 2 * ks[0] ** 2 * (o.a2g(cosmo, a) / (o.a2g(cosmo, a_md) / a_md)) / (3. * cosmo.Omega_m)
    assert abs(trans[0] - closed) < 1e-12 * closed
    # low k: T(k) -> 1, so trans ~ k^2 (Eisenstein & Hu: 1 - T = O((k / k_eq)^2), 1e-3 at k = 3e-4 h/Mpc)
    low = ks < 3e-4
    assert low.sum() > 10
    assert np.abs(trans[low] / ks[low] ** 2 / (trans[0] / ks[0] ** 2) - 1.).max() < 2e-3
    # the restatement (oracle power table and growth) agrees: the two growth tables and EH fits differ at the 1e-6 level
    ks_o, trans_o = pf.trans_table(cosmo, a=a, kpow=kpow)
    assert np.abs(trans / trans_o - 1.).max() < 1e-5
    # sigma8 only rescales the power, which enters through a ratio
    ks2, trans2 = bricks.trans_phi2delta_table(bricks.Planck18(sigma8=0.6), a=a, kpow=kpow)
    assert np.array_equal(trans, trans2) and np.array_equal(ks, ks2)
    # a = 1 default, and D(a) scaling
    _, trans1 = bricks.trans_phi2delta_table(cosmo, kpow=kpow)
    np.testing.assert_allclose(trans / trans1, o.a2g(cosmo, a) / o.a2g(cosmo, 1.), rtol=1e-12)


def test_bias_reparametrisation_algebra(bricks):
    dc = 1.686
    assert bricks.b_phi(1.0) == pytest.approx(2 * dc * 1.0)               # p = 1: 2 dc b1
    assert bricks.b_phi(1.0, p=1.6) == pytest.approx(2 * dc * 0.4)
    assert bricks.b_phi_delta(1.0, 0.5) == pytest.approx(2 * (dc * 0.5 - 1.0))
    assert bricks.bpd_L2E(0.7, 0.4) == pytest.approx(0.9) and bricks.bpd_E2L(bricks.bpd_L2E(0.7, 0.4), 0.4) == pytest.approx(0.7)
    png = dict(fNL=30., fNL_bp=1.5, fNL_bpd=-0.5, fNL_bpd2=0.2, fNL_bps2=0.1, fNL_bn2p=3.)
    bias = dict(b1=1.1, b2=0.3)
    for png_type in (None, "fNL", "bias"):
        got, want = bricks.fNL_bias(png, bias, p=1.2, png_type=png_type), pf.fNL_bias(png, bias, p=1.2, png_type=png_type)
        assert set(got) == set(want)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-15), (png_type, k)
    f = bricks.fNL_bias(png, bias, png_type="fNL")
    assert f["fNL_bp"] == pytest.approx(30. * 2 * dc * 1.1) and f["fNL_bpd"] == pytest.approx(30. * 2 * (dc * 0.3 - 1.1))
    b = bricks.fNL_bias(png, bias, png_type="bias")
    assert b["fNL_bp"] == pytest.approx(45.) and b["fNL_bpd"] == pytest.approx(-15.) and b["fNL_bpd2"] == 0.2
    assert png["fNL_bp"] == 1.5                                           # the input dict is not modified
    assert bricks.fNL_bias(dict(fNL=2.), bias, png_type="bias")["fNL_bp"] == 0.     # missing keys are 0
    with pytest.raises(ValueError):
        bricks.fNL_bias(png, bias, png_type="nope")


@pytest.mark.parametrize("png_type", [None, "fNL", "bias"])
def test_fNL_bias_vjp_against_central_differences(bricks, png_type):
    rng = np.random.default_rng(3)
    png = dict(fNL=30., fNL_bp=1.5, fNL_bpd=-0.5, fNL_bpd2=0.2, fNL_bps2=0.1, fNL_bn2p=3.)
    bias = dict(b1=1.1, b2=0.3)
    bar = {k: float(rng.standard_normal()) for k in pf.PNG_KEYS}
    L = lambda pg, bs: sum(bar[k] * v for k, v in bricks.fNL_bias(pg, bs, p=1.3, png_type=png_type).items())
    png_bar, bias_bar = bricks.fNL_bias_vjp(png, bias, bar, p=1.3, png_type=png_type)
    for k in pf.PNG_KEYS:
        h = 1e-5 * max(abs(png[k]), 1.)
        fd = (L(dict(png, **{k: png[k] + h}), bias) - L(dict(png, **{k: png[k] - h}), bias)) / (2 * h)
        assert abs(fd - png_bar[k]) < 1e-8 * max(abs(fd), 1.), (k, fd, png_bar[k])
    for k in ("b1", "b2"):
        h = 1e-5
        fd = (L(png, dict(bias, **{k: bias[k] + h})) - L(png, dict(bias, **{k: bias[k] - h}))) / (2 * h)
        assert abs(fd - bias_bar[k]) < 1e-8 * max(abs(fd), 1.), (k, fd, bias_bar[k])


@pytest.mark.parametrize("shape,box", [((16, 16, 16), (160., 160., 160.)), ((16, 12, 8), (200., 120., 100.))])
def test_restatement_identities(shape, box):
    """add_png(fNL = 0) returns the field (without its k = 0 mode, where t = 0), and the quadratic term leaves <phi> alone."""
    rng = np.random.default_rng(5)
    cosmo = o_cosmo()
    table = pf.trans_table(cosmo)
    lin = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    lin[0, 0, 0] = 0.
    out0 = pf.add_png(table, 0., lin, box)
    assert np.linalg.norm(out0 - lin) < 1e-13 * np.linalg.norm(lin)
    out, phi0 = pf.add_png(table, -500., lin, box, return_phi=True)
    t = pf.trans_mesh(table, shape, box)
    phi_nl = np.fft.irfftn(o.safe_div(out, t), s=shape, axes=(0, 1, 2))
    assert abs(phi_nl.mean() - phi0.mean()) < 1e-14 * np.abs(phi0).max()
    assert np.linalg.norm(out - lin) > 1e-3 * np.linalg.norm(lin)        # ... while the field itself has changed
    assert out[0, 0, 0] == 0.


def o_cosmo():
    from oracle import background
    return background.Planck18()
