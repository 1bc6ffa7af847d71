"""Eulerian bias (bricks.eulerian_bias / eulerian_bias_vjp, FieldLevelForward(bias_type='eulerian')) against the float64 restatement
tests/_eulerian_f64.py.  Gates: those of tests/test_gpu_bias.py (2e-5 relative L2 forward, 2e-4 of the scale of tests/test_gpu_png_model.py for
scalar cotangents) and of tests/test_gpu_model.py (2e-4 forward of evolve; central differences: eps 1e-5 on meshes, 1e-4 on scalars, 3e-3 of
the quotient, 1e-2 for Omega_m)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _eulerian_f64 as ef  # noqa: E402
from oracle import background as obg  # noqa: E402  (checker only)

BIAS = dict(b1=1.1, b2=0.3, bs2=-0.2, b3=0.15, bds2=0.25, bs3=-0.1, bn2=2.0, bnpar=1.5)
PNG = dict(fNL_bp=2.0e4, fNL_bpd=1.0e4)      # phi ~ 2e-5: terms of a few 0.1
UNIT = dict(b1=-1., b2=8 / 21, bs2=0., bn2=0.)      # b1E = b2E = 0 exactly: every coefficient of the expansion vanishes
SHAPES = [((16, 16, 16), (160., 160., 160.)), ((16, 12, 8), (200., 120., 100.)), ((10, 14, 6), (100., 180., 90.)),      # M = 840: ragged
          ((32, 32, 32), (640., 640., 640.))]                                                                        # 128 partial blocks through the fold


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def pair(a, b):
    return float((a.real * b.real + a.imag * b.imag).sum())


def _inputs(shape, with_phi):
    rng = np.random.default_rng(11)
    X = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    X[0, 0, 0] = 0.3 * np.prod(shape)      # a mean that the expansion must drop
    P = np.fft.rfftn(2e-5 * rng.standard_normal(shape)) if with_phi else None
    return rng, X.astype(np.complex64), None if P is None else P.astype(np.complex64)


@pytest.mark.parametrize("with_phi", [False, True])
@pytest.mark.parametrize("shape,box", SHAPES)
def test_eulerian_bias_forward(gpu, shape, box, with_phi):
    """Forward against the restatement on the same complex64 input; the all-zero-coefficient call is w == 1.0 bitwise, and the bias terms
    move w away from it (so the comparison does not pass on a dead branch)."""
    from montecosmo_amd import bricks
    _, X32, P32 = _inputs(shape, with_phi)
    png_type = "bias" if with_phi else None
    w = bricks.eulerian_bias(X32, P32, box, BIAS, PNG, png_type=png_type).cpu().numpy()
    w_o, _ = ef.eulerian_bias(X32, P32, box, ef.l2e(BIAS, PNG if with_phi else None))
    w_one = bricks.eulerian_bias(X32, P32, box, UNIT, {}, png_type=png_type).cpu().numpy()
    assert w.shape == tuple(shape) and w.dtype == np.float32
    assert bool((w_one == 1.0).all())
    e, share = rel_l2(w, w_o), rel_l2(w, w_one)
    print(f"eulerian_bias{shape} phi={with_phi}: rel L2 {e:.3e}; the bias terms change w by {share:.3e}")
    assert share > 1e-3
    assert e < 2e-5


@pytest.mark.parametrize("with_phi", [False, True])
@pytest.mark.parametrize("shape,box", SHAPES)
def test_eulerian_bias_vjp(gpu, shape, box, with_phi):
    """Coefficient cotangents against the restatement's sums; matter / phi spectrum cotangents against central differences of the float64
    restatement (a Hermitian direction and a single interior complex mode); zero-mode cotangent exactly 0; two calls bitwise equal."""
    from montecosmo_amd import bricks
    rng, X32, P32 = _inputs(shape, with_phi)
    png_type = "bias" if with_phi else None
    png = PNG if with_phi else None
    _, ctx = bricks.eulerian_bias(X32, P32, box, BIAS, PNG, png_type=png_type, return_ctx=True)
    wb = rng.standard_normal(shape)
    outs = [bricks.eulerian_bias_vjp(ctx, wb.astype(np.float32)) for _ in range(2)]
    mb, pb, bb, qb = outs[0]
    assert bool((mb == outs[1][0]).all()) and bb == outs[1][2] and qb == outs[1][3], "repeat calls must be bitwise equal"
    assert (pb is None) == (not with_phi) and (qb is None) == (not with_phi)
    if with_phi:
        assert bool((pb == outs[1][1]).all())
    mbn = mb.cpu().numpy().astype(np.complex128)
    assert mbn[0, 0, 0] == 0
    assert bb["b3"] == 0.0 and bb["bds2"] == 0.0 and bb["bs3"] == 0.0 and bb["bnpar"] == 0.0
    # coefficients: w is linear in coef, so the cotangents are the sums of the restatement's factors, chained to the Lagrangian parameters
    terms = ef.eulerian_terms(X32, P32, box)
    cb = [float((wb * t).sum()) for t in terms]
    scale = [max(abs(c), np.abs(wb).sum() * np.abs(t).max() * 1e-2) for c, t in zip(cb, terms)]
    # (a chained cotangent inherits the bounds of its two parts, with the chain rule's weights)
    want = {"b1": (cb[0] + 8 / 21 * cb[1], scale[0] + 8 / 21 * scale[1]), "b2": (cb[1], scale[1]), "bs2": (cb[2], scale[2]), "bn2": (cb[3], scale[3])}
    got = dict(bb)
    if with_phi:
        want.update({"fNL_bp": (cb[4] + cb[5] / 2, scale[4] + scale[5] / 2), "fNL_bpd": (cb[5], scale[5])})
        got.update(qb)
    for k, (v, s) in want.items():
        print(k, got[k], v)
        assert abs(got[k] - v) < 2e-4 * s, (k, got[k], v)
    X64 = X32.astype(np.complex128)
    P64 = None if P32 is None else P32.astype(np.complex128)
    coef = ef.l2e(BIAS, png)
    L = lambda X_, P_: float((wb * ef.eulerian_bias(X_, P_, box, coef)[0]).sum())
    dH = np.fft.rfftn(rng.standard_normal(shape))
    d1 = np.zeros_like(X64)
    d1[2, 3, 1] = 0.7 - 1.3j
    eps = 1e-5
    for tag, d in (("hermitian", dH / 40.), ("single mode", d1)):
        dX = d * np.abs(X64).mean()
        fd = (L(X64 + eps * dX, P64) - L(X64 - eps * dX, P64)) / (2 * eps)
        an = pair(mbn, dX)
        print("matter_k", tag, fd, an)
        assert abs(fd - an) < 3e-3 * abs(fd), ("matter_k", tag, fd, an)
        if with_phi:
            dP = d * np.abs(P64).mean()
            fd = (L(X64, P64 + eps * dP) - L(X64, P64 - eps * dP)) / (2 * eps)
            an = pair(pb.cpu().numpy().astype(np.complex128), dP)
            print("phi_k", tag, fd, an)
            assert abs(fd - an) < 3e-3 * abs(fd), ("phi_k", tag, fd, an)


def _kpow():
    ks = np.logspace(-3, 1, 128)
    return ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6)


MBIAS = dict(b1=0.8, b2=0.2, bs2=-0.15, b3=0.1, bds2=0.1, bs3=-0.05, bn2=20.0, bnpar=5.0)
MPNG = dict(fNL=300., fNL_bp=3.0, fNL_bpd=-2.0, fNL_bpd2=-20., fNL_bps2=30., fNL_bn2p=2.0e3)


def _model_kw(evolution, a_obs, curved):
    # final (8, 8, 8); every oversampling 2 except init 1.5, so that init_shape != paint_shape and the paint Jacobian matters
    return dict(final_shape=(8, 8, 8), cell_length=40., box_center=(60., -40., 1400.), box_rotvec=(0.1, 0.2, -0.1), evolution=evolution,
                nbody_n_steps=3, lpt_order=2, init_oversamp=1.5, evol_oversamp=2., ptcl_oversamp=2., paint_oversamp=2., a_obs=a_obs,
                curved_sky=curved, lin_kpow=_kpow(), nbody_a_start=0.1)


@pytest.mark.parametrize("png_type", [None, "bias"])
@pytest.mark.parametrize("evolution,a_obs,curved", [("lpt", 0.6, False), ("lpt", None, True), ("nbody", 0.7, True)])
def test_evolve_eulerian(gpu, evolution, a_obs, curved, png_type):
    """evolve with bias_type='eulerian' against the restated float64 evolve; evolve_vjp + cosmo_vjp against central differences of the
    float64 chain; b3, bds2, bs3 are not read; bias_type='lagrangian' is bitwise the model built without the argument."""
    from montecosmo_amd import bricks, model
    rng = np.random.default_rng(31)
    kw = _model_kw(evolution, a_obs, curved)
    fwd = model.FieldLevelForward(png_type=png_type, bias_type="eulerian", **kw)
    cfg = fwd.config()
    cosmo, cosmo_o = bricks.Planck18(), obg.Planck18()
    cosmo_o.sigma8 = cosmo.sigma8
    white = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * (12 ** 3 / np.prod(cfg["box_size"])) ** .5
    w32 = white.astype(np.complex64)
    pkw = {} if png_type is None else {"png": MPNG}
    g_lag = model.FieldLevelForward(png_type=png_type, **kw).evolve(cosmo, MBIAS, w32, **pkw)
    g_lag2 = model.FieldLevelForward(png_type=png_type, bias_type="lagrangian", **kw).evolve(cosmo, MBIAS, w32, **pkw)
    assert bool((g_lag == g_lag2).all())
    gxy, ctx = fwd.evolve(cosmo, MBIAS, w32, return_ctx=True, **pkw)
    assert tuple(gxy.shape) == tuple(cfg["paint_shape"])
    ref = ef.evolve(cfg, cosmo_o, MBIAS, white, MPNG, png_type)
    e, share = rel_l2(gxy.cpu().numpy(), ref), rel_l2(ref, g_lag.cpu().numpy())
    print(f"evolve[{evolution} {a_obs} {png_type}] eulerian rel L2 {e:.3e}; differs from the Lagrangian output by {share:.3e}")
    assert share > 1e-3
    assert e < 2e-4
    gb = rng.standard_normal(gxy.shape)
    grads = fwd.evolve_vjp(ctx, gb.astype(np.float32))

    def L(white_=white, bias=MBIAS, png=MPNG, dom=0.):
        c = obg.Planck18(Omega_c=cosmo.Omega_c + dom)
        c.sigma8 = cosmo.sigma8
        return float((gb * ef.evolve(cfg, c, bias, white_, png, png_type)).sum())
    for k in ("b1", "b2", "bs2", "bn2"):
        h = 1e-4 * max(1.0, abs(MBIAS[k]))
        fd = (L(bias=dict(MBIAS, **{k: MBIAS[k] + h})) - L(bias=dict(MBIAS, **{k: MBIAS[k] - h}))) / (2 * h)
        print(k, fd, grads["bias"][k])
        assert abs(fd - grads["bias"][k]) < 3e-3 * abs(fd), (k, fd, grads["bias"][k])
    for k in ("b3", "bds2", "bs3"):
        assert grads["bias"][k] == 0.0, (k, grads["bias"][k])
    if png_type is not None:
        for k in ("fNL_bp", "fNL"):
            h = 1e-4 * abs(MPNG[k])
            fd = (L(png=dict(MPNG, **{k: MPNG[k] + h})) - L(png=dict(MPNG, **{k: MPNG[k] - h}))) / (2 * h)
            print(k, fd, grads["png"][k])
            assert abs(fd - grads["png"][k]) < 3e-3 * abs(fd), (k, fd, grads["png"][k])
    eps = 1e-5
    dW = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * np.abs(white).mean() / 40.
    fd = (L(white_=white + eps * dW) - L(white_=white - eps * dW)) / (2 * eps)
    an = pair(grads["white_mesh"].cpu().numpy().astype(np.complex128), dW)
    print("white_mesh", fd, an)
    assert abs(fd - an) < 3e-3 * abs(fd), ("white_mesh", fd, an)
    h = 1e-4
    got = fwd.cosmo_vjp(ctx, grads, params=("Omega_m",))["Omega_m"]
    fdo = (L(dom=h) - L(dom=-h)) / (2 * h)
    print("Omega_m", fdo, got)
    assert abs(fdo - got) < 1e-2 * abs(fdo), ("Omega_m", fdo, got)


@pytest.mark.parametrize("png_type", [None, "bias"])
def test_kaiser_ignores_bias_type(gpu, png_type):
    """evolution='kaiser' never consults bias_type (model.py:690-696): bitwise the same mesh."""
    from montecosmo_amd import bricks, model
    rng = np.random.default_rng(33)
    kw = dict(_model_kw("kaiser", 0.65, False), png_type=png_type)
    white = (np.fft.rfftn(rng.standard_normal((12, 12, 12))) * (12 ** 3 / (8 * 40.) ** 3) ** .5).astype(np.complex64)
    pkw = {} if png_type is None else {"png": MPNG}
    a = model.FieldLevelForward(bias_type="eulerian", **kw).evolve(bricks.Planck18(), MBIAS, white, **pkw)
    b = model.FieldLevelForward(bias_type="lagrangian", **kw).evolve(bricks.Planck18(), MBIAS, white, **pkw)
    assert bool((a == b).all())


def test_evolve_eulerian_off_lattice_particles(gpu):
    """ptcl_shape != evol_shape: phi is READ at the Lagrangian lattice (NGP) and its cotangent painted back, instead of the identity."""
    from montecosmo_amd import bricks, model
    rng = np.random.default_rng(35)
    kw = dict(_model_kw("lpt", 0.6, False), ptcl_oversamp=1.5)
    fwd = model.FieldLevelForward(png_type="bias", bias_type="eulerian", **kw)
    cfg = fwd.config()
    assert tuple(cfg["ptcl_shape"]) != tuple(cfg["evol_shape"])
    cosmo, cosmo_o = bricks.Planck18(), obg.Planck18()
    cosmo_o.sigma8 = cosmo.sigma8
    white = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * (12 ** 3 / np.prod(cfg["box_size"])) ** .5
    gxy, ctx = fwd.evolve(cosmo, MBIAS, white.astype(np.complex64), png=MPNG, return_ctx=True)
    e = rel_l2(gxy.cpu().numpy(), ef.evolve(cfg, cosmo_o, MBIAS, white, MPNG, "bias"))
    print(f"evolve eulerian, ptcl != evol: rel L2 {e:.3e}")
    assert e < 2e-4
    gb = rng.standard_normal(gxy.shape)
    grads = fwd.evolve_vjp(ctx, gb.astype(np.float32))
    L = lambda png: float((gb * ef.evolve(cfg, cosmo_o, MBIAS, white, png, "bias")).sum())
    h = 1e-4 * MPNG["fNL"]      # fNL reaches the output through the advected phi as well: the read's adjoint is on this path
    fd = (L(dict(MPNG, fNL=MPNG["fNL"] + h)) - L(dict(MPNG, fNL=MPNG["fNL"] - h))) / (2 * h)
    print("fNL", fd, grads["png"]["fNL"])
    assert abs(fd - grads["png"]["fNL"]) < 3e-3 * abs(fd), ("fNL", fd, grads["png"]["fNL"])


def test_log_density_eulerian(gpu):
    """FieldLevelLogDensity on an Eulerian model: logdensity_and_grad runs, is finite, and three calls are bitwise equal."""
    import torch
    from montecosmo_amd import model, logdensity
    rng = np.random.default_rng(41)
    fwd = model.FieldLevelForward(png_type="fNL", bias_type="eulerian", **_model_kw("nbody", 0.65, True))
    lat = {"fNL": dict(loc=0., scale=1e3, loc_fid=200., scale_fid=50.),
           "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2), "b2": dict(loc=0., scale=1e2, loc_fid=0.2, scale_fid=3e-2)}
    fixed = dict(Omega_m=0.3111, sigma8=0.8102, bs2=-0.15, bn2=20., bnpar=5., b3=0.1, bds2=0.1, bs3=-0.05, ngbars=1e-3, s_e=1.0, s_ed=0.1,
                 s_e2=0.02, fNL_bpd2=-20., fNL_bps2=30., fNL_bn2p=2.0e3)
    sample = {k + "_": float(rng.normal(0, 1.0)) for k in lat}
    sample["white_mesh_"] = rng.standard_normal((12, 12, 12)).astype(np.float32)
    obs = 64. + 8. * rng.standard_normal((8, 8, 8))
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="fourier")
    runs = [ld.logdensity_and_grad(sample) for _ in range(3)]
    lp, grad = runs[0]
    assert np.isfinite(lp) and all(np.isfinite(grad[k + "_"]) for k in lat) and bool(torch.isfinite(grad["white_mesh_"]).all())
    assert any(grad[k + "_"] != 0. for k in lat) and bool((grad["white_mesh_"] != 0).any())
    for lp2, grad2 in runs[1:]:
        assert lp == lp2 and all(grad[k + "_"] == grad2[k + "_"] for k in lat) and bool((grad["white_mesh_"] == grad2["white_mesh_"]).all())
