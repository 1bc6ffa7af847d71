"""tests/_bias_f64.py is a reference only if it is right: the restatement against the oracle's lagrangian_bias on identity reads, every
hand-written gradient against float64 central differences, and the general-shape mesh formulas against the oracle (which takes odd nx, ny
as they are) and against tests/_png_f64.py.  CPU only."""
import numpy as np
import pytest

import _bias_f64 as bf
import _png_f64 as pf
from oracle import pm_oracle as o, bias_oracle as bo

BIAS8 = (1.1, 0.3, -0.2, 0.15, 0.25, -0.1, 2.0, 1.5)
PNG5 = (0.7, -0.4, 0.3, 0.2, -1.2)


def _reads(rng, n):
    return [rng.standard_normal(n) for _ in range(4)] + [rng.standard_normal((n, 3))]


@pytest.mark.parametrize("per_particle", [False, True])
def test_against_the_oracle_on_identity_reads(per_particle):
    shape, box = (8, 8, 8), (80., 100., 120.)
    rng = np.random.default_rng(3)
    X = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    pos = o.regular_pos(shape)
    n = len(pos)
    g = (0.4 + 0.5 * rng.uniform(size=(n, 1))) if per_particle else 0.7
    fld, _ = bo.bias_fields(X, box)
    reads = [fld[k].reshape(-1) for k in ("delta", "shear2", "shear3", "nab2")] + [np.stack([f.reshape(-1) for f in fld["grad"]], axis=-1)]
    bias = dict(zip(bo.BIAS_KEYS, BIAS8))
    w, dvel, sigma2 = bf.bias_weights(*reads, g, BIAS8)
    w_o, dv_o = bo.lagrangian_bias(g, pos, box, X, bias, 1)
    assert np.allclose(w, w_o, rtol=0, atol=1e-13 * np.abs(w_o).max()) and np.allclose(dvel, dv_o, rtol=0, atol=1e-13 * np.abs(dv_o).max())
    assert abs(sigma2 - ((reads[0] * np.reshape(g, -1)) ** 2).mean()) < 1e-15
    wb, vb = rng.standard_normal(n), rng.standard_normal((n, 3))
    *_, gbar, bbar, gsum = bf.bias_weights_vjp(*reads, g, BIAS8, wb, vb)
    _, bb_o, gb_o = bo.lagrangian_bias_vjp(g, pos, box, X, bias, wb, vb, 1)
    for i, k in enumerate(bo.BIAS_KEYS):
        assert abs(bbar[i] - bb_o[k]) < 1e-12 * max(abs(v) for v in bb_o.values()), k
    if per_particle:
        assert np.allclose(gbar, gb_o.reshape(-1), rtol=0, atol=1e-12 * np.abs(gb_o).max())
    else:
        assert abs(gsum - float(gb_o)) < 1e-12 * abs(float(gb_o))
    # the mesh side of the restatement, same input
    f7, h6 = bf.bias_fields(X, box)
    want = [fld["delta"], fld["shear2"], fld["shear3"], fld["nab2"]] + list(fld["grad"])
    assert all(np.abs(a - b).max() < 1e-12 * np.abs(b).max() for a, b in zip(f7, want))


def _fd(f, x, d, eps):
    return (f(x + eps * d) - f(x - eps * d)) / (2 * eps)


@pytest.mark.parametrize("per_particle", [False, True])
@pytest.mark.parametrize("n", [1, 37])
def test_bias_weights_vjp_against_central_differences(n, per_particle):
    rng = np.random.default_rng(5)
    reads = _reads(rng, n)
    g = (0.4 + 0.5 * rng.uniform(size=n)) if per_particle else 0.7
    wb, vb = rng.standard_normal(n), rng.standard_normal((n, 3))
    L = lambda r, g_=g, b=BIAS8: (lambda w, dv, _: float((w * wb).sum() + (dv * vb).sum()))(*bf.bias_weights(*r, g_, b))
    drb, s2rb, s3rb, lrb, grb, gbar, bbar, gsum = bf.bias_weights_vjp(*reads, g, BIAS8, wb, vb)
    eps = 1e-6
    for i, bar in enumerate((drb, s2rb, s3rb, lrb, grb)):
        d = rng.standard_normal(reads[i].shape)
        fd = _fd(lambda x: L(reads[:i] + [x] + reads[i + 1:]), reads[i], d, eps)
        assert abs(fd - (bar * d).sum()) < 1e-7 * max(abs(fd), np.linalg.norm(bar) * np.linalg.norm(d)), (i, fd, (bar * d).sum())
    for i in range(8):
        e = np.eye(8)[i]
        fd = _fd(lambda b: L(reads, b=tuple(b)), np.array(BIAS8), e, eps)
        assert abs(fd - bbar[i]) < 1e-7 * max(abs(fd), 1.), (i, fd, bbar[i])
    if per_particle:
        d = rng.standard_normal(n)
        fd = _fd(lambda x: L(reads, g_=x), g, d, eps)
        assert abs(fd - (gbar * d).sum()) < 1e-7 * max(abs(fd), np.linalg.norm(gbar) * np.linalg.norm(d))
    fd = _fd(lambda x: L(reads, g_=g * x), 1., 1., eps)      # the summed growth cotangent: all growths move together
    assert abs(fd - ((gbar * g).sum() if per_particle else gsum * g)) < 1e-7 * max(abs(fd), 1.)
    assert abs(gsum - gbar.sum()) < 1e-12 * np.abs(gbar).sum()


@pytest.mark.parametrize("per_particle", [False, True])
@pytest.mark.parametrize("n", [1, 37])
def test_png_weights_vjp_against_central_differences(n, per_particle):
    rng = np.random.default_rng(6)
    reads = [rng.standard_normal(n) for _ in range(4)]      # dr, s2r, ph, lp
    g = (0.4 + 0.5 * rng.uniform(size=n)) if per_particle else 0.7
    wb = rng.standard_normal(n)
    w0, pre = rng.standard_normal(n), [rng.standard_normal(n) for _ in range(3)]
    L = lambda r, g_=g, b=PNG5: float((bf.png_weights(*r, g_, b, w0)[0] * wb).sum())
    drb, s2rb, phb, lpb, gbar, b5, spdb, sigb, gsum = bf.png_weights_vjp(*reads, g, PNG5, wb, *pre)
    w, mom = bf.png_weights(*reads, g, PNG5, w0)
    d = reads[0] * g
    assert abs(mom[0] - (d ** 2).mean()) < 1e-15 and abs(mom[1] - (reads[2] * d).mean()) < 1e-15
    eps = 1e-6
    const = float((w0 * wb).sum())
    for i, bar in enumerate((drb - pre[0], s2rb - pre[1], phb, lpb)):      # (the accumulated outputs: their increments)
        dd = rng.standard_normal(n)
        fd = _fd(lambda x: L(reads[:i] + [x] + reads[i + 1:]), reads[i], dd, eps)
        assert abs(fd - (bar * dd).sum()) < 1e-7 * max(abs(fd), np.linalg.norm(bar) * np.linalg.norm(dd)), (i, fd, (bar * dd).sum())
    for i in range(5):
        fd = _fd(lambda b: L(reads, b=tuple(b)), np.array(PNG5), np.eye(5)[i], eps)
        assert abs(fd - b5[i]) < 1e-7 * max(abs(fd), 1.), (i, fd, b5[i])
    gb = gbar - pre[2]
    if per_particle:
        dd = rng.standard_normal(n)
        fd = _fd(lambda x: L(reads, g_=x), g, dd, eps)
        assert abs(fd - (gb * dd).sum()) < 1e-7 * max(abs(fd), np.linalg.norm(gb) * np.linalg.norm(dd))
    assert abs(gsum - gb.sum()) < 1e-12 * max(np.abs(gb).sum(), 1e-300) and np.isfinite(const)
    # the two mean cotangents: move the mean alone by shifting one particle's share is not possible, so they are checked through the
    # identity they enter by: drb's increment carries sigb * 2 d / n g and spdb / n ph g on top of the direct terms (covered above); here
    # their definition as sums
    bpd, bpd2, bps2 = PNG5[1], PNG5[2], PNG5[3]
    assert abs(spdb - (wb * (-bpd - 2 * bpd2 * d)).sum()) < 1e-12 * max(abs(spdb), 1.)
    assert abs(sigb - (wb * reads[2] * (-bpd2 - 2 / 3 * bps2)).sum()) < 1e-12 * max(abs(sigb), 1.)


@pytest.mark.parametrize("with_f2", [True, False])
def test_lpt_combine_vjp_against_central_differences(with_f2):
    rng = np.random.default_rng(7)
    n = 23
    F1, F2, gt = rng.standard_normal((n, 3)), (rng.standard_normal((n, 3)) if with_f2 else None), rng.standard_normal((n, 3))
    xb, vb = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    L = lambda f1, f2, g: (lambda dp, v: float((dp * xb).sum() + (v * vb).sum()))(*bf.lpt_combine(f1, f2, g))
    f2b, f1b, gtb = bf.lpt_combine_vjp(F1, F2, gt, xb, vb)
    d = rng.standard_normal((n, 3))
    eps = 1e-6
    assert abs(_fd(lambda x: L(x, F2, gt), F1, d, eps) - (f1b * d).sum()) < 1e-8 * np.linalg.norm(f1b) * np.linalg.norm(d)
    assert abs(_fd(lambda x: L(F1, F2, x), gt, d, eps) - (gtb * d).sum()) < 1e-8 * max(np.linalg.norm(gtb), 1.) * np.linalg.norm(d)
    if with_f2:
        assert abs(_fd(lambda x: L(F1, x, gt), F2, d, eps) - (f2b * d).sum()) < 1e-8 * np.linalg.norm(f2b) * np.linalg.norm(d)
    else:
        assert not gtb[:, 1:].any()


@pytest.mark.parametrize("shape,box", [((9, 15, 8), (90., 120., 100.)), ((15, 10, 12), (150., 80., 110.)), ((10, 9, 6), (70., 90., 80.)),
                                       ((12, 10, 8), (100., 120., 90.))])
def test_mesh_formulas_at_odd_shapes(shape, box):
    """The general form against the oracle's bias_fields (fftfreq wavevectors, numpy irfftn: valid as it stands for odd nx, ny) and against
    tests/_png_f64.py; an odd axis has no Nyquist entry."""
    rng = np.random.default_rng(8)
    X = np.fft.rfftn(rng.standard_normal(shape))
    fld, (a, b, c, d, e, f) = bo.bias_fields(X, box)
    f7, h6 = bf.bias_fields(X, box)
    want = [fld["delta"], fld["shear2"], fld["shear3"], fld["nab2"]] + list(fld["grad"])
    for i, (x, y) in enumerate(zip(f7, want)):
        assert np.abs(x - y).max() < 1e-12 * np.abs(y).max(), i
    assert np.abs(h6[1] - h6[0] / 3 - a).max() < 1e-12 * np.abs(a).max() and np.abs(h6[5] - f).max() < 1e-12 * np.abs(f).max()
    for ax in (0, 1):
        k = bf.kvec(shape, box)[ax].ravel()
        assert bool(np.isclose(k.min(), -np.pi * shape[ax] / box[ax])) == (shape[ax] % 2 == 0)      # the Nyquist entry, at -pi n / L
        assert bool(np.isclose(-k.min(), k.max())) == (shape[ax] % 2 == 1)
    km = bf.kabs(shape, box)
    assert np.abs(km - pf.kmesh(shape, box)).max() < 1e-14 * km.max()
    ks = np.linspace(0.3 * km.max(), 0.8 * km.max(), 17)
    table = (ks, 0.5 + ks ** 2)
    phi, lap = bf.png_phi(table, X, box)
    phi_o, lap_o = pf.png_fields(table, X, box)
    assert np.abs(phi - phi_o).max() < 1e-12 * np.abs(phi_o).max() and np.abs(lap - lap_o).max() < 1e-12 * np.abs(lap_o).max()
    out, mean = bf.add_png(table, 0.3, X, box)
    out_o, phi0 = pf.add_png(table, 0.3, X, box, return_phi=True)
    assert np.abs(out - out_o).max() < 1e-12 * np.abs(out_o).max() and abs(mean - (phi0 ** 2).mean()) < 1e-14 * mean
    pm = bf.power_mult(X, box, ks, 2. + np.sin(ks), 0.64)
    pm_o = bo.white2lin(0.8, X, shape, box, (ks, 2. + np.sin(ks)))
    assert np.abs(pm - pm_o).max() < 1e-12 * np.abs(pm_o).max()
    assert pm[0, 0, 0] == 0 and (pm == 0).sum() > 1 and (pm != 0).sum() > 1


def test_float32_runs_stay_float32():
    """dtype=np.float32 must not promote silently: the deviation it measures would shrink to nothing."""
    rng = np.random.default_rng(9)
    n = 50
    r = [x.astype(np.float32) for x in _reads(rng, n)]
    g = (0.4 + 0.5 * rng.uniform(size=n)).astype(np.float32)
    wb, vb = rng.standard_normal(n).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    for gg in (g, np.float32(0.7)):
        w, dv, _ = bf.bias_weights(*r, gg, BIAS8, dtype=np.float32)
        assert w.dtype == dv.dtype == np.float32
        outs = bf.bias_weights_vjp(*r, gg, BIAS8, wb, vb, dtype=np.float32)
        assert all(x.dtype == np.float32 for x in outs[:6]) and outs[6].dtype == np.float64
        w64 = bf.bias_weights(*r, gg, BIAS8)[0]
        assert 0 < np.abs(w - w64).max() < 1e-5 * np.abs(w64).max()
        p = bf.png_weights(r[0], r[1], r[2], r[3], gg, PNG5, w, dtype=np.float32)[0]
        assert p.dtype == np.float32
        outs = bf.png_weights_vjp(r[0], r[1], r[2], r[3], gg, PNG5, wb, r[0], r[1], r[2], dtype=np.float32)
        assert all(x.dtype == np.float32 for x in outs[:5])
    a, b = bf.lpt_combine(r[4], r[4][::-1].copy(), r[4] * 2, dtype=np.float32)
    assert a.dtype == b.dtype == np.float32
    assert all(x.dtype == np.float32 for x in bf.lpt_combine_vjp(r[4], None, r[4] * 2, vb, vb, dtype=np.float32))
