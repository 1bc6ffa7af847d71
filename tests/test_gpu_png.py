"""Local primordial non-Gaussianity on the GPU (bricks.add_png / add_png_vjp, mcpm_png_add_f32 / mcpm_png_add_vjp_f32) against
the float64 restatement tests/_png_f64.py, an analytic plane-wave answer that does not use the restatement, and central
differences of the restatement for the adjoint.  Gates: the project's 2e-5 relative L2 forward (tests/test_gpu_bias.py); the
finite-difference step and tolerance of tests/test_gpu_model.py (eps 1e-5, 3e-3 of the difference quotient)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _png_f64 as pf  # noqa: E402
from oracle import pm_oracle as o  # noqa: E402  (checker only)

SHAPES = [((16, 16, 16), (160., 160., 160.)), ((16, 12, 8), (200., 120., 100.)), ((32, 32, 32), (640., 640., 640.))]
sid = lambda v: "x".join(str(int(s)) for s in v[0]) if isinstance(v, tuple) and isinstance(v[0], tuple) else None


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    dt = np.complex128 if (np.iscomplexobj(a) or np.iscomplexobj(b)) else np.float64
    return float(np.linalg.norm(a.astype(dt) - b.astype(dt)) / np.linalg.norm(b.astype(dt)))


def lin_field(rng, shape):
    """A real field's half-spectrum without its k = 0 mode (a linear density field has none: P(0) = 0)."""
    X = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    X[0, 0, 0] = 0.
    return X.astype(np.complex64)


def pair(a, b):
    """Real-pair inner product of two half-spectra: the pairing every `_vjp` here uses for complex cotangents."""
    return float((a.real * b.real + a.imag * b.imag).sum())


@pytest.mark.parametrize("case", SHAPES, ids=sid)
def test_add_png_forward(gpu, case):
    """(i) forward against the restatement for fNL in {0, 100, -500}; fNL = 0 returns the input to float32 round-off."""
    from montecosmo_amd import bricks
    shape, box = case
    cosmo = bricks.Planck18()
    table = bricks.trans_phi2delta_table(cosmo)
    X = lin_field(np.random.default_rng(11), shape)
    errs, outs = [], {}
    for fNL in (0., 100., -500.):
        out = bricks.add_png(cosmo, fNL, X, box)
        again = bricks.add_png(cosmo, fNL, X, box)
        assert out.shape == X.shape and str(out.dtype) == "torch.complex64"
        assert bool((out == again).all()), "repeat calls must be bitwise equal"
        outs[fNL] = got = out.cpu().numpy()
        want = pf.add_png(table, fNL, X, box)
        e = rel_l2(got, want)
        print(f"add_png[{sid(case)} fNL={fNL}] rel L2 {e:.3e}")
        if e >= 2e-5:
            errs.append((fNL, e))
        assert got[0, 0, 0] == 0.
    e0 = rel_l2(outs[0.], X)
    print(f"add_png[{sid(case)} fNL=0] vs input rel L2 {e0:.3e}")
    assert e0 < 2e-5
    # the non-Gaussian increment is 2e-3 .. 1.5e-2 of the field here: a 2e-5 error of the whole is up to 1e-2 of it, which must
    # still tell fNL = 100 from fNL = -500 (increments in the ratio -5)
    inc = lambda f: outs[f] - outs[0.]
    assert rel_l2(inc(-500.), -5. * inc(100.)) < 2e-2
    assert not errs, errs


def test_add_png_phi_argument(gpu):
    """`phi=`: handing over the Gaussian potential gives the same output (bitwise: the same kernels run on the same values)."""
    from montecosmo_amd import bricks
    shape, box = SHAPES[1]
    cosmo = bricks.Planck18()
    X = lin_field(np.random.default_rng(12), shape)
    out, ctx = bricks.add_png(cosmo, 80., X, box, return_ctx=True)
    phi_o = pf.add_png(bricks.trans_phi2delta_table(cosmo), 80., X, box, return_phi=True)[1]
    assert rel_l2(ctx.phi.cpu().numpy(), phi_o) < 2e-5
    out2 = bricks.add_png(cosmo, 80., X, box, phi=ctx.phi.clone())
    assert bool((out == out2).all())


def test_add_png_plane_wave(gpu):
    """(ii) phi = A cos(k0 x): the output has power at +-k0 (the input, unchanged) and at +-2 k0 with cosine amplitude
    fNL A^2 / 2 * t(2 k0), nothing at k = 0 -- worked out by hand, independent of the restatement."""
    from montecosmo_amd import bricks
    n, L, j, A, fNL = 16, 400., 2, 1e-4, 100.
    shape, box = (n, n, n), (L, L, L)
    cosmo = bricks.Planck18()
    ks, trans = bricks.trans_phi2delta_table(cosmo)
    k0 = 2 * np.pi * j / L
    t1, t2 = np.interp(k0, ks, trans), np.interp(2 * k0, ks, trans)
    M = n ** 3
    X = np.zeros((n, n, n // 2 + 1), dtype=np.complex128)
    X[j, 0, 0] = X[n - j, 0, 0] = 0.5 * A * M * t1                        # A cos(k0 x) -> A/2 M at +-k0, times t(k0)
    want = X.copy()
    want[2 * j, 0, 0] = want[n - 2 * j, 0, 0] = 0.5 * (fNL * A * A / 2) * M * t2
    got = bricks.add_png(cosmo, fNL, X.astype(np.complex64), box).cpu().numpy().astype(np.complex128)
    scale = abs(want[j, 0, 0])
    assert abs(want[2 * j, 0, 0]) > 1e-3 * scale                         # the second harmonic is well above round-off
    assert got[0, 0, 0] == 0.
    # float32 round-off scales with the largest coefficient: every coefficient to the forward gate of that scale
    print("plane wave: k0", abs(got[j, 0, 0] - want[j, 0, 0]) / scale, "2k0", abs(got[2 * j, 0, 0] - want[2 * j, 0, 0]) / scale,
          "largest other", np.abs(got - want).max() / scale)
    assert np.abs(got - want).max() < 2e-5 * scale
    assert rel_l2(got, want) < 2e-5


@pytest.mark.parametrize("case", SHAPES[:2], ids=sid)
def test_add_png_vjp(gpu, case):
    """(iii) lin_mesh, fNL and table cotangents against central differences of the restatement; two calls bitwise equal."""
    from montecosmo_amd import bricks
    shape, box = case
    rng = np.random.default_rng(21)
    cosmo = bricks.Planck18()
    ks, trans = bricks.trans_phi2delta_table(cosmo)
    X = lin_field(rng, shape)
    X64 = X.astype(np.complex128)
    fNL = -300.
    ob = (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)).astype(np.complex64)   # a generic (non-Hermitian) cotangent
    out, ctx = bricks.add_png(cosmo, fNL, X, box, return_ctx=True)
    lb, fb, tb = bricks.add_png_vjp(ctx, ob)
    lb2, fb2, tb2 = bricks.add_png_vjp(ctx, ob)
    assert bool((lb == lb2).all()) and fb == fb2 and np.array_equal(tb, tb2), "repeat calls must be bitwise equal"
    assert tb.shape == (256,) and tb.dtype == np.float64 and np.isfinite(tb).all()
    lb = lb.cpu().numpy().astype(np.complex128)
    ob64 = ob.astype(np.complex128)
    L = lambda lin, f, tr: pair(ob64, pf.add_png((ks, tr), f, lin, box))
    eps = 1e-5
    # lin_mesh: a real field's half-spectrum as direction (the Hermitian redundancy of the kz = 0 / Nyquist planes is part of the
    # real-pair convention: the cotangent pairs with variations of the half-spectrum that numpy's irfftn sees)
    d = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    fd = (L(X64 + eps * d, fNL, trans) - L(X64 - eps * d, fNL, trans)) / (2 * eps)
    an = pair(lb, d)
    print(f"add_png_vjp[{sid(case)}] lin_mesh fd {fd:.6e} an {an:.6e}")
    assert abs(fd - an) < 3e-3 * abs(fd), ("lin_mesh", fd, an)
    # a single interior mode (kz not in {0, nz/2}) with an arbitrary complex value: a direction no real field's spectrum gives
    d1 = np.zeros_like(X64)
    d1[2, 3, 1] = (0.7 - 1.3j) * np.abs(X64).mean()
    fd1 = (L(X64 + eps * d1, fNL, trans) - L(X64 - eps * d1, fNL, trans)) / (2 * eps)
    an1 = pair(lb, d1)
    print(f"add_png_vjp[{sid(case)}] lin_mesh single mode fd {fd1:.6e} an {an1:.6e}")
    assert abs(fd1 - an1) < 3e-3 * abs(fd1), ("lin_mesh single mode", fd1, an1)
    # fNL
    h = eps * abs(fNL)
    fdf = (L(X64, fNL + h, trans) - L(X64, fNL - h, trans)) / (2 * h)
    print(f"add_png_vjp[{sid(case)}] fNL fd {fdf:.6e} an {fb:.6e}")
    assert abs(fdf - fb) < 3e-3 * abs(fdf), ("fNL", fdf, fb)
    # the table: a smooth relative tilt and a node-by-node random relative direction
    lk = np.log(ks / ks[0]) / np.log(ks[-1] / ks[0])
    for name, dirn in (("tilt", trans * (0.5 + lk)), ("random", trans * rng.standard_normal(256))):
        fdt = (L(X64, fNL, trans + eps * dirn) - L(X64, fNL, trans - eps * dirn)) / (2 * eps)
        ant = float((tb * dirn).sum())
        print(f"add_png_vjp[{sid(case)}] table {name} fd {fdt:.6e} an {ant:.6e}")
        assert abs(fdt - ant) < 3e-3 * abs(fdt), ("table " + name, fdt, ant)
    # nodes no mode of this mesh brackets receive nothing
    km = pf.kmesh(shape, box)
    used = np.zeros(256, bool)
    lo = np.searchsorted(ks, km[km > 0], side="right") - 1
    used[lo] = used[lo + 1] = True
    assert np.all(tb[~used] == 0.) and np.any(tb[used] != 0.)
