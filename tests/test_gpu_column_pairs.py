"""Column FFT passes with two kz columns per thread (fftpm.hip, ColShape NL = 2): the Poisson solve and its adjoint against
the float64 oracle, the half-valid last pair (nzh = nz/2 + 1 is odd: Nyquist column + one pad column), the windowed and
chunked slab passes, and bitwise repeatability.  Every axis length from 64 to 256 takes each role (z, y, x)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pm_oracle as o  # noqa: E402  (checker only)

# nzh = 33, 129, 65: every axis length from 64 to 256 in every role; the last three put 256 and 512 on the y axis and 512 on the
# x axis, the lengths at which the y passes with factors and the forward x pass run two columns per thread
MESHES = [(64, 64, 64), (64, 128, 256), (256, 64, 128), (64, 256, 64), (64, 512, 64), (512, 64, 64)]
TOL = 2e-6                                                # the bound of tests/test_gpu_fftpm.py


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(white rho, red rho, f_bar) float32 and their float64 oracle results, computed once per mesh."""
    rng = np.random.default_rng(sum(shape))
    white = rng.standard_normal(shape).astype(np.float32)
    kvec = o.rfftk(shape)
    kk = sum(np.asarray(k, np.float64) ** 2 for k in kvec)
    kk[0, 0, 0] = 1.0
    red = np.fft.irfftn(np.fft.rfftn(rng.standard_normal(shape)) * kk ** -0.75, s=shape, axes=(0, 1, 2))
    red = (red / red.std()).astype(np.float32)
    fbar = rng.standard_normal((3,) + shape).astype(np.float32)
    mult = [-o.gradient_hat(kvec, c) * o.invlaplace_hat(kvec) for c in range(3)]
    want = {}
    for name, rho in (("white", white), ("red", red)):
        X = np.fft.rfftn(rho.astype(np.float64))
        want[name] = np.stack([np.fft.irfftn(m * X, s=shape, axes=(0, 1, 2)) for m in mult])
    acc = sum(np.conj(mult[c]) * np.fft.rfftn(fbar[c].astype(np.float64)) for c in range(3))
    want["vjp"] = np.fft.irfftn(acc, s=shape, axes=(0, 1, 2))
    return {"white": white, "red": red, "fbar": fbar, "want": want}


@pytest.fixture(scope="module")
def nb(gpu):
    from montecosmo_amd import nbody
    return nbody


def _p(t):
    return C.c_void_p(t.data_ptr())


def _force(nb, rho):
    import torch
    plan = nb.get_plan(rho.shape)
    r = torch.from_numpy(rho).cuda()
    fm = torch.empty((3,) + rho.shape, dtype=torch.float32, device="cuda")
    plan.call("mcpm_force_meshes_f32", _p(r), _p(fm))
    return fm.cpu().numpy()


def _vjp(nb, fbar):
    import torch
    shape = fbar.shape[1:]
    plan = nb.get_plan(shape)
    f = torch.from_numpy(fbar).cuda()
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    plan.call("mcpm_force_meshes_vjp_f32", _p(f), _p(out))
    return out.cpu().numpy()


class _Passes:
    """The solve issued pass by pass (the slab entry points on a one-rank plan) on spectra this test owns, so that it can
    reach the pad columns nzh..nzp-1 of every spectrum."""

    def __init__(self, nb, shape, chunks=1):
        import torch
        self.torch, self.shape = torch, shape
        self.plan = nb.Plan(shape)
        self.plan.call("mcpm_slab_set_chunks", chunks)
        self.ss = self.plan.call("mcpm_slab_spec_elems")
        nx, ny, nz = shape
        self.nzh, self.nzp = nz // 2 + 1, nz // 2 + 16
        assert self.ss == nx * ny * self.nzp
        self.M = nx * ny * nz

    def spec(self, n, fill):
        return self.torch.full((n, self.shape[0], self.shape[1], self.nzp, 2), fill, dtype=self.torch.float32, device="cuda")

    def window(self, x0=0, count=None):
        self.plan.call("mcpm_slab_set_window", x0, self.shape[0] if count is None else count)

    def forward(self, rho, fill, interleaved=False, packed=0):
        """rho -> three force meshes; every spectrum starts filled with `fill` (pads included)."""
        t = self.torch
        r = t.from_numpy(rho).cuda()
        s1, s2, s3 = self.spec(1, fill), self.spec(2, fill), self.spec(3, fill)
        call = self.plan.call
        call("mcpm_slab_zfwd", _p(r), self.M, _p(s1), 1)
        call("mcpm_slab_ycol", _p(s1), _p(s1), 1, -1, 0, 0)
        call("mcpm_slab_xfused", _p(s1), _p(s2), 0)
        call("mcpm_slab_ycol2", _p(s2), _p(s3), 1, packed, 0, 3)
        if interleaved:
            out = t.empty(self.shape + (3,), dtype=t.float32, device="cuda")
            call("mcpm_slab_zinv3_il", _p(s3), _p(out))
            return np.moveaxis(out.cpu().numpy(), -1, 0)
        out = t.empty((3,) + self.shape, dtype=t.float32, device="cuda")
        call("mcpm_slab_zinv", _p(s3), _p(out), self.M, 3)
        return out.cpu().numpy()

    def adjoint(self, fbar, fill):
        t = self.torch
        f = t.from_numpy(fbar).cuda()
        s3, s2, s1 = self.spec(3, fill), self.spec(2, fill), self.spec(1, fill)
        call = self.plan.call
        call("mcpm_slab_zfwd", _p(f), self.M, _p(s3), 3)
        call("mcpm_slab_ycol2", _p(s3), _p(s2), 0, 0, 0, 3)
        call("mcpm_slab_xfused", _p(s2), _p(s1), 1)
        call("mcpm_slab_ycol", _p(s1), _p(s1), 1, +1, 0, 0)
        out = t.empty(self.shape, dtype=t.float32, device="cuda")
        call("mcpm_slab_zinv", _p(s1), _p(out), self.M, 1)
        return out.cpu().numpy()


@pytest.mark.parametrize("shape", MESHES)
@pytest.mark.parametrize("colour", ["white", "red"])
def test_forward_matches_oracle(nb, shape, colour):
    d = _inputs(shape)
    planar = _force(nb, d[colour])
    inter = _Passes(nb, shape).forward(d[colour], 0.0, interleaved=True)
    for c in range(3):
        ep, ei = rel_l2(planar[c], d["want"][colour][c]), rel_l2(inter[c], d["want"][colour][c])
        print(shape, colour, c, "planar %.3g interleaved %.3g" % (ep, ei))
        assert ep < TOL and ei < TOL, c


@pytest.mark.parametrize("shape", MESHES)
def test_adjoint_matches_oracle(nb, shape):
    d = _inputs(shape)
    e = rel_l2(_vjp(nb, d["fbar"]), d["want"]["vjp"])
    print(shape, "%.3g" % e)
    assert e < TOL


@pytest.mark.parametrize("shape", MESHES)
def test_adjointness(nb, shape):
    """<F_bar, J rho> = <J^T F_bar, rho>, accumulated in float64; the bound is the one of tests/test_gpu_fftpm.py."""
    d = _inputs(shape)
    fm, rb = _force(nb, d["white"]), _vjp(nb, d["fbar"])
    lhs = np.sum(fm.astype(np.float64) * d["fbar"])
    rhs = np.sum(d["white"].astype(np.float64) * rb)
    scale = np.sqrt(np.sum(fm.astype(np.float64) ** 2) * np.sum(d["fbar"].astype(np.float64) ** 2))
    print(shape, "%.3g" % (abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) < 1e-5 * scale


@pytest.mark.parametrize("shape", MESHES)
def test_pad_columns_are_never_read(nb, shape):
    """NaN in the pad columns nzh..nzp-1 of every spectrum (the last pair of a row holds the Nyquist column and the first of
    them) changes nothing, forward or adjoint, and equals the solve on the plan's own scratch bit for bit."""
    d = _inputs(shape)
    ps = _Passes(nb, shape)
    clean, dirty = ps.forward(d["white"], 0.0), ps.forward(d["white"], float("nan"))
    assert np.isfinite(dirty).all() and np.array_equal(clean, dirty)
    assert np.array_equal(clean, _force(nb, d["white"]))
    clean, dirty = ps.adjoint(d["fbar"], 0.0), ps.adjoint(d["fbar"], float("nan"))
    assert np.isfinite(dirty).all() and np.array_equal(clean, dirty)
    assert np.array_equal(clean, _vjp(nb, d["fbar"]))


@pytest.mark.parametrize("shape", [(64, 64, 64), (256, 256, 64)])   # one column per thread / two
def test_windowed_and_chunked_passes_are_bitwise_the_whole_pass(nb, shape):
    """mcpm_slab_ycol / ycol2 over two windows of planes, and all three column passes with two chunks (transposed-order
    layouts in and out), give the bits of the unwindowed, unchunked pass, in the one-column forms (64^3) and the pair forms.  (On one rank a chunked layout orders the planes
    as the plain one does; the x pass has no window: it runs whole rows.)"""
    import torch
    nx, ny, nz = shape
    rng = np.random.default_rng(7)
    src = torch.from_numpy(rng.standard_normal((3, nx, ny, nz // 2 + 16, 2)).astype(np.float32)).cuda()
    results = []
    a, h = 3 * nx // 8, nx // 2
    for chunks, windows in ((1, [(0, nx)]), (1, [(0, a), (a, nx - a)]), (2, [(0, h), (h, h)])):
        ps = _Passes(nb, shape, chunks)
        y1, y2e, y2c, xa, xb = ps.spec(1, 0.0), ps.spec(3, 0.0), ps.spec(2, 0.0), ps.spec(2, 0.0), ps.spec(1, 0.0)
        packed = int(chunks > 1)
        for x0, n in windows:
            ps.window(x0, n)
            ps.plan.call("mcpm_slab_ycol", _p(src), _p(y1), 1, -1, 0, packed)
            ps.plan.call("mcpm_slab_ycol2", _p(src), _p(y2e), 1, packed, 0, 3)
            ps.plan.call("mcpm_slab_ycol2", _p(src), _p(y2c), 0, 0, packed, 3)
        ps.plan.call("mcpm_slab_xfused", _p(src), _p(xa), 0)     # window still set: the x pass ignores it
        ps.plan.call("mcpm_slab_xfused", _p(src), _p(xb), 1)
        ps.window()
        results.append([t.cpu().numpy()[..., :ps.nzh, :] for t in (y1, y2e, y2c, xa, xb)])
    for other in results[1:]:
        for name, a, b in zip(("ycol", "ycol2 expand", "ycol2 contract", "xfused 0", "xfused 1"), results[0], other):
            assert np.isfinite(a).all() and np.abs(a).max() > 0, name
            assert np.array_equal(a, b), name


@pytest.mark.parametrize("shape", MESHES)
def test_bitwise_repeat(nb, shape):
    d = _inputs(shape)
    assert np.array_equal(_force(nb, d["white"]), _force(nb, d["white"]))
    assert np.array_equal(_vjp(nb, d["fbar"]), _vjp(nb, d["fbar"]))
