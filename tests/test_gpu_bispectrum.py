"""Binned bispectrum on the GPU (montecosmo_amd/metrics.py `bispectrum`, csrc/bispectrum.hip) against the float64 restatement
tests/_bispectrum_f64.py: the triple sums S = sum_x F_i F_j F_l and the triangle counts per triangle, judged against
A = sum_x |F_i F_j F_l| (the fields carry the rounding of one float32 C2R each, the sums themselves are float64), every shape of the
work the kernels take another path at, bitwise reproducibility, the bins against those of `spectrum`, and the bindings.

The gate.  Largest |S - S_ref| / A_ref over the parity cases of PARITY and the half-spectrum input, measured on one MI355X: 2.132e-07,
on (16, 12, 10) (the others 2.4e-08 .. 1.4e-07; the triangle counts 1.4e-08 .. 2.2e-07 of their A, the largest on (64, 64, 64), which
was added to the issue's shapes because the hand-written FFT passes start at 64, not at 32; profiles/bispectrum.txt has the list).
TOL is 4 times that, 8.528e-07: the float32 FFT error moves with shape and seed.  It is well below the 2e-5
tests/test_gpu_spectrum.py allows the power of a float32 mesh."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bispectrum_f64 as ref  # noqa: E402

MEASURED = 2.132e-7
TOL = 4 * MEASURED

BOX = {(8, 6, 4): (8., 6., 4.), (6, 6, 6): (6., 6., 6.), (16, 12, 10): (160., 132., 90.), (32, 32, 32): (320., 320., 320.),
       (20, 18, 14): (100., 90., 77.), (64, 64, 64): (640., 640., 640.)}


def _mesh(shape, seed=0):
    g = np.random.default_rng(1000 * seed + sum(shape)).standard_normal(shape).astype(np.float32)
    return (g + np.float32(0.5) * (g * g - np.float32(1))).astype(np.float32)


def _edges(shape, n_edges, past=1.):
    """n_edges from half a fundamental to `past` times the Nyquist wavenumber of the coarsest axis."""
    box = np.asarray(BOX[shape])
    return np.linspace(0.5 * 2 * np.pi / box.max(), past * np.pi * (np.asarray(shape) / box).min(), n_edges)


_REF = {}


def _reference(shape, n_edges, past=1., seed=0):
    """The float64 restatement of one case, all triangles i <= j <= l, computed once and shared."""
    key = (shape, n_edges, past, seed)
    if key not in _REF:
        _REF[key] = ref.bispectrum(_mesh(shape, seed).astype(np.float64), box_size=BOX[shape], kedges=_edges(shape, n_edges, past))
    return _REF[key]


def _raw_sums(mesh, shape, edges, tri, deconv=0):
    """(S, SN) [T]: the device's triple sums of the mesh's shell fields and of the indicator fields."""
    from montecosmo_amd import metrics
    t, real, _, shp = metrics._prepare(mesh)
    assert shp == tuple(shape)
    box = np.asarray(BOX[shape])
    ktab, ts = metrics._ktable(shape, box), np.sort(np.asarray(tri), axis=1)
    S = metrics._triple_sums(t, real, shape, ktab, metrics._deconv_table(shape, deconv), edges, ts)[0]
    SN = metrics._triple_sums(None, False, shape, ktab, None, edges, ts)[0]
    return S, SN


def _check(S, SN, r, rows=slice(None), what=""):
    eS = np.abs(S - r["S"][rows]) / np.where(r["A"][rows] > 0, r["A"][rows], 1.)
    eN = np.abs(SN - r["SN"][rows]) / np.where(r["AN"][rows] > 0, r["AN"][rows], 1.)
    print(f"bispectrum parity {what}: max |S - S_ref| / A = {eS.max():.3e}, max |SN - SN_ref| / AN = {eN.max():.3e}")
    assert np.all(np.abs(S - r["S"][rows]) <= TOL * r["A"][rows]), eS.max()
    assert np.all(np.abs(SN - r["SN"][rows]) <= TOL * r["AN"][rows]), eN.max()


PARITY = [((8, 6, 4), 5, 1.8), ((6, 6, 6), 5, 1.8), ((16, 12, 10), 6, 1.), ((32, 32, 32), 6, 1.), ((20, 18, 14), 6, 1.),
          ((64, 64, 64), 6, 1.)]


@pytest.mark.parametrize("shape,n_edges,past", PARITY)
def test_parity_vs_f64(gpu, shape, n_edges, past):
    """(8, 6, 4), (6, 6, 6): also the direct sum, edges past Nyquist; (16, 12, 10): rocFFT, non-cubic; (32, 32, 32): power of two, still
    rocFFT; (20, 18, 14): 5040 cells, a ragged last chunk; (64, 64, 64): the hand-written FFT passes, which start at 64."""
    from montecosmo_amd import metrics
    mesh, edges, r = _mesh(shape), _edges(shape, n_edges, past), _reference(shape, n_edges, past)
    tri = r["tri"]
    S, SN = _raw_sums(torch.from_numpy(mesh).to(gpu), shape, edges, tri)
    _check(S, SN, r, what=str(shape))
    # the public call is these sums, normalised
    M, V = float(np.prod(shape)), float(np.prod(BOX[shape]))
    tri_o, kmean, ntri, bk = metrics.bispectrum(torch.from_numpy(mesh).to(gpu), box_size=BOX[shape], kedges=list(edges), triangles=tri)
    np.testing.assert_array_equal(tri_o, tri)
    np.testing.assert_array_equal(ntri, SN / M)
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_array_equal(bk, (V ** 2 / M ** 3) * (S / M) / (SN / M))
    ok = np.isfinite(r["kmean"])
    np.testing.assert_allclose(kmean[ok], r["kmean"][ok], rtol=1e-10)
    if np.prod(shape) < 300:
        s_dir, n_dir = ref.direct(mesh.astype(np.float64), box_size=BOX[shape], kedges=edges)
        assert n_dir.sum() > 0
        np.testing.assert_array_equal(np.rint(ntri).astype(np.int64), n_dir)
        assert np.all(np.abs(S / M - s_dir) * M <= TOL * r["A"])


def test_parity_half_spectrum_input(gpu):
    shape, n_edges = (16, 12, 10), 6
    mesh, edges, r = _mesh(shape), _edges(shape, n_edges), _reference(shape, n_edges)
    spec = np.fft.rfftn(mesh.astype(np.float64)).astype(np.complex64)
    S, SN = _raw_sums(torch.from_numpy(spec).to(gpu), shape, edges, r["tri"])
    _check(S, SN, r, what="complex64 input")


def test_one_bin_one_triangle(gpu):
    shape = (16, 12, 10)
    mesh, edges = _mesh(shape), _edges(shape, 6)[[1, 4]]
    r = ref.bispectrum(mesh.astype(np.float64), box_size=BOX[shape], kedges=edges)
    assert len(r["tri"]) == 1
    S, SN = _raw_sums(mesh, shape, edges, [[0, 0, 0]])
    _check(S, SN, r, what="1 bin, T = 1")


def test_32_bins(gpu):
    shape = (32, 32, 32)
    from montecosmo_amd import metrics
    mesh, edges = _mesh(shape), _edges(shape, 33, 1.2)
    tri = metrics._bispec_triangles(edges)[::7]
    assert tri.max() == 31 and len(tri) > 256
    r = ref.bispectrum(mesh.astype(np.float64), box_size=BOX[shape], kedges=edges, triangles=tri)
    S, SN = _raw_sums(mesh, shape, edges, tri)
    _check(S, SN, r, what=f"32 bins, T = {len(tri)}")


def test_65_triangles_with_repeats_and_orders(gpu):
    """T = 65: one more than a wave, lanes split into two groups of 128; rows repeat and come in any index order."""
    shape, n_edges = (16, 12, 10), 6
    mesh, edges, r = _mesh(shape), _edges(shape, n_edges), _reference(shape, n_edges)
    rng = np.random.default_rng(65)
    rows = rng.integers(0, len(r["tri"]), 65)
    tri = np.stack([rng.permutation(row) for row in r["tri"][rows]])
    S, SN = _raw_sums(mesh, shape, edges, tri)
    _check(S, SN, r, rows=rows, what="T = 65")


def test_364_triangles(gpu):
    """All triangles of 12 bins: more triangles than lanes, two per lane and a ragged second round."""
    shape = (16, 12, 10)
    mesh, edges = _mesh(shape), _edges(shape, 13, 1.5)
    r = ref.bispectrum(mesh.astype(np.float64), box_size=BOX[shape], kedges=edges)
    assert len(r["tri"]) == 364
    S, SN = _raw_sums(mesh, shape, edges, r["tri"])
    _check(S, SN, r, what="T = 364")


def test_8192_triangles_on_64(gpu):
    """MAX_TRIANGLES rows on 2^18 cells: eight tiles of the list, four lanes' worth of triangles per lane, and workgroups that walk four
    chunks each.  The rows repeat the 35 triangles of the parity case, in any index order."""
    from montecosmo_amd import metrics
    shape, n_edges = (64, 64, 64), 6
    mesh, edges, r = _mesh(shape), _edges(shape, n_edges), _reference(shape, n_edges)
    rng = np.random.default_rng(8192)
    rows = rng.integers(0, len(r["tri"]), metrics.MAX_TRIANGLES)
    tri = rng.permuted(r["tri"][rows], axis=1)
    S, SN = _raw_sums(torch.from_numpy(mesh).to(gpu), shape, edges, tri)
    _check(S, SN, r, rows=rows, what="T = 8192 on 64^3")


def test_row_order_and_index_order_do_not_change_a_bit(gpu):
    from montecosmo_amd import metrics
    shape, n_edges = (16, 12, 10), 6
    mesh, edges, tri = torch.from_numpy(_mesh(shape)).to(gpu), list(_edges(shape, n_edges)), _reference(shape, n_edges)["tri"]
    kw = dict(box_size=BOX[shape], kedges=edges)
    base = metrics.bispectrum(mesh, triangles=tri, **kw)
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(tri))
    shuffled = np.stack([rng.permutation(row) for row in tri[perm]])
    got = metrics.bispectrum(mesh, triangles=shuffled, **kw)
    np.testing.assert_array_equal(got[0], shuffled)
    assert np.array_equal(got[2], base[2][perm]) and np.array_equal(got[3], base[3][perm], equal_nan=True)


def test_bin_above_every_mode(gpu):
    from montecosmo_amd import metrics
    shape = (16, 12, 10)
    edges = list(_edges(shape, 4)) + [50., 60.]      # bin 3 takes every mode above Nyquist, bin 4 lies above the corner of the spectrum
    tri, kmean, ntri, bk = metrics.bispectrum(_mesh(shape), box_size=BOX[shape], kedges=edges, triangles=[[0, 1, 4], [4, 4, 4], [0, 1, 1]])
    assert ntri[0] == 0 and ntri[1] == 0 and ntri[2] > 0.5
    assert np.isnan(bk[0]) and np.isnan(bk[1]) and np.isfinite(bk[2]) and np.isnan(kmean[4])


def test_bitwise_repeat_batch_and_unaligned(gpu):
    from montecosmo_amd import metrics
    shape, n_edges = (16, 12, 10), 6
    kw = dict(box_size=BOX[shape], kedges=list(_edges(shape, n_edges)), reduced=True)
    rows = torch.from_numpy(np.stack([_mesh(shape, seed) for seed in range(3)])).to(gpu)
    first = metrics.bispectrum(rows[0], **kw)
    again = metrics.bispectrum(rows[0], **kw)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, again))
    batched = metrics.bispectrum(rows, **kw)
    assert batched[3].shape == (3, len(first[0])) and batched[4].shape == batched[3].shape
    for i in range(3):
        single = metrics.bispectrum(rows[i], **kw)
        assert np.array_equal(batched[2], single[2])
        assert np.array_equal(batched[3][i], single[3], equal_nan=True) and np.array_equal(batched[4][i], single[4], equal_nan=True)
    # a view one float into a larger buffer
    buf = torch.zeros(rows[0].numel() + 1, dtype=torch.float32, device=gpu)
    buf[1:] = rows[0].reshape(-1)
    view = buf[1:].reshape(shape)
    assert view.data_ptr() % 8 == 4
    off = metrics.bispectrum(view, **kw)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, off))


def test_bins_are_the_bins_of_spectrum(gpu):
    """The shell split puts every mode where `spectrum` bins it.  Before the transform, exactly: the Hermitian-weighted count of the
    unit spectrum's shells is kcount, and their power the bin sums of |d|^2 to float64 rounding.  After it: sum_x F_b^2 / M is the same
    bin sum (Parseval) to the float32 gate of tests/test_gpu_spectrum.py, and I_b(0) is kcount.  I_b(0) is exact where every pass of the
    C2R leaves its zeroth output as a plain sum of integers, which the hand-written passes of (64, 64, 64) do; rocFFT's real inverse of
    an even length recombines the line with rounded twiddles, and (16, 12, 10) came out one float32 ulp off in one bin of eight
    (204.000015 for 204), so that shape holds I_b(0) to the float32 gate and to the integer it rounds to."""
    from montecosmo_amd import metrics
    for shape in ((16, 12, 10), (64, 64, 64)):
        box, edges = np.asarray(BOX[shape]), _edges(shape, 9, 1.6)
        mesh = torch.from_numpy(_mesh(shape)).to(gpu)
        t, real, _, _ = metrics._prepare(mesh)
        ktab = metrics._ktable(shape, box)
        sums = metrics._bin_sums(mesh, None, box, (0., 0., 0.), 0, list(edges), True, 0)[2][0]
        kcount, p2 = sums[0], sums[2]
        assert np.count_nonzero(kcount) >= 6
        w = torch.full((shape[2] // 2 + 1,), 2., dtype=torch.float64, device=gpu)
        w[0] = w[-1] = 1.
        unit = metrics._shell_spectra(None, False, shape, gpu, ktab, None, edges)[0]
        assert torch.all(unit.imag == 0) and torch.all((unit.real == 0) | (unit.real == 1))
        np.testing.assert_array_equal((unit.real.to(torch.float64) * w).sum(dim=(1, 2, 3)).cpu().numpy(), kcount)
        sh = metrics._shell_spectra(t, real, shape, gpu, ktab, None, edges)[0].to(torch.complex128)
        np.testing.assert_allclose(((sh.real ** 2 + sh.imag ** 2) * w).sum(dim=(1, 2, 3)).cpu().numpy(), p2, rtol=1e-12)
        F = metrics._shell_fields(t, real, shape, gpu, ktab, None, edges)[0].to(torch.float64)
        I0 = metrics._shell_fields(None, False, shape, gpu, ktab, None, edges)[0][:, 0, 0, 0].cpu().numpy().astype(np.float64)
        p = (F * F).sum(dim=(1, 2, 3)).cpu().numpy() / float(np.prod(shape))
        assert np.all(np.abs(p - p2) <= 2e-5 * p2), (p, p2)
        print(f"bispectrum I_b(0) - kcount on {shape}: {I0 - kcount}")
        if shape == (64, 64, 64):
            np.testing.assert_array_equal(I0, kcount)
        else:
            np.testing.assert_array_equal(np.rint(I0), kcount)
            assert np.all(np.abs(I0 - kcount) <= 2e-5 * kcount)


def test_reduced_and_deconv(gpu):
    from montecosmo_amd import metrics
    shape, n_edges = (16, 12, 10), 6
    mesh, edges = _mesh(shape), _edges(shape, n_edges)
    r = ref.bispectrum(mesh.astype(np.float64), box_size=BOX[shape], kedges=edges, deconv=2)
    tri, kmean, ntri, bk, qk = metrics.bispectrum(mesh, box_size=BOX[shape], kedges=list(edges), triangles=r["tri"], deconv=2, reduced=True)
    M, V = float(np.prod(shape)), float(np.prod(BOX[shape]))
    # bk = c S / ntri: the errors of S (TOL A) and of ntri (TOL AN / M), to first order
    with np.errstate(divide="ignore", invalid="ignore"):
        c = V ** 2 / M ** 4
        bound = TOL * (c * r["A"] / r["ntri"] + np.abs(r["bk"]) * (r["AN"] / M) / r["ntri"]) * 1.01
        pi, pj, pl = (r["pk"][r["tri"][:, a]] for a in range(3))
        den = pi * pj + pj * pl + pl * pi
    ok = r["ntri"] > 0.5
    assert ok.sum() > 20
    assert np.all(np.abs(bk - r["bk"])[ok] <= bound[ok])
    # qk = bk / den, den = P_i P_j + ... of positive float32-gated powers (2e-5 each, so 4e-5 on a product)
    assert np.all(np.abs(qk - r["qk"])[ok] <= (bound / den + 4.1e-5 * np.abs(r["qk"]))[ok])


def test_bispectrum_chains(gpu):
    from montecosmo_amd import chains, model
    shape = (16, 12, 10)
    fwd = model.FieldLevelForward(final_shape=shape, cell_length=10.)
    meshes = np.stack([_mesh(shape, seed) for seed in range(6)]).reshape((2, 3) + shape)
    ch = chains.Chains({"m": torch.from_numpy(meshes).to(gpu), "n_evals": np.ones((2, 3))})
    out = fwd.bispectrum_chains(ch, names="m", kedges=5)
    assert "kb_m" not in ch and set(out) == {"m", "n_evals", "kb_m"} and len(out["kb_m"]) == 4
    tri, kmean, ntri, bk = out["kb_m"]
    T = len(tri)
    assert T > 4 and tri.shape == (T, 3) and kmean.shape == (4,) and ntri.shape == (T,) and bk.shape == (2, 3, T)
    for c in range(2):
        for i in range(3):
            single = fwd.bispectrum(torch.from_numpy(meshes[c, i]).to(gpu), kedges=5)
            assert np.array_equal(single[0], tri) and np.array_equal(single[2], ntri)
            assert np.array_equal(bk[c, i], single[3], equal_nan=True)
    assert len(fwd.bispectrum_chains(ch, names="m", kedges=5, reduced=True)["kb_m"]) == 5


def test_argument_errors(gpu):
    from montecosmo_amd import metrics, _lib
    mesh = np.zeros((16, 12, 10), np.float32)
    with pytest.raises(ValueError):
        metrics.bispectrum(np.zeros((16, 12, 9), np.float32), kedges=[0.1, 0.5, 1.])
    with pytest.raises((ValueError, _lib.McpmError)):
        metrics.bispectrum(mesh, kedges=list(np.linspace(0.1, 3., 34)))
    with pytest.raises((ValueError, _lib.McpmError)):
        metrics.bispectrum(mesh, kedges=[0.1, 0.5, 1.], triangles=np.zeros((0, 3), dtype=np.int64))
    with pytest.raises((ValueError, _lib.McpmError)):
        metrics.bispectrum(mesh, kedges=[0.1, 0.5, 1.], triangles=[[0, 1, 2]])
    with pytest.raises((ValueError, _lib.McpmError)):
        metrics.bispectrum(mesh, kedges=[0.1, 1., 0.5])
    with pytest.raises((ValueError, _lib.McpmError)):
        metrics.bispectrum(mesh)      # the default spacing leaves one edge on this small mesh: no bin
