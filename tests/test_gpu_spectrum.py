"""Binned spectra on the GPU (montecosmo_amd/metrics.py, csrc/spectrum.hip) against the float64 restatement
tests/_spectrum_f64.py: mode counts exactly (bin assignment is digitize restated bit for bit), bin means and powers to the
float64 rounding of the sums (judged against the bin sum of |weights|, which is |pow| for an auto monopole), bitwise
reproducibility and batch equality, and the FieldLevelForward bindings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _spectrum_f64 as ref  # noqa: E402


def _white_spec(shape, seed):
    rng = np.random.default_rng(seed)
    h = (shape[0], shape[1], shape[2] // 2 + 1)
    return (rng.standard_normal(h) + 1j * rng.standard_normal(h)).astype(np.complex64)


def _check(got, want, rtol=1e-10, min_count=0):
    kc, km, pw = got
    kc_r, km_r, pw_r, pa_r = want
    np.testing.assert_array_equal(kc, kc_r)
    ok = kc_r > min_count
    np.testing.assert_array_equal(np.isnan(km), np.isnan(km_r))
    np.testing.assert_allclose(km[ok], km_r[ok], rtol=rtol, atol=0)
    if not isinstance(pw, dict):
        pw, pw_r, pa_r = {0: pw}, {0: pw_r}, {0: pa_r}
    assert sorted(pw) == sorted(pw_r)
    for ell in pw:
        np.testing.assert_array_equal(np.isnan(pw[ell]), np.isnan(pw_r[ell]))
        err = np.abs(pw[ell] - pw_r[ell])[ok]
        assert np.all(err <= rtol * pa_r[ell][ok]), (ell, np.max(err / np.where(pa_r[ell][ok] > 0, pa_r[ell][ok], 1)))


CASES = [((64, 64, 64), (640., 640., 640.)), ((48, 64, 40), (480., 640., 400.))]


@pytest.mark.parametrize("shape,box", CASES)
@pytest.mark.parametrize("center", [(0., 0., 0.), (300., -800., 2000.)])
@pytest.mark.parametrize("cross", [False, True])
def test_spectrum_input_vs_f64(gpu, shape, box, center, cross):
    from montecosmo_amd import metrics
    s0 = _white_spec(shape, 1)
    s1 = _white_spec(shape, 2) if cross else None
    kw = dict(box_size=box, box_center=center, ells=[0, 2, 4])
    got = metrics._spectrum(torch.from_numpy(s0).to(gpu), None if s1 is None else torch.from_numpy(s1).to(gpu), **kw)
    want = ref.spectrum(s0.astype(np.complex128), None if s1 is None else s1.astype(np.complex128), mesh_shape=shape, **kw)
    _check(got, want)
    # edges on mode values: many modes sit exactly on an edge
    los = np.asarray(center) / (np.linalg.norm(center) or 1.)
    kmesh = ref.waves(np.array(shape), box, None, True, los)[1]
    edges = list(np.unique(kmesh)[::7])
    got = metrics._spectrum(s0, s1, kedges=edges, **{**kw, "ells": 0})
    want = ref.spectrum(s0.astype(np.complex128), None if s1 is None else s1.astype(np.complex128), mesh_shape=shape,
                        kedges=edges, **{**kw, "ells": 0})
    _check(got, want)


@pytest.mark.parametrize("n", [64, 128])
def test_real_mesh_input_vs_f64(gpu, n):
    from montecosmo_amd import metrics
    rng = np.random.default_rng(n)
    m = rng.standard_normal((n, n, n)).astype(np.float32)
    box = (n * 10., n * 10., n * 10.)
    got = metrics._spectrum(torch.from_numpy(m).to(gpu), box_size=box)
    want = ref.spectrum(m.astype(np.float64), box_size=box)
    _check(got, want, rtol=2e-5, min_count=3.5)


@pytest.mark.parametrize("deconv", [(2, 2), (3, 0)])
def test_deconv_orders(gpu, deconv):
    from montecosmo_amd import metrics
    shape, box = (64, 64, 64), (500., 500., 500.)
    s0, s1 = _white_spec(shape, 3), _white_spec(shape, 4)
    for a, b in ((s0, None), (s0, s1)):
        got = metrics._spectrum(a, b, box_size=box, ells=[0, 2], box_center=(0., 0., 1.), deconv=deconv)
        want = ref.spectrum(a.astype(np.complex128), None if b is None else b.astype(np.complex128), box_size=box, ells=[0, 2],
                            box_center=(0., 0., 1.), deconv=deconv)
        _check(got, want)


def test_identities_and_empty_bins(gpu):
    from montecosmo_amd import metrics
    shape, box = (32, 32, 32), (320., 320., 320.)
    m = torch.from_numpy(np.random.default_rng(5).standard_normal(shape).astype(np.float32)).to(gpu)
    ks, tr = metrics.transfer(m, 2 * m, box)
    np.testing.assert_allclose(tr, 2., rtol=1e-12, atol=0)
    ks, coh = metrics.coherence(m, m, box)
    np.testing.assert_allclose(coh, 1., rtol=1e-12, atol=0)
    kc, km, p_auto = metrics._spectrum(m, box_size=box, ells=[0, 2])
    kc2, km2, p_cross = metrics._spectrum(m, m, box_size=box, ells=[0, 2])
    for ell in (0, 2):
        np.testing.assert_allclose(p_cross[ell], np.abs(p_auto[ell]), rtol=1e-14, atol=0)
    # edges with gaps between neighbouring mode values: empty bins are NaN where the restatement has them
    u = np.unique(ref.waves(np.array(shape), box, None, True, (0., 0., 0.))[1])[:40]
    edges = np.unique(np.concatenate([u, (2 * u[:-1] + u[1:]) / 3, (u[:-1] + 2 * u[1:]) / 3]))
    s = _white_spec(shape, 6)
    got = metrics._spectrum(s, box_size=box, kedges=list(edges))
    want = ref.spectrum(s.astype(np.complex128), box_size=box, kedges=list(edges))
    assert np.isnan(want[2]).sum() > 10
    _check(got, want)


def test_bitwise_repeat_and_batch(gpu):
    from montecosmo_amd import metrics
    shape, box = (64, 64, 64), (640., 640., 640.)
    s0 = torch.from_numpy(_white_spec(shape, 7)).to(gpu)
    s1 = torch.from_numpy(np.stack([_white_spec(shape, 10 + i) for i in range(4)])).to(gpu)
    kw = (box, (100., 200., 300.), [0, 2, 4], None, True, (0, 0))
    first = metrics._bin_sums(s0, s1[0], *kw)[2]
    for _ in range(4):
        assert np.array_equal(metrics._bin_sums(s0, s1[0], *kw)[2], first)
    batched = metrics._bin_sums(s0, s1, *kw)[2]
    assert batched.shape[0] == 4
    for i in range(4):
        assert np.array_equal(batched[i], metrics._bin_sums(s0, s1[i], *kw)[2][0])
    # spectrum with a batched mesh0, and powtranscoh with a batched mesh1: leading batch axis on every output
    km, pw = metrics.spectrum(s1, box_size=box)
    assert km.shape[0] == 4 and pw.shape[0] == 4
    out = metrics.powtranscoh(s0, s1, box)
    assert all(o.shape[0] == 4 for o in out)
    single = metrics.powtranscoh(s0, s1[2], box)
    for a, b in zip(out, single):
        assert np.array_equal(a[2], b, equal_nan=True)


# spec_layout (csrc/spectrum.hip) gives the mesh (10, 15, 8) 150 rows of the half-spectrum, one per wave, so ceil(150 / 4) = 38 workgroups:
# no multiple of the fold's 32 first-level chunks (csrc/reduce.hip).  C = ceil(38 / 32) = 2 workgroups per chunk, chunks 19 .. 31 empty.
@pytest.mark.parametrize("cross", [False, True])
def test_fold_of_ragged_workgroup_count(gpu, cross):
    from montecosmo_amd import metrics
    shape, box = (10, 15, 8), (100., 150., 80.)
    kw = dict(box_size=box, box_center=(300., -800., 2000.), ells=[0, 2])
    s = np.stack([_white_spec(shape, 20 + i) for i in range(4)])
    assert s.shape == (4, 10, 15, 5)
    d = torch.from_numpy(s).to(gpu)
    # auto: the batch on mesh0; cross: one mesh0 against a batch of mesh1
    a, a_dev, b, b_dev = (s[1:], d[1:], None, None) if not cross else (s[0], d[0], s[1:], d[1:])
    row = lambda x, i: x[i] if x is not None and x.ndim == 4 else x
    c128 = lambda x: None if x is None else x.astype(np.complex128)
    got = metrics._spectrum(row(a_dev, 0), row(b_dev, 0), **kw)
    _check(got, ref.spectrum(c128(row(a, 0)), c128(row(b, 0)), mesh_shape=shape, **kw))
    args = (box, kw["box_center"], kw["ells"], None, True, (0, 0))
    batched = metrics._bin_sums(a_dev, b_dev, *args)[2]
    assert batched.shape[0] == 3
    for i in range(3):
        assert np.array_equal(batched[i], metrics._bin_sums(row(a_dev, i), row(b_dev, i), *args)[2][0])


def test_many_workgroups_256(gpu):
    from montecosmo_amd import metrics
    shape, box = (256, 256, 256), (1000., 1000., 1000.)
    s0 = _white_spec(shape, 8)
    got = metrics._spectrum(torch.from_numpy(s0).to(gpu), box_size=box, box_center=(0., 500., 500.), ells=[0, 2])
    want = ref.spectrum(s0.astype(np.complex128), box_size=box, box_center=(0., 500., 500.), ells=[0, 2])
    _check(got, want)


def test_model_bindings(gpu):
    from montecosmo_amd import metrics
    from montecosmo_amd.model import FieldLevelForward
    fwd = FieldLevelForward(final_shape=(32, 32, 32), cell_length=10., box_center=(0., 0., 1000.))
    rng = np.random.default_rng(9)
    m0 = torch.from_numpy(rng.standard_normal((32, 32, 32)).astype(np.float32)).to(gpu)
    m1 = torch.from_numpy(rng.standard_normal((3, 32, 32, 32)).astype(np.float32)).to(gpu)
    km, pw = fwd.spectrum(m0, ells=[0, 2])
    km_r, pw_r = metrics.spectrum(m0, box_size=fwd.box_size, box_center=fwd.box_center, ells=[0, 2])
    assert np.array_equal(km, km_r, equal_nan=True)
    assert all(np.array_equal(pw[l], pw_r[l], equal_nan=True) for l in (0, 2))
    got = fwd.powtranscoh(m0, m1)
    want = metrics.powtranscoh(m0, m1, box_size=fwd.box_size)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))
