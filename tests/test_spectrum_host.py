"""Host side of the binned spectra (montecosmo_amd/metrics.py): the float64 restatement tests/_spectrum_f64.py against an
analytic plane wave, metrics' edge logic against the restatement's, and the input checks that fire before any device work."""
import numpy as np
import pytest

from montecosmo_amd import metrics
import _spectrum_f64 as ref


@pytest.mark.parametrize("shape,box,m", [((16, 16, 16), (160., 160., 160.), (2, 3, 4)), ((12, 16, 10), (60., 160., 50.), (-3, 5, 2))])
def test_plane_wave_power_in_one_bin(shape, box, m):
    x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    mesh = np.cos(2 * np.pi * sum(mi * xi / n for mi, xi, n in zip(m, x, shape)))
    kcount, kmean, pow, _ = ref.spectrum(mesh, box_size=box, kedges=None)
    kvec = [2 * np.pi * mi / b for mi, b in zip(m, box)]
    km = np.sqrt(sum(k ** 2 for k in kvec))
    edges = ref.waves(np.array(shape), box, None, True, (0., 0., 0.))[0]
    ib = np.digitize(km, edges) - 1
    M = np.prod(shape)
    expect = 2 * (M / 2) ** 2 * np.prod(np.asarray(box) / np.asarray(shape) ** 2) / kcount[ib]
    np.testing.assert_allclose(pow[ib], expect, rtol=1e-12)
    others = np.delete(pow, ib)
    assert np.all(np.abs(others[np.isfinite(others)]) < 1e-12 * expect)


@pytest.mark.parametrize("shape,box", [((64, 64, 64), (640., 640., 640.)), ((48, 64, 40), (480., 640., 400.)),
                                       ((32, 16, 24), (100., 300., 50.))])
@pytest.mark.parametrize("kedges", [None, 10, 0.03, [0.01, 0.02, 0.05, 0.1, 0.2]])
@pytest.mark.parametrize("corners", [True, False])
def test_edges_match_restatement(shape, box, kedges, corners):
    got = metrics._kedges(shape, box, kedges, corners)
    want = ref.waves(np.array(shape), box, kedges, corners, (0., 0., 0.))[0]
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, want)


def test_rejects_bad_input():
    with pytest.raises(ValueError):
        metrics.spectrum(np.zeros((8, 8, 8), np.float32), box_size=(8., 8., 8.), kedges=[0.1, 0.3, 0.3, 0.5])
    with pytest.raises(ValueError):
        metrics.spectrum(np.zeros((8, 8, 8), np.float32), kedges=[0.5, 0.3])
    with pytest.raises(ValueError):
        metrics.spectrum(np.zeros((8, 8, 7), np.float32))
    with pytest.raises(ValueError):
        metrics.spectrum(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        metrics.spectrum(np.zeros((2, 2, 8, 8, 8), np.float32))
    with pytest.raises(ValueError):
        metrics._kedges((8, 8, 8), (8., 8., 8.), list(np.linspace(0.1, 1., metrics.MAX_EDGES + 1)))
