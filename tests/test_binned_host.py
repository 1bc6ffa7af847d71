"""Host side of the real-space binned diagnostics (montecosmo_amd/metrics.py): known answers of the float64 restatement
tests/_binned_f64.py, the edge logic of `metrics._vedges` against it and against np.quantile, the input checks (each fires before any
device work, so they pass without a GPU), the mask helpers and FieldLevelForward.radius_mesh."""
import numpy as np
import pytest
import torch

import _binned_f64 as ref

# (shape, box centre, cell length, edges of redges=None, cells outside the outer edges): counted once by hand with np.digitize
KNOWN = [((24, 20, 28), (0., 0., 600.), 10., 16, 399), ((17, 9, 13), (0., 0., 0.), 10., 6, 43)]


@pytest.mark.parametrize("shape,center,cell,n_edges,dropped", KNOWN)
def test_restatement_known_answers(shape, center, cell, n_edges, dropped):
    rng = np.random.default_rng(1)
    rmesh = ref.radius_mesh(shape, center, cell)
    assert len(ref.vedges(rmesh, None, 1, cell)[0]) == n_edges
    c = 2.5
    rcount, rmean, distr, dabs = ref.distr_radial(np.full(shape, c), rmesh, cell)
    assert rcount.sum() == rmesh.size - dropped
    np.testing.assert_allclose(distr, c / cell ** 3, rtol=1e-13)
    np.testing.assert_allclose(dabs, c / cell ** 3, rtol=1e-13)
    m0 = rng.standard_normal(shape)
    rcount2, rmean2, mse, _ = ref.mse_radius(m0, m0 + c, rmesh, cell)
    np.testing.assert_array_equal(rcount2, rcount)
    np.testing.assert_allclose(mse, c ** 2 * cell ** 3, rtol=1e-12)
    vcount, vmean, mse, _ = ref.mse_value(m0, m0 + c, cell, 20)
    assert vcount.sum() == m0.size - np.sum(m0 < np.quantile(m0, 1 / 40)) - np.sum(m0 >= np.quantile(m0, 39 / 40))
    np.testing.assert_allclose(mse, c ** 2 * cell ** 3, rtol=1e-12)
    assert np.all(np.diff(rmean) > 0) and np.all(np.diff(vmean) > 0)


def _meshes():
    rng = np.random.default_rng(2)
    return rng.standard_normal((30, 31, 33)).astype(np.float32), rng.poisson(2., (30, 31, 33)).astype(np.float32)


@pytest.mark.parametrize("vedges,min_count", [(7, 1), (0.3, 1), ([-1., 0., 0., 0.5, 2.], 1), (None, 1), (50, None), (0.04, None),
                                              ([0., 0.1, 0.5, 0.99, 1.], None)])
def test_vedges_equals_restatement(vedges, min_count):
    from montecosmo_amd import metrics
    for m in _meshes():
        got, mc = metrics._vedges(torch.from_numpy(m), vedges, min_count, cell_length=0.2)
        want, mc_r = ref.vedges(m, vedges, min_count, cell_length=0.2)
        assert got.dtype == np.float64 and mc == mc_r == (1 if min_count is None else min_count)
        np.testing.assert_array_equal(got, want)


def test_quantile_edges_are_np_quantile_bit_for_bit():
    from montecosmo_amd import metrics
    gauss, poisson = _meshes()
    q = np.linspace(0., 1., 50, endpoint=False) + 1 / 100
    for m in (gauss, poisson, gauss.astype(np.float64) ** 3):
        got, _ = metrics._vedges(torch.from_numpy(m), 50, None)
        np.testing.assert_array_equal(got, np.quantile(m.astype(np.float64), q))
    got, _ = metrics._vedges(torch.from_numpy(poisson), 50, None)      # tied data: 50 levels, a handful of distinct edges, accepted
    assert 2 < len(np.unique(got)) < 10 and len(got) == 50
    got, _ = metrics._vedges(torch.from_numpy(gauss.reshape(-1)[:7]), [0., 0.5, 1.], None)      # the ends of the range
    np.testing.assert_array_equal(got, np.quantile(gauss.reshape(-1)[:7].astype(np.float64), [0., 0.5, 1.]))


def test_input_checks_fire_before_any_device_work(monkeypatch):
    from montecosmo_amd import metrics, nbody

    def no_device():
        raise AssertionError("an input check came after the first device call")
    monkeypatch.setattr(nbody, "_device", no_device)
    rng = np.random.default_rng(3)
    v = rng.uniform(0., 10., (4, 5, 6))
    m0, m1 = rng.standard_normal((4, 5, 6)).astype(np.float32), rng.standard_normal((3, 4, 5, 6)).astype(np.float32)
    with pytest.raises(ValueError, match="non-decreasing"):
        metrics.mse_radius(m0, m1, v, 1., redges=[1., 3., 2.])
    with pytest.raises(ValueError, match="finite"):
        metrics.distr_radial(m0, v, 1., redges=[1., np.nan, 3.])
    with pytest.raises(ValueError, match="finite"):
        metrics.bin_and_aggregate(m0, v, [1., np.inf])
    with pytest.raises(ValueError, match="bin edges"):
        metrics.bin_and_aggregate(m0, v, list(np.linspace(0., 10., metrics.MAX_EDGES + 1)))
    with pytest.raises(ValueError, match="bin edges"):
        metrics.mse_value(m0, m1, 1., vedges=metrics.MAX_EDGES + 1)
    with pytest.raises(ValueError, match="does not match"):
        metrics.mse_radius(m0, m1, v[:3], 1.)
    with pytest.raises(ValueError, match="does not match"):
        metrics.bin_and_aggregate(m0.reshape(-1)[:-1], v, 5)
    with pytest.raises(ValueError, match="does not match"):
        metrics.mse_value(m0, m1[:, :3], 1., 5)
    with pytest.raises(ValueError, match="mask"):
        metrics.distr_radial(m0, v, 1., mask=np.ones(7, bool))
    with pytest.raises(ValueError, match="batched"):      # batched binning values
        metrics.mse_value(m1, m0, 1., 5)
    with pytest.raises(ValueError, match="batched"):
        metrics.bin_and_aggregate(m0, np.stack([v, v]), 5)
    with pytest.raises(ValueError, match="batched"):
        metrics.mse_radius(m1, m1, v, 1.)
    with pytest.raises(ValueError, match="unbatched"):      # aggr_fn with a batch
        metrics.mse_radius(m0, m1, v, 1., aggr_fn=np.median)
    with pytest.raises(ValueError, match="unbatched"):
        metrics.bin_and_aggregate(m1, v, 5, aggr_fn=np.median)


def test_aggr_fn_host_path_needs_no_device(monkeypatch):
    from montecosmo_amd import metrics, nbody
    monkeypatch.setattr(nbody, "_device", lambda: (_ for _ in ()).throw(AssertionError("the aggr_fn path is a host path")))
    rng = np.random.default_rng(4)
    shape, cell = (17, 9, 13), 10.
    rmesh = ref.radius_mesh(shape, (0., 0., 0.), cell)
    m0, m1 = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    for got, want in ((metrics.mse_radius(m0, m1, rmesh, cell, aggr_fn=np.median), ref.mse_radius(m0, m1, rmesh, cell, aggr_fn=np.median)),
                      (metrics.distr_radial(m0, rmesh, cell, redges=5, aggr_fn=np.max), ref.distr_radial(m0, rmesh, cell, redges=5, aggr_fn=np.max)),
                      (metrics.mse_value(m0, m1, cell, 12, aggr_fn=np.median), ref.mse_value(m0, m1, cell, 12, aggr_fn=np.median))):
        assert all(g.dtype == np.float64 for g in got)
        for g, w in zip(got, want[:3]):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("as_torch", [False, True])
def test_mesh2masked_round_trip(as_torch):
    from montecosmo_amd.utils import mesh2masked, masked2mesh
    rng = np.random.default_rng(5)
    mask = rng.uniform(size=(5, 4, 6)) < 0.6
    mesh = rng.standard_normal((3, 5, 4, 6)).astype(np.float32)
    x, m = (torch.from_numpy(mesh), torch.from_numpy(mask)) if as_torch else (mesh, mask)
    assert mesh2masked(x) is x and masked2mesh(x) is x and mesh2masked(x, None) is x
    v = mesh2masked(x, m)
    assert tuple(v.shape) == (3, int(mask.sum())) and v.dtype == x.dtype
    np.testing.assert_array_equal(np.asarray(v), mesh[..., mask])
    back = masked2mesh(v, m)
    assert tuple(back.shape) == mesh.shape and back.dtype == x.dtype
    np.testing.assert_array_equal(np.asarray(back), np.where(mask, mesh, 0.))
    np.testing.assert_array_equal(np.asarray(mesh2masked(back, m)), np.asarray(v))
    np.testing.assert_array_equal(np.asarray(masked2mesh(v[0], mask)), np.where(mask, mesh[0], 0.))      # unbatched, a numpy mask


@pytest.mark.parametrize("curved_sky", [True, False])
def test_radius_mesh_is_lattice_radius(curved_sky):
    from montecosmo_amd import model
    fwd = model.FieldLevelForward(final_shape=(6, 4, 8), cell_length=25., box_center=(100., -50., 400.), box_rotvec=(0.1, 0.2, -0.1),
                                  curved_sky=curved_sky)
    for shape in (None, (4, 6, 2)):
        want_shape = fwd.final_shape if shape is None else shape
        r = fwd.radius_mesh(shape)
        assert r.shape == want_shape and r.dtype == np.float64
        np.testing.assert_array_equal(r, np.asarray(fwd.lattice_radius(want_shape)).reshape(want_shape))
        p = fwd.pos_mesh(shape)
        assert p.shape == want_shape + (3,)
        if curved_sky:
            np.testing.assert_allclose(np.linalg.norm(p, axis=-1), r, rtol=1e-14)
    if curved_sky:      # an unrotated box: the closed form of the restatement
        fwd = model.FieldLevelForward(final_shape=(6, 4, 8), cell_length=25., box_center=(100., -50., 400.))
        np.testing.assert_allclose(fwd.radius_mesh(), ref.radius_mesh((6, 4, 8), (100., -50., 400.), 25.), rtol=1e-14)
