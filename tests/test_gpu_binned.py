"""Real-space binned diagnostics on the GPU (montecosmo_amd/metrics.py, csrc/binned.hip) against the float64 restatement
tests/_binned_f64.py: counts exactly (the bin of a cell is np.digitize restated bit for bit), bin means and aggregates to the float64
rounding of the sums -- 1e-10 of the bin's mean |term|, the tolerance of tests/test_gpu_spectrum.py; the worst reordering bound
2 n 2^-53 is 2e-12 at the largest n here -- bitwise reproducibility, batch rows against their own calls, aligned against misaligned
views, and the model bindings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _binned_f64 as ref  # noqa: E402

RTOL = 1e-10


def _dev(a, gpu, misaligned=False):
    """The array on the device; misaligned: as the view x[1:] of a buffer one element longer (no 16-byte alignment)."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    if not misaligned:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=gpu)
    view = buf[1:]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 != 0
    return view if t.ndim == 1 else view.reshape(t.shape)


def _vabs(values, edges, min_count=1, cell_length=None):
    """Mean |value| per kept bin: the scale of the rounding error of vmean."""
    with np.errstate(invalid="ignore"):
        return ref.bin_and_aggregate(np.abs(np.asarray(values, dtype=np.float64)), values, edges, min_count, None, cell_length)[2]


def _check(got, want, vabs):
    vc, vm, ta = got
    vc_r, vm_r, ta_r, tabs = want
    assert vc.dtype == vm.dtype == ta.dtype == np.float64
    np.testing.assert_array_equal(vc, vc_r)
    assert vm.shape == vm_r.shape and ta.shape == ta_r.shape
    err_v, err_t = np.abs(vm - vm_r), np.abs(ta - ta_r)
    print("max error / scale: vmean", np.max(err_v / np.where(vabs > 0, vabs, 1), initial=0.),
          "taggr", np.max(err_t / np.where(tabs > 0, tabs, 1), initial=0.), "bins", len(vc))
    assert np.all(err_v <= RTOL * vabs)
    assert np.all(err_t <= RTOL * tabs)


def _bitwise(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- flat sizes: one cell, one lane short of a round, a round, a round and a lane, 16 steps of 256 and three cells ------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
@pytest.mark.parametrize("vdtype", [np.float32, np.float64])
def test_flat_sizes_aligned_and_misaligned(gpu, n, vdtype):
    from montecosmo_amd import metrics
    rng = np.random.default_rng(n)
    v = rng.uniform(0., 10., n).astype(vdtype)
    v[0] = 3.                      # n = 1: the one cell is inside the edges
    t0, t1 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    edges = [1., 2.5, 2.5, 4., 7., 9.]
    cell = 1.5
    want_plain = ref.bin_and_aggregate(t0, v, edges)
    want_sq = ref.mse_radius(t0, t1, v, cell, redges=edges)
    vabs = _vabs(v, edges)
    out = {}
    for mis in (False, True):
        dv, d0, d1 = _dev(v, gpu, mis), _dev(t0, gpu, mis), _dev(t1, gpu, mis)
        out[mis] = (metrics.bin_and_aggregate(d0, dv, edges), metrics.mse_radius(d0, d1, dv, cell, redges=edges))
        _check(out[mis][0], want_plain, vabs)
        _check(out[mis][1], want_sq, vabs)
    _bitwise(out[False][0], out[True][0])      # the order of the sums does not depend on the load path
    _bitwise(out[False][1], out[True][1])
    mixed = metrics.mse_radius(_dev(t0, gpu, True), _dev(t1, gpu), _dev(v, gpu), cell, redges=edges)      # one pointer off: scalar path
    _bitwise(mixed, out[False][1])


# ---- workgroup counts that are no multiple of the fold's 32 first-level chunks ---------------------------------------------------------
# bin_layout (csrc/binned.hip) with 6 edges: nblk = min(2048, ceil(n / 1024)), cells_per_wave = 256, so n = 33 * 1024 gives 33 workgroups
# and n = 41 * 1024 + 5 gives 42, the last one with 5 cells.  The fold (csrc/reduce.hip) then has C = ceil(nblk / 32) = 2 workgroups per
# chunk: 33 leaves chunk 16 with one workgroup and chunks 17 .. 31 empty, 42 leaves chunks 21 .. 31 empty.  Batch 5 is two groups of
# rb = 4 rows, the last one short.
@pytest.mark.parametrize("n", [33 * 1024, 41 * 1024 + 5])
def test_fold_of_ragged_workgroup_counts(gpu, n):
    from montecosmo_amd import metrics
    rng = np.random.default_rng(n)
    v = rng.uniform(0., 10., n).astype(np.float32)
    t0, t1 = rng.standard_normal(n).astype(np.float32), rng.standard_normal((5, n)).astype(np.float32)
    edges = [1., 2.5, 2.5, 4., 7., 9.]
    cell = 1.5
    vabs = _vabs(v, edges)
    dv, d0, d1 = _dev(v, gpu), _dev(t0, gpu), _dev(t1, gpu)
    modes = {"plain": (lambda x: metrics.bin_and_aggregate(x, dv, edges), lambda x: ref.bin_and_aggregate(x, v, edges)),
             "squared": (lambda x: metrics.mse_radius(d0, x, dv, cell, redges=edges), lambda x: ref.mse_radius(t0, x, v, cell, redges=edges))}
    for name, (f, f_ref) in modes.items():
        full = f(d1)                                   # batch 5
        _check(full, f_ref(t1), vabs)
        assert full[2].shape == (5, len(full[0]))
        for b in range(5):                             # batch 1
            one = f(d1[b])
            if b == 0:
                _check(one, f_ref(t1[0]), vabs)
            _bitwise(one[:2], full[:2])
            np.testing.assert_array_equal(one[2], full[2][b])


# ---- 3-D meshes binned by radius, whole and through a mask ------------------------------------------------------------------------------
def _bare_logdensity(fwd, mask, gpu):
    """A FieldLevelLogDensity with only what the diagnostics read (the geometry and the mask): its constructor sets a sampler up and
    takes even shapes only."""
    from montecosmo_amd import logdensity
    ld = object.__new__(logdensity.FieldLevelLogDensity)
    ld.fwd, ld.final_shape = fwd, tuple(fwd.final_shape)
    ld.count_obs = torch.zeros(ld.final_shape, dtype=torch.float32, device=gpu)
    ld.mask = None if mask is None else torch.from_numpy(mask).to(gpu)
    return ld


@pytest.mark.parametrize("shape", [(24, 20, 28), (17, 9, 13)])
@pytest.mark.parametrize("center", [(0., 0., 600.), (100., -50., 400.)])
def test_radius_bins_of_3d_meshes_and_masks(gpu, shape, center):
    from montecosmo_amd import metrics, model
    rng = np.random.default_rng(shape[0])
    cell = 10.
    fwd = model.FieldLevelForward(final_shape=shape, cell_length=cell, box_center=center)
    rmesh = fwd.radius_mesh()
    np.testing.assert_allclose(rmesh, ref.radius_mesh(shape, center, cell), rtol=1e-13)
    m0, m1 = rng.standard_normal(shape).astype(np.float32), rng.standard_normal((3,) + shape).astype(np.float32)
    d0, d1, dr = _dev(m0, gpu), _dev(m1, gpu), _dev(rmesh, gpu)
    # the whole mesh, default shells
    _check(metrics.mse_radius(d0, d1, dr, cell), ref.mse_radius(m0, m1, rmesh, cell), _vabs(rmesh, None, 1, cell))
    _check(metrics.distr_radial(d1, dr, cell), ref.distr_radial(m1, rmesh, cell), _vabs(rmesh, None, 1, cell))
    _check(metrics.distr_radial(m0, rmesh, cell, redges=7), ref.distr_radial(m0, rmesh, cell, redges=7), _vabs(rmesh, 7))      # host inputs
    # a random mask over ~60 % of the cells: masked vectors and full meshes, against the restatement on rmesh[mask], and each other
    mask = rng.uniform(size=shape) < 0.6
    ld = _bare_logdensity(fwd, mask, gpu)
    assert ld.rmasked.dtype == torch.float64 and ld.rmasked.is_cuda and ld.rmasked is ld.rmasked
    np.testing.assert_array_equal(ld.rmasked.cpu().numpy(), rmesh[mask])
    v0, v1 = ld.mesh2masked(d0), ld.mesh2masked(d1)
    assert tuple(v1.shape) == (3, int(mask.sum()))
    for redges in (None, 9, [350., 420., 500., 650.]):
        vabs = _vabs(rmesh[mask], redges, 1, cell)
        a = ld.mse_radius(v0, v1, redges=redges)
        b = ld.mse_radius(d0, d1, redges=redges, from_masked=False)
        _check(a, ref.mse_radius(m0[mask], m1[:, mask], rmesh[mask], cell, redges=redges), vabs)
        _bitwise(a, b)
        a = ld.distr_radial(v1, redges=redges)
        b = ld.distr_radial(d1, redges=redges, from_masked=False)
        _check(a, ref.distr_radial(m1[:, mask], rmesh[mask], cell, redges=redges), vabs)
        _bitwise(a, b)
    # the module-level mask argument against the compacted arrays (another order of the same sums)
    got = metrics.mse_radius(d0, d1, dr, cell, redges=9, mask=_dev(mask, gpu))
    want = ref.mse_radius(m0[mask], m1[:, mask], rmesh[mask], cell, redges=9)
    _check(got, want, _vabs(rmesh[mask], 9))
    _check(metrics.mse_radius(v0, v1, ld.rmasked, cell, redges=9), want, _vabs(rmesh[mask], 9))


# ---- bin patterns within one 64-lane round ------------------------------------------------------------------------------------------
def _poisson_mesh():
    return np.random.default_rng(11).poisson(2., (24, 20, 28)).astype(np.float32)


def _patterns():
    rng = np.random.default_rng(7)
    n = 4099
    gauss = rng.standard_normal(n).astype(np.float32)
    pois = _poisson_mesh().reshape(-1)
    wild = rng.uniform(0., 10., n)
    wild[::5], wild[1::7], wild[2::11] = np.nan, np.inf, -np.inf
    wild[:64] = np.nan                      # a whole round without a live lane
    return {
        "one bin": (rng.uniform(1., 2., n), [0., 5.]),
        "64 distinct bins": (rng.permutation(64).astype(np.float64), list(np.arange(65) - .5)),
        "320 distinct bins": (rng.permutation(320).astype(np.float32), list(np.arange(321) - .5)),
        "edges on the data": (gauss, list(np.unique(gauss)[::7].astype(np.float64))),
        "repeated edges": (pois, list(np.quantile(pois.astype(np.float64), np.linspace(0., 1., 50, endpoint=False) + .01))),
        "4096 edges": (rng.uniform(0., 1., n), list(np.linspace(0., 1., 4096))),
        "nan and inf": (wild, [1., 2.5, 2.5, 4., 7., 9.]),
    }


@pytest.mark.parametrize("name", ["one bin", "64 distinct bins", "320 distinct bins", "edges on the data", "repeated edges", "4096 edges",
                                  "nan and inf"])
def test_bin_patterns(gpu, name):
    from montecosmo_amd import metrics
    v, edges = _patterns()[name]
    rng = np.random.default_rng(8)
    t0, t1 = rng.standard_normal(v.size).astype(np.float32), rng.standard_normal((3, v.size)).astype(np.float32)
    if name == "repeated edges":
        assert len(edges) == 50 and len(np.unique(edges)) < 10
    with np.errstate(invalid="ignore"):
        want_plain, want_sq = ref.bin_and_aggregate(t1, v, edges), ref.mse_radius(t0, t1, v, 2., redges=edges)
        vabs = _vabs(v, edges)
    if name == "nan and inf":
        assert want_plain[0].sum() == np.sum((v >= 1.) & (v < 9.))
    if name == "one bin":
        assert want_plain[0].tolist() == [v.size]
    if "distinct" in name:
        assert np.all(want_plain[0] == 1.) and len(want_plain[0]) == v.size
    _check(metrics.bin_and_aggregate(_dev(t1, gpu), _dev(v, gpu), edges), want_plain, vabs)
    _check(metrics.mse_radius(_dev(t0, gpu), _dev(t1, gpu), _dev(v, gpu), 2., redges=edges), want_sq, vabs)


# ---- mse_value ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "poisson"])
def test_mse_value_quantile_and_counted_bins(gpu, kind):
    from montecosmo_amd import metrics
    rng = np.random.default_rng(12)
    m0 = rng.standard_normal((24, 20, 28)).astype(np.float32) if kind == "gauss" else _poisson_mesh()
    m1 = (m0 + rng.standard_normal((3,) + m0.shape) * (1 + np.abs(m0))).astype(np.float32)
    cell = 7.
    d0, d1 = _dev(m0, gpu), _dev(m1, gpu)
    want = ref.mse_value(m0, m1, cell, 50, None)
    assert len(want[0]) == 49 if kind == "gauss" else 2 < len(want[0]) < 10      # tied data: most of the 49 bins are empty and removed
    _check(metrics.mse_value(d0, d1, cell, 50), want, _vabs(m0, 50, None))
    _check(metrics.mse_value(d0, d1[0], cell, [0.1, 0.5, 0.9]), ref.mse_value(m0, m1[0], cell, [0.1, 0.5, 0.9]), _vabs(m0, [0.1, 0.5, 0.9], None))
    want = ref.mse_value(m0, m1, cell, 0.25, min_count=5)
    if kind == "gauss":
        assert len(want[0]) < len(ref.mse_value(m0, m1, cell, 0.25, min_count=1)[0])      # the filter removes the thin bins of the tails
    _check(metrics.mse_value(d0, d1, cell, 0.25, min_count=5), want, _vabs(m0, 0.25, 5))
    _check(metrics.mse_value(m0, m1, cell, 30, min_count=2), ref.mse_value(m0, m1, cell, 30, min_count=2), _vabs(m0, 30, 2))      # host inputs


# ---- batch rows and repeats, to the bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 3, 5])
def test_batch_rows_and_repeats_bitwise(gpu, B, monkeypatch):
    from montecosmo_amd import metrics
    rng = np.random.default_rng(13)
    shape, cell = (24, 20, 28), 10.
    rmesh = _dev(ref.radius_mesh(shape, (0., 0., 600.), cell), gpu)
    m0, m1 = _dev(rng.standard_normal(shape).astype(np.float32), gpu), _dev(rng.standard_normal((B,) + shape).astype(np.float32), gpu)
    calls = {"radius": lambda x: metrics.mse_radius(m0, x, rmesh, cell), "value": lambda x: metrics.mse_value(m0, x, cell, 50),
             "distr": lambda x: metrics.distr_radial(x, rmesh, cell)}
    for name, f in calls.items():
        full = f(m1)
        assert full[2].shape == (B, len(full[0])) and full[0].ndim == full[1].ndim == 1
        for b in range(B):
            one = f(m1[b])
            _bitwise(one[:2], full[:2])
            np.testing.assert_array_equal(one[2], full[2][b])
        for _ in range(5):
            _bitwise(f(m1), full)
    full = calls["radius"](m1)
    monkeypatch.setattr(metrics, "CHUNK_BYTES", 1)      # one batch row per chunk
    _bitwise(calls["radius"](m1), full)


def test_aggr_fn_median_host_path(gpu):
    from montecosmo_amd import metrics
    rng = np.random.default_rng(14)
    shape, cell = (17, 9, 13), 10.
    rmesh = ref.radius_mesh(shape, (0., 0., 0.), cell)
    m0, m1 = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    got = metrics.mse_radius(_dev(m0, gpu), _dev(m1, gpu), _dev(rmesh, gpu), cell, aggr_fn=np.median)
    _bitwise(got, ref.mse_radius(m0, m1, rmesh, cell, aggr_fn=np.median)[:3])
    got = metrics.mse_value(_dev(m0, gpu), _dev(m1, gpu), cell, 12, aggr_fn=np.median)
    _bitwise(got, ref.mse_value(m0, m1, cell, 12, aggr_fn=np.median)[:3])


def test_mse_wave_vs_f64(gpu):
    from montecosmo_amd import metrics
    rng = np.random.default_rng(15)
    n = 64
    m0, m1 = rng.standard_normal((n, n, n)).astype(np.float32), rng.standard_normal((2, n, n, n)).astype(np.float32)
    box = (n * 10.,) * 3
    rtol, min_count = 2e-5, 3.5      # the figures of test_gpu_spectrum.py::test_real_mesh_input_vs_f64 for a real-mesh input
    kc, km, pw = metrics.mse_wave(_dev(m0, gpu), _dev(m1, gpu), box)
    assert pw.shape == (2, len(kc[0]))
    for b in range(2):
        kc_r, km_r, pw_r, pa_r = ref.mse_wave(m0, m1[b], box)
        np.testing.assert_array_equal(kc[b], kc_r)
        ok = kc_r > min_count
        np.testing.assert_allclose(km[b][ok], km_r[ok], rtol=rtol, atol=0)
        assert np.all(np.abs(pw[b] - pw_r)[ok] <= rtol * pa_r[ok])
    one = metrics.mse_wave(m0, m1[1], box, kedges=12, include_corners=False)      # host inputs
    want = ref.mse_wave(m0, m1[1], box, kedges=12, include_corners=False)
    np.testing.assert_array_equal(one[0], want[0])
    assert np.all(np.abs(one[2] - want[2])[want[0] > min_count] <= rtol * want[3][want[0] > min_count])


# ---- the model's bindings -------------------------------------------------------------------------------------------------------------
def test_model_bindings_on_a_cut_sky(gpu):
    from montecosmo_amd import model, logdensity
    rng = np.random.default_rng(16)
    ks = np.logspace(-3, 1, 128)
    kpow = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))
    shape, cell = (8, 8, 8), 40.      # the smallest final shape of the cut-sky tests in tests/test_gpu_model.py
    fwd = model.FieldLevelForward(final_shape=shape, cell_length=cell, box_center=(60., -40., 1400.), box_rotvec=(0.1, 0.2, -0.1),
                                  evolution="lpt", lpt_order=2, init_oversamp=1.5, evol_oversamp=2., ptcl_oversamp=2.,
                                  paint_oversamp=1., a_obs=0.65, curved_sky=True, lin_kpow=kpow)
    mask = rng.uniform(size=shape) < 0.6
    lat = {"b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2)}
    fixed = dict(Omega_m=0.3111, sigma8=0.8102, b2=0.1, bs2=-0.1, bn2=0., b3=0., bds2=0., bs3=0., bnpar=0., ngbars=1e-3, s_e=1.0, s_ed=0.,
                 s_e2=0.)
    obs = np.where(mask, rng.poisson(60., shape), 0).astype(np.float64)
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="fourier", mask_mesh=mask)
    rmesh = fwd.radius_mesh()
    np.testing.assert_array_equal(ld.rmasked.cpu().numpy(), rmesh[mask])
    m0, m1 = rng.standard_normal(shape).astype(np.float32), rng.standard_normal((3,) + shape).astype(np.float32)
    d0, d1 = _dev(m0, gpu), _dev(m1, gpu)
    v0, v1 = ld.mesh2masked(d0), ld.mesh2masked(d1)
    np.testing.assert_array_equal(ld.masked2mesh(v1).cpu().numpy(), np.where(mask, m1, 0.))
    vabs = _vabs(rmesh[mask], None, 1, cell)
    got = ld.mse_radius(v0, v1)
    _check(got, ref.mse_radius(m0[mask], m1[:, mask], rmesh[mask], cell), vabs)
    _bitwise(got, ld.mse_radius(d0, d1, from_masked=False))
    _bitwise(got, ld.mse_radius(m0[mask], m1[:, mask]))      # host inputs
    got = ld.distr_radial(v1)
    _check(got, ref.distr_radial(m1[:, mask], rmesh[mask], cell), vabs)
    _bitwise(got, ld.distr_radial(d1, from_masked=False))
    _check(ld.distr_radial(v0, cell_length=20., redges=4), ref.distr_radial(m0[mask], rmesh[mask], 20., redges=4), _vabs(rmesh[mask], 4))
    got = ld.mse_radius(v0, v1[0], aggr_fn=np.median)
    _bitwise(got, ref.mse_radius(m0[mask], m1[0][mask], rmesh[mask], cell, aggr_fn=np.median)[:3])
    _bitwise(got, ld.mse_radius(d0, d1[0], aggr_fn=np.median, from_masked=False))
    # mse_value and mse_wave forward to the forward model: its cell_length, its box_size, 50 quantile bins by default
    _check(ld.mse_value(d0, d1), ref.mse_value(m0, m1, cell, 50, None), _vabs(m0, 50, None))
    _bitwise(ld.mse_value(d0, d1), fwd.mse_value(d0, d1))
    kc, km, pw = ld.mse_wave(d0, d1[0])
    kc_r, km_r, pw_r, pa_r = ref.mse_wave(m0, m1[0], fwd.box_size)
    np.testing.assert_array_equal(kc, kc_r)
    assert np.all(np.abs(pw - pw_r)[kc_r > 3.5] <= 2e-5 * pa_r[kc_r > 3.5])
    # without a mask every cell is observed
    ld0 = _bare_logdensity(fwd, None, gpu)
    _check(ld0.mse_radius(d0, d1), ref.mse_radius(m0, m1, rmesh, cell), _vabs(rmesh, None, 1, cell))
    assert ld0.mesh2masked(d0) is d0 and ld0.masked2mesh(d0) is d0
