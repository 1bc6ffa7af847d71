"""Catalogue registration on the GPU: the five passes of csrc/catalog.hip against numpy float64, then `register_catalog` end to
end (cut sky and full sky) against the float64 chain of tests/_catalog_f64.py, its reproducibility, and the way from a catalogue
to one log density.

Gates.  Coordinates: the kernels work in float64 and round once, so a result lies within 1 float32 ulp of the float64 reference
rounded to float32 (half an ulp of rounding, half for ties moved by last-bit differences in sin / cos).  Meshes: relative L2 1e-5,
the gate tests/test_gpu_nufft.py holds `nufft` to.  Masks: exact; on the end-to-end case the product's positions are float32 where
the chain's are float64, so cells whose reference value depends on objects within 1e-4 cells of a cell face ("fragile") are set
aside -- the chain has none at either mask shape for this input, so any disagreement fails."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _catalog_f64 as ref  # noqa: E402
from oracle import pm_oracle as o, background as obg  # noqa: E402  (checker only)

SIZES = [1, 63, 64, 65, 257, 4099]
GEOM = dict(box_center=(-700., 1100., 650.), box_rotvec=(0.1, -0.2, 0.3), box_size=(1500., 1300., 1100.))
SHAPE = (28, 24, 20)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def within_ulp32(got, want64, ulps=1):
    """|got - float32(want64)| <= ulps float32 ulps of float32(want64), elementwise."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("max error in float32 ulps", float(np.max(err / np.spacing(np.abs(want)).astype(np.float64))))
    return bool(np.all(err <= ulps * np.spacing(np.abs(want)).astype(np.float64)))


@pytest.fixture(scope="module")
def br(gpu):
    from montecosmo_amd import bricks
    return bricks


def sky_objects(n, seed=0):
    """n objects on the sky; the first ones are the edge cases: both poles, RA = 0 and 360, z = 0, z beyond the table (clamped)."""
    rng = np.random.default_rng(seed)
    d = {'RA': rng.uniform(0, 360, n), 'DEC': np.rad2deg(np.arcsin(rng.uniform(-1, 1, n))), 'Z': rng.uniform(0.01, 2.5, n)}
    edge = [(10., 90., 0.5), (200., -90., 0.7), (0., 20., 0.3), (360., -35., 1.1), (77., 12., 0.), (150., 40., 2000.)]
    for i, (ra, dec, z) in enumerate(edge[:n]):
        d['RA'][i], d['DEC'][i], d['Z'][i] = ra, dec, z
    return d


@pytest.mark.parametrize("n", SIZES)
def test_sky2cell(br, n):
    d = sky_objects(n)
    cosmo = br.Planck18()
    want = ref.sky2cell(obg.Planck18(), d, GEOM['box_center'], GEOM['box_rotvec'], GEOM['box_size'], SHAPE)
    got = br.sky2cell_pos(cosmo, d, mesh_shape=SHAPE, **GEOM)
    assert got.shape == (n, 3) and within_ulp32(got.cpu().numpy(), want)
    ratio = np.divide((18, 16, 14), SHAPE)
    got1, got2 = br.sky2cell_pos(cosmo, d, mesh_shape=SHAPE, ratio=ratio, **GEOM)
    assert torch.equal(got1, got)
    assert np.array_equal(got2.cpu().numpy(), got.cpu().numpy() * ratio.astype(np.float32))      # `pos *= ratio` on the float32 result


@pytest.mark.parametrize("n", SIZES)
def test_sky_extent(br, n):
    d = sky_objects(n, seed=1)
    w = np.random.default_rng(2).uniform(0.5, 1.5, n)
    cart = ref.radecz2cart(obg.Planck18(), d)
    lo, hi, ws = br.sky_extent(br.Planck18(), d, w)
    tol = 64 * np.spacing(np.abs(cart).max())
    print("min/max error in ulps of max|x|", np.abs(lo - cart.min(0)).max() / (tol / 64), np.abs(hi - cart.max(0)).max() / (tol / 64))
    assert np.all(np.abs(lo - cart.min(0)) <= tol) and np.all(np.abs(hi - cart.max(0)) <= tol)
    assert abs(ws - w.sum()) <= n * 2. ** -53 * w.sum()
    lo2, hi2, ws2 = br.sky_extent(br.Planck18(), d, w)
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2) and ws == ws2                       # bitwise, call after call
    assert br.sky_extent(br.Planck18(), d)[2] == 0.


def test_sky_extent_of_nothing(br):
    none = {'RA': np.zeros(0), 'DEC': np.zeros(0), 'Z': np.zeros(0)}
    lo, hi, ws = br.sky_extent(br.Planck18(), none, np.zeros(0))
    assert np.all(lo == np.inf) and np.all(hi == -np.inf) and ws == 0.
    assert br.sky2cell_pos(br.Planck18(), none, mesh_shape=SHAPE, **GEOM).shape == (0, 3)


@pytest.mark.parametrize("n", [1, 65, 4099])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_vel", [False, True])
def test_box2cell(br, n, dtype, with_vel):
    rng = np.random.default_rng(3)
    pos = rng.uniform(-700, 800, (n, 3)).astype(dtype)
    vel = (300 * rng.standard_normal((n, 3))).astype(dtype) if with_vel else None
    los = np.array([0.6, 0., 0.8])
    vscale = 1. / (0.7 * 100 * obg.Esqr(obg.Planck18(), 0.7) ** .5)
    geom = dict(box_center=(50., 0., 0.), box_rotvec=(0., 0.3, -0.1), box_size=(1500., 1500., 1600.))
    want = ref.box2cell(pos, vel, los, vscale, mesh_shape=(16, 18, 20), **geom)
    got = br.box2cell_pos(pos, vel, los, vscale, mesh_shape=(16, 18, 20), **geom)
    assert got.shape == (n, 3) and within_ulp32(got.cpu().numpy(), want)


FP_SHAPE = (16, 12, 20)


def footprint_objects(n):
    """float32 positions on FP_SHAPE: random ones, then (from the front) a fraction of exactly 0 on every axis, on one axis,
    positions at shape - 0.5 (the upper neighbour wraps to 0), negative ones, one exactly at 0.5 above an even and an odd cell
    (NGP rounds half to even) and one beyond the box."""
    rng = np.random.default_rng(5)
    pos = (rng.uniform(-0.2, 1.2, (n, 3)) * np.array(FP_SHAPE)).astype(np.float32)
    edge = np.array([[3., 5., 7.], [4.25, 6., 2.75], [15.5, 11.5, 19.5], [-0.25, -3.5, -1e-9], [2.5, 3.5, 8.5], [17., 30.25, -21.75]],
                    dtype=np.float32)
    pos[:min(n, len(edge))] = edge[:n]
    return pos


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_footprint(br, order, n):
    pos = footprint_objects(n)
    rng = np.random.default_rng(6)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    want = ref.footprint(pos, FP_SHAPE, None, order)
    got = br.footprint(pos, FP_SHAPE, None, order).cpu().numpy()
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)                                                # exactly
    if n == 1 and order == 2:
        assert want.sum() == 1 and want[3, 5, 7]                                                 # fraction 0: no upper neighbour
    assert np.array_equal(br.footprint(pos, FP_SHAPE, w, order).cpu().numpy().astype(bool), want)
    w0 = w.copy()
    w0[::2] = 0.                                                                                 # zero-weight objects mark nothing
    got0 = br.footprint(pos, FP_SHAPE, w0, order).cpu().numpy().astype(bool)
    assert np.array_equal(got0, ref.footprint(pos, FP_SHAPE, w0, order)) and np.array_equal(got0, ref.footprint(pos[1::2], FP_SHAPE, None, order))
    assert not br.footprint(pos, FP_SHAPE, np.zeros(n, np.float32), order).any()
    perm = rng.permutation(n)
    assert np.array_equal(br.footprint(pos[perm], FP_SHAPE, w[perm], order).cpu().numpy().astype(bool), want)      # any order
    half = n // 2
    part = br.footprint(pos[:half], FP_SHAPE, w[:half], order)                                   # two chunks are one call
    both = br.footprint(pos[half:], FP_SHAPE, w[half:], order, mask=part)
    assert both is part and np.array_equal(both.cpu().numpy().astype(bool), want)


@pytest.mark.parametrize("shape", [(1, 1, 7), (16, 12, 20), (64, 70, 130)])
def test_masked_sum(br, shape):
    rng = np.random.default_rng(7)
    mesh = (1. + rng.standard_normal(shape)).astype(np.float32)
    mask = rng.uniform(size=shape) < 0.4
    s, c = br.masked_sum(mesh, mask)
    want = mesh.astype(np.float64)[mask].sum()      # (0.66, 1.5e3 and 2.3e5 on these draws: no cancellation to speak of)
    print("masked sum: relative error", abs(s - want) / abs(want))
    assert c == int(mask.sum()) and abs(s - want) <= 1e-12 * abs(want)
    assert br.masked_sum(mesh, mask) == (s, c)                                                   # bitwise repeatable
    assert br.masked_sum(mesh, mask.astype(np.uint8) * 7) == (s, c)                              # any non-zero byte is "in"
    assert br.masked_sum(mesh, np.zeros(shape, bool)) == (0., 0)


# ------------------------------------------------------------------------------------------------
def _sky(rng, n):
    ra = rng.uniform(100, 140, n)
    sin_dec = rng.uniform(np.sin(np.deg2rad(10)), np.sin(np.deg2rad(40)), n)
    z, w = rng.uniform(0.4, 0.7, n), rng.uniform(0.5, 1.5, n)
    return {'RA': ra, 'DEC': np.rad2deg(np.arcsin(sin_dec)), 'Z': z, 'WEIGHT': w}


@pytest.fixture(scope="module")
def cutsky(gpu):
    """The catalogue, the float64 chain on it and two product runs, computed once for the tests below."""
    from montecosmo_amd import bricks, register
    rng = np.random.default_rng(0)
    random, data = _sky(rng, 40000), _sky(rng, 5000)
    want = ref.register_catalog(16 ** 3, obg.Planck18(), data, random, padding=0.2)
    run = lambda: register.register_catalog(16 ** 3, bricks.Planck18(), data, random, padding=0.2)
    return dict(random=random, data=data, want=want, got=run(), again=run())


def test_cutsky_end_to_end(cutsky, br):
    from montecosmo_amd import register, utils
    got, want, random = cutsky["got"], cutsky["want"], cutsky["random"]
    register.validate(got)
    assert isinstance(got["count_mesh"], np.ndarray) and isinstance(got["selec_mesh"], np.ndarray) and got["mask_mesh"].dtype == bool
    assert want["final_shape"] == (18, 16, 14) and want["init_shape"] == (28, 24, 20) and want["paint_shape"] == (32, 28, 24)
    assert got["count_mesh"].shape == want["final_shape"] == got["mask_mesh"].shape and got["selec_mesh"].shape == want["paint_shape"]
    assert utils.scale_shape(got["count_mesh"].shape, got["init_oversamp"]) == want["init_shape"]
    assert got["curved_sky"] is True and got["a_obs"] is None and got["kernel_type"] == "rectangular"
    assert abs(got["cell_length"] - want["cell_length"]) <= 1e-12 * want["cell_length"]
    assert np.all(np.abs(got["box_center"] - want["box_center"]) <= 1e-12 * np.abs(want["box_center"]))
    assert np.array_equal(got["box_rotvec"], want["box_rotvec"])                                  # zeros: 1e-12 relative is equality
    errs = rel_l2(got["count_mesh"], want["count_mesh"]), rel_l2(got["selec_mesh"], want["selec_mesh"])
    print("count, selection rel L2", errs)
    assert max(errs) < 1e-5
    assert abs(got["n_tracers"] - want["n_tracers"]) <= 1e-12 * want["n_tracers"]
    assert abs(got["n_randoms"] - want["n_randoms"]) <= 1e-12 * want["n_randoms"]
    # masks: at final_shape (the register's) and at init_shape (the one the selection is normalised over)
    cfg = dict(box_size=want["box_size"], box_center=want["box_center"], box_rotvec=want["box_rotvec"])
    selec, mask = br.cutsky2selection(random, br.Planck18(), want["final_shape"], want["init_shape"], want["paint_shape"], **cfg)
    assert np.array_equal(mask.cpu().numpy(), got["mask_mesh"])
    pos = br.sky2cell_pos(br.Planck18(), random, mesh_shape=want["init_shape"], **cfg)
    mask_selec = br.footprint(pos, want["init_shape"], random['WEIGHT'], 2).cpu().numpy().astype(bool)
    mean = selec.cpu().numpy().astype(np.float64)[mask_selec].mean()
    print("mean of the selection over its footprint", mean)
    assert abs(mean - 1.) < 1e-6
    d_selec, d_mask = ref.face_distance(obg.Planck18(), random, selec_shape=want["init_shape"], mask_shape=want["final_shape"], **cfg)
    for mine, theirs, dist, key in ((mask_selec, want["mask_selec"], d_selec, 1), (got["mask_mesh"], want["mask_mesh"], d_mask, 2)):
        sturdy = ref.cutsky2selection(random, obg.Planck18(), want["final_shape"], want["init_shape"], want["paint_shape"],
                                      keep=dist >= 1e-4, **cfg)[key]
        fragile = sturdy != theirs
        print("fragile cells", int(fragile.sum()), "of", int(theirs.sum()), "disagreements", int((mine != theirs).sum()))
        assert fragile.sum() <= 0.005 * theirs.sum()
        assert np.array_equal(mine[~fragile], theirs[~fragile])


def test_cutsky_is_reproducible_and_chunks_agree(cutsky, br):
    from montecosmo_amd import register
    got, again = cutsky["got"], cutsky["again"]
    for k in ("count_mesh", "selec_mesh", "mask_mesh"):
        assert np.array_equal(got[k], again[k]), k                                               # bitwise
    assert got["n_tracers"] == again["n_tracers"] and got["n_randoms"] == again["n_randoms"] and got["cell_length"] == again["cell_length"]
    random, data = cutsky["random"], cutsky["data"]
    cut = lambda d, i: {k: v[i] for k, v in d.items()}
    parts = [cut(random, slice(0, 15000)), cut(random, slice(15000, 40000))]
    chunked = register.register_catalog(16 ** 3, br.Planck18(), (data,), parts, padding=0.2, chunk=7000)
    assert np.array_equal(chunked["mask_mesh"], got["mask_mesh"]) and chunked["count_mesh"].shape == got["count_mesh"].shape
    # (the same float32 paints summed in another grouping: a few roundings of 6e-8 each, the full-sky gate for chunks)
    assert rel_l2(chunked["count_mesh"], got["count_mesh"]) < 1e-6 and rel_l2(chunked["selec_mesh"], got["selec_mesh"]) < 1e-6
    assert abs(chunked["n_randoms"] - got["n_randoms"]) <= 1e-12 * got["n_randoms"]
    assert np.all(np.abs(chunked["box_center"] - got["box_center"]) <= 1e-12 * np.abs(got["box_center"]))


def test_fullsky_end_to_end(br):
    from montecosmo_amd import model, register
    rng = np.random.default_rng(1)
    n = 20000
    data = {'pos': rng.uniform(0, 640, (n, 3)), 'vel': 300 * rng.standard_normal((n, 3))}
    kw = dict(box_size=(640., 640., 640.), box_center=(0., 0., 0.), a_obs=0.7, los=(0., 0., 1.))
    want = ref.register_catalog(16 ** 3, obg.Planck18(), data, **kw)
    got = model.FieldLevelForward.register_catalog(16 ** 3, br.Planck18(), data, **kw)
    register.validate(got)
    assert got["count_mesh"].shape == want["final_shape"] == (16, 16, 16) and got["selec_mesh"] is None and got["mask_mesh"] is None
    assert got["curved_sky"] is False and got["a_obs"] == 0.7 and got["n_randoms"] is None
    err = rel_l2(got["count_mesh"], want["count_mesh"])
    print("count rel L2", err)
    assert err < 1e-5
    assert abs(got["count_mesh"].sum(dtype=np.float64) - n) <= 1e-5 * n and abs(got["n_tracers"] - n) <= 1e-5 * n
    chi = o.a2chi(obg.Planck18(), 0.7)
    assert np.all(np.abs(got["box_center"] - np.array([0., 0., chi])) <= 1e-12 * chi)
    cut = lambda i: {k: v[i] for k, v in data.items()}
    three = [cut(slice(0, 5000)), cut(slice(5000, 5001)), cut(slice(5001, n))]
    assert rel_l2(register.register_catalog(16 ** 3, br.Planck18(), three, **kw)["count_mesh"], got["count_mesh"]) < 1e-6
    assert rel_l2(register.register_catalog(16 ** 3, br.Planck18(), iter(three), chunk=3000, **kw)["count_mesh"], got["count_mesh"]) < 1e-6
    weighted = dict(data, WEIGHT=rng.uniform(0.5, 1.5, n))                                        # weights, float32 positions, no velocities
    weighted.pop('vel')
    weighted['pos'] = weighted['pos'].astype(np.float32)
    gw = register.register_catalog(16 ** 3, br.Planck18(), weighted, **kw)
    assert rel_l2(gw["count_mesh"], ref.register_catalog(16 ** 3, obg.Planck18(), weighted, **kw)["count_mesh"]) < 1e-5
    assert abs(gw["n_tracers"] - weighted['WEIGHT'].sum()) <= 1e-5 * n


def test_catalog_to_log_density(cutsky, br, tmp_path):
    """register_catalog -> save_register -> load_register -> model_arguments -> the Kaiser model and its log density: one finite
    value with finite gradients at the fiducial point."""
    from montecosmo_amd import logdensity, model, register
    path = register.save_register(tmp_path / "mock.npz", cutsky["got"])
    reg = register.load_register(path)
    assert "a_obs" not in reg and reg["curved_sky"] is True and np.array_equal(reg["mask_mesh"], cutsky["got"]["mask_mesh"])
    args = register.model_arguments(reg, evolution="kaiser")
    fwd = model.FieldLevelForward(**args["forward"])
    assert fwd.final_shape == (18, 16, 14) and fwd.init_shape == (28, 24, 20) and fwd.paint_shape == (32, 28, 24)
    loc = args["loc"]
    lat = {"Omega_m": dict(loc=loc["Omega_m"], scale=0.1, loc_fid=loc["Omega_m"], scale_fid=1e-2, low=0.05, high=1.),
           "sigma8": dict(loc=loc["sigma8"], scale=0.1, loc_fid=loc["sigma8"], scale_fid=1e-2, low=0., high=np.inf),
           "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2)}
    # the stochastic parameters at the reference's fiducial values (model.py:215-247: s_e = 1, s_ed = s_e2 = 0).  Away from s_e2 = 0 the
    # QuadGaussian's support is bounded below by -scale1^2 / (4 scale2) ~ -sqrt(selec) / (4 s_e2), which the thinly covered cells at the
    # edge of the footprint leave at once (model.py:899-900 says as much): -inf there is the density's answer, not a fault.
    fixed = dict(b2=0., bs2=0., bn2=0., bnpar=0., b3=0., bds2=0., bs3=0., ngbars=loc["ngbars"], s_e=1.0, s_ed=0., s_e2=0.)
    ld = logdensity.FieldLevelLogDensity(fwd, args["density"]["count_mesh"], lat, fixed, precond="kaiser",
                                         selec_mesh=args["density"]["selec_mesh"], mask_mesh=args["density"]["mask_mesh"])
    sample = {k + "_": 0. for k in lat}
    sample["white_mesh_"] = np.random.default_rng(8).standard_normal(fwd.init_shape).astype(np.float32)
    lp, grad = ld.logdensity_and_grad(sample)
    print("log density", lp)
    assert np.isfinite(lp) and set(grad) == set(sample)
    for k, g in grad.items():
        g = g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        assert np.all(np.isfinite(g)), k
    assert float(np.abs(grad["white_mesh_"].cpu().numpy() if torch.is_tensor(grad["white_mesh_"]) else grad["white_mesh_"]).max()) > 0
