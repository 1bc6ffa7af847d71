"""The 'shash', 'poisson' and 'fourier_gauss' likelihoods on the HIP path (csrc/likelihood.hip, logdensity.py) against their float64
restatement (tests/_lik_f64.py): the kernels through the ABI, the log density and its gradient on the set-up of tests/test_gpu_model.py,
and two answers known from the 'quad_gauss' path.

TOLERANCE RULE of the kernel-level tests.  The restatement is run twice on the same float32-rounded inputs (meshes AND scalars: the ABI
takes float scalars), in float64 and in float32 (numpy on the CPU).  The float32 run's deviation from the float64 run is what single
precision delivers for these formulas; the kernel is held to 4 x that deviation (a different summation order, ocml instead of libm
transcendentals).  For a mesh the deviation is max |x32 - x64| over the mesh.  For a sum, both sides add in float64, so its error is the
sum of its terms' errors d_i = t32_i - t64_i, which have a part common to all cells (a rounded scalar such as sqrt(selec) enters every
cell alike) and a part of their own: the deviation is max(|sum d_i|, sqrt(sum d_i^2)) -- the signed sum as it is, and never less than the
expected size of the independent part, because the signed sum of one realisation can cancel to nothing by chance and would make a bound
that means nothing.  Nothing is fixed in advance; the tests print what they measure.
Measured on the MI355X, float32 restatement's deviation / kernel's error, the case with the least room of each kind:
    shash   lp 1.25e-5 / 1.37e-5   d s_e 4.76e-5 / 1.05e-4   d s_ed 1.30e-5 / 2.57e-5   d s_e2 1.68e-4 / 1.85e-4   count_bar 3.30e-7 / 3.66e-7
            sqsel_bar 4.09e-7 / 6.00e-7 (mesh), 9.45e-7 / 1.63e-6 (its sum)
    poisson lp 6.18e-4 / 2.3e-12 (the kernel forms this value in float64)   count_bar 5.92e-8 / 5.92e-8
    fourier lp 8.31e-6 / 7.06e-6   d s_e 1.23e-5 / 1.79e-5   d s_k2e 5.03e-8 / 9.72e-8   d s_kmu2e 7.98e-8 / 1.46e-7   d sqrt(selec) 1.75e-6 / 2.83e-6
            Y_bar 4.04e-8 / 5.2e-9
Known answers (test_known_answer_against_quad_gauss), difference of the two routes / float32 deviation: fourier_gauss lp 1.3e-4 / 4.3e-4,
s_e_ 1e-6 / 2.8e-6, white_mesh_ 2.7e-7 / 3.0e-7 relative; shash lp 1.1e-4 / 2.1e-4, s_e_ 1e-6 / 1.5e-6, white_mesh_ 2.0e-7 / 2.2e-7."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _lik_f64 as L  # noqa: E402
from oracle import pm_oracle as o, bias_oracle as bo, background as obg  # noqa: E402  (checker only)

SHAPE = (6, 10, 14)      # 840 cells: four workgroups of 256, the last one partly filled


def _dev_sum(c32, c64):
    d = (c32 - c64).reshape(c64.shape[0], -1)
    return np.maximum(np.abs(d.sum(1)), np.sqrt((d ** 2).sum(1)))


def _gate(name, got, want, dev):
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))
    print(f"  {name}: float32 restatement deviates {float(dev):.3e}, kernel errs {err:.3e} (|value| <= {float(np.max(np.abs(want))):.3e})")
    assert err <= 4 * float(dev), (name, err, float(dev))


def _real_inputs(family, masked, mesh_sel, seed=7):
    rng = np.random.default_rng(seed)
    count = rng.uniform(35., 95., SHAPE).astype(np.float32)
    if family == "poisson":      # a few negative mean counts: the rate is |count|, the gradient carries the sign
        count.reshape(-1)[::97] *= -1.
    obs = np.rint(np.abs(count) + 8. * rng.standard_normal(SHAPE)).clip(0).astype(np.float32)
    selec = rng.uniform(50., 80., SHAPE).astype(np.float32) if mesh_sel else np.float32(64.5)
    mask = (rng.uniform(size=SHAPE) < 0.8) if masked else None
    if family == "poisson":      # lambda = 0 with obs > 0 (-inf, alone in its test), and with obs = 0
        count[0, 0, 3], obs[0, 0, 3] = 0., 0.
        count[5, 9, 13], obs[5, 9, 13] = -0., 0.
    if masked:      # what an unobserved cell may hold: an exactly zero selection, a NaN observation
        obs[~mask] = np.nan
        if mesh_sel:
            selec[~mask] = 0.
    return obs, count, selec, mask


def _call_real(family, obs, count, selec, mask, st, want_sq=True):
    import torch
    from montecosmo_amd import nbody, _lib
    plan = nbody.get_plan(SHAPE)
    d = lambda a: nbody._f32(a)
    ob, ct = d(obs), d(count)
    sel = d(selec) if np.ndim(selec) else None
    mk = None if mask is None else torch.from_numpy(mask).to(ob.device)
    cb, qb = torch.full_like(ct, float("nan")), (torch.full_like(ct, float("nan")) if want_sq else None)
    sums = torch.full((5,), float("nan"), dtype=torch.float64, device=ob.device)
    plan.call("mcpm_lik_real_f32", _lib.LIK_SHASH if family == "shash" else _lib.LIK_POISSON, C.c_int64(ct.numel()), nbody._ptr(ob),
              nbody._ptr(ct), nbody._ptr(sel), 1.0 if sel is not None else float(selec), nbody._ptr(mk), *[float(v) for v in st],
              nbody._ptr(cb), nbody._ptr(qb), nbody._ptr(sums))
    return cb.cpu().numpy(), None if qb is None else qb.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("family,masked,mesh_sel,s_e2", [("shash", False, False, 0.08), ("shash", True, True, -0.08), ("shash", True, False, 0.0),
                                                         ("shash", False, True, 0.08), ("poisson", False, False, 0.), ("poisson", True, True, 0.)])
def test_real_space_kernel(gpu, family, masked, mesh_sel, s_e2):
    """mcpm_lik_real_f32 through the ABI: the five sums and the two meshes within 4 x the float32 restatement's deviation, bitwise equal
    across two calls, exact zeros (and no NaN) in the unobserved cells."""
    obs, count, selec, mask = _real_inputs(family, masked, mesh_sel)
    st = tuple(float(np.float32(v)) for v in (0.9, 0.4, s_e2))
    r64 = L.real_terms(family, obs, count, selec, mask, *st)
    r32 = L.real_terms(family, obs, count, selec, mask, *st, dtype=np.float32)
    cb, qb, sums = _call_real(family, obs, count, selec, mask, st)
    cb2, qb2, sums2 = _call_real(family, obs, count, selec, mask, st)
    assert np.array_equal(cb, cb2) and np.array_equal(qb, qb2) and np.array_equal(sums, sums2)      # bitwise
    assert np.isfinite(cb).all() and np.isfinite(qb).all() and np.isfinite(sums).all()
    if masked:
        assert not cb[~mask].any() and not qb[~mask].any()
    print(f"\n{family} masked={masked} mesh_sel={mesh_sel} s_e2={s_e2}")
    dev = _dev_sum(r32["cells"], r64["cells"])
    for i, k in enumerate(("lp", "d s_e", "d s_ed", "d s_e2", "sum sqsel_bar")):
        if family == "poisson" and i:
            assert sums[i] == 0.
            continue
        _gate(k, sums[i], r64["sums"][i], dev[i])
    _gate("count_bar", cb, r64["count_bar"], np.abs(r32["count_bar"] - r64["count_bar"]).max())
    if family == "shash":
        _gate("sqsel_bar", qb, r64["sqsel_bar"], np.abs(r32["sqsel_bar"] - r64["sqsel_bar"]).max())
    cb3, qb3, sums3 = _call_real(family, obs, count, selec, mask, st, want_sq=False)      # without the second mesh: the same numbers
    assert qb3 is None and np.array_equal(cb, cb3) and np.array_equal(sums, sums3)


def test_poisson_zero_rate_with_counts_is_minus_infinity(gpu):
    obs, count, selec, mask = _real_inputs("poisson", False, False)
    count[2, 3, 4], obs[2, 3, 4] = 0., 3.
    cb, _, sums = _call_real("poisson", obs, count, selec, mask, (0., 0., 0.))
    assert sums[0] == -np.inf and cb[2, 3, 4] == 0. and np.isfinite(cb).all()
    assert L.real_terms("poisson", obs, count, selec, mask)["sums"][0] == -np.inf


@pytest.mark.parametrize("shape", [(4, 6, 8), (6, 8, 10)])      # one workgroup (120 modes), two (288); unequal even sides: every face, edge, corner
def test_fourier_kernel(gpu, shape):
    """mcpm_lik_fourier_f32 through the ABI: sums and Y_bar within 4 x the float32 restatement's deviation; every stored mode written (the
    output buffer starts as NaN), zeros exactly where the restatement's adjoint has them (the redundant mirror modes); bitwise repeatable."""
    import torch
    from montecosmo_amd import nbody
    rng = np.random.default_rng(11)
    box = tuple(float(np.float32(25. * n * f)) for n, f in zip(shape, (1.0, 1.2, 0.9)))
    los = np.array([0.3, -0.5, 0.81])
    los = (los / np.linalg.norm(los)).astype(np.float32).astype(np.float64)
    count = rng.uniform(40., 90., shape)
    obs = count + 8. * rng.standard_normal(shape)
    Y = np.fft.rfftn(count).astype(np.complex64)
    org = o.cgh2rg(np.fft.rfftn(obs)).astype(np.float32)
    pr = tuple(float(np.float32(v)) for v in (60., -1.1, -8., -10.))      # selec, s_e, s_k2e, s_kmu2e (all negative: the |.| of the scale)
    t64 = L.fourier_terms(Y, org, box, los, *pr)
    t32 = L.fourier_terms(Y, org, box, los, *pr, dtype=np.float32)
    plan = nbody.get_plan(shape)
    Yd, od = nbody._c64(Y), nbody._f32(org)

    def call():
        Yb = torch.full_like(Yd, complex(float("nan"), float("nan")))
        sums = torch.full((5,), float("nan"), dtype=torch.float64, device=Yd.device)
        plan.call("mcpm_lik_fourier_f32", nbody._ptr(Yd), nbody._ptr(od), *[float(b) for b in box], *[float(v) for v in los], float(pr[0]),
                  *[float(v) for v in pr[1:]], nbody._ptr(Yb), nbody._ptr(sums))
        return Yb.cpu().numpy(), sums.cpu().numpy()
    Yb, sums = call()
    Yb2, sums2 = call()
    assert np.array_equal(Yb.view(np.float32), Yb2.view(np.float32)) and np.array_equal(sums, sums2)
    assert np.isfinite(Yb.view(np.float32)).all()
    zero = (t64["Y_bar"].real == 0, t64["Y_bar"].imag == 0)
    assert zero[0].sum() + zero[1].sum() == 2 * Y.size - int(np.prod(shape))      # as many cotangents as real elements, the rest zero
    assert not Yb.real[zero[0]].any() and not Yb.imag[zero[1]].any()
    print(f"\nfourier_gauss {shape}")
    dev = _dev_sum(t32["cells"], t64["cells"])
    for i, k in enumerate(("lp", "d s_e", "d s_k2e", "d s_kmu2e", "d sqrt(selec)")):
        _gate(k, sums[i], t64["sums"][i], dev[i])
    scale = np.sqrt(2. / np.prod(shape))      # Y_bar = scale * (+-1 or 1 / sqrt2) * loc_bar: the deviation of loc_bar carries over
    _gate("Y_bar", np.stack([Yb.real, Yb.imag]), np.stack([t64["Y_bar"].real, t64["Y_bar"].imag]),
          scale * np.abs(t32["loc_bar"] - t64["loc_bar"]).max())


# ---- model level: the set-up of tests/test_gpu_model.py ---------------------------------------------------------------------------
def _kpow():
    ks = np.logspace(-3, 1, 128)
    return ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6)


def _cos(c, s8):
    c.sigma8 = s8
    return c


_N = lambda loc, fid_scale, scale=10.: dict(loc=loc, scale=scale, loc_fid=loc, scale_fid=fid_scale)


def _model(evolution, lik_type, survey, sampled_ngbars, seed=41, stoch_fixed=None):
    from montecosmo_amd import model, logdensity
    rng = np.random.default_rng(seed)
    fwd = model.FieldLevelForward(final_shape=(8, 8, 8), cell_length=40., box_center=(60., -40., 1400.), box_rotvec=(0.1, 0.2, -0.1),
                                  evolution=evolution, nbody_n_steps=3, lpt_order=2, init_oversamp=1.5, evol_oversamp=2., ptcl_oversamp=2.,
                                  paint_oversamp=2., a_obs=0.65, curved_sky=True, lin_kpow=_kpow(), nbody_a_start=0.1)
    cfg = dict(fwd.config(), final_shape=(8, 8, 8), cell_length=40., precond="fourier")
    extra = {}
    if survey:
        g = np.indices(fwd.paint_shape).astype(float)
        extra["selec_mesh"] = 0.7 + 0.3 * np.cos(2 * np.pi * g[0] / fwd.paint_shape[0]) * np.sin(2 * np.pi * g[2] / fwd.paint_shape[2]) \
            + 0.1 * rng.uniform(size=fwd.paint_shape)
        extra["mask_mesh"] = rng.uniform(size=(8, 8, 8)) < 0.8
        cfg.update(extra)
    lat = {"sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2, low=0., high=np.inf), "b1": _N(1., 1e-2, 1e2)}
    stoch = {"shash": dict(s_e=_N(1., 1e-2), s_ed=_N(0.3, 1e-2), s_e2=_N(0.03, 1e-3)), "poisson": {},
             "quad_gauss": dict(s_e=_N(1., 1e-2)),
             "fourier_gauss": dict(s_e=_N(1., 1e-2), s_k2e=_N(10., 1.), s_kmu2e=_N(10., 1.))}[lik_type]
    fixed = dict(Omega_m=0.3111, b2=0.2, bs2=-0.15, bn2=20., bnpar=5., b3=0.1, bds2=0.1, bs3=-0.05,
                 ngbars=(np.array([1e-3, 1.4e-3]) if survey else 1e-3))
    if stoch_fixed is not None:      # the known-answer comparisons: only s_e is sampled
        stoch = {"s_e": stoch["s_e"]}
        fixed.update(stoch_fixed)
    lat.update(stoch)
    if sampled_ngbars:
        fixed.pop("ngbars")
        lat["ngbars"] = dict(loc=np.array([1e-3, 1.4e-3]), scale=1e-2, loc_fid=np.array([1e-3, 1.4e-3]), scale_fid=1e-5, low=0., high=np.inf)
        extra["n_rbins"] = 2
    sample = {k + "_": (float(rng.normal(0, 1.0)) if k != "ngbars" else rng.normal(0, 1.0, 2)) for k in lat}
    sample["white_mesh_"] = rng.standard_normal((12, 12, 12))
    make_cosmo = lambda base: _cos(obg.Planck18(Omega_c=base["Omega_m"] - 0.0490), base["sigma8"])
    mk = lambda obs, lt=lik_type: logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="fourier", lik_type=lt, **extra)
    dev_sample = lambda s: {k: (v if (np.ndim(v) == 0 or k == "ngbars_") else v.astype(np.float32)) for k, v in s.items()}
    truth = dev_sample(dict(sample, b1_=sample["b1_"] + 5.0, white_mesh_=rng.standard_normal((12, 12, 12))))
    obs = mk(np.zeros((8, 8, 8))).draw_counts(truth, seed=seed).cpu().numpy().astype(np.float64)
    return dict(fwd=fwd, cfg=cfg, lat=lat, fixed=fixed, sample=sample, dev_sample=dev_sample, make_cosmo=make_cosmo, mk=mk, obs=obs, rng=rng)


@pytest.mark.parametrize("evolution,lik_type,survey,sampled_ngbars", [("lpt", "shash", True, False), ("nbody", "shash", False, True),
                                                                      ("lpt", "poisson", True, True), ("lpt", "fourier_gauss", False, True)])
def test_log_density_and_gradient(gpu, evolution, lik_type, survey, sampled_ngbars):
    """Prior + evolve + likelihood on the HIP path against the float64 restatement, with the gates of tests/test_gpu_model.py unchanged:
    lp within 2e-4 |lp| + 0.05; every sampled scalar against central differences (h = 1e-4) within 1e-2 |fd| + 1e-3; white_mesh_ along a random
    direction within 5e-3 max(|fd|, typical).  The data are drawn from the likelihood itself (draw_counts) at a truth sample."""
    m = _model(evolution, lik_type, survey, sampled_ngbars)
    ld = m["mk"](m["obs"])
    sample, lat = m["sample"], m["lat"]
    lp, grad = ld.logdensity_and_grad(m["dev_sample"](sample))
    los = ld.los_fid if lik_type == "fourier_gauss" else None
    ref = lambda s: L.log_density(m["cfg"], lat, m["fixed"], s, m["obs"], m["make_cosmo"], lik_type, los_fid=los)
    lp_o = ref(sample)
    print(f"\n{evolution} {lik_type}: lp {lp:.6f} oracle {lp_o:.6f}")
    assert np.isfinite(lp_o) and abs(lp - lp_o) < 2e-4 * abs(lp_o) + 0.05, (lp, lp_o)
    assert set(grad) == set(ld.names())
    h = 1e-4
    for k in lat:
        if k == "ngbars":
            for i in range(2):
                e = np.eye(2)[i] * h
                fd = (ref(dict(sample, ngbars_=sample["ngbars_"] + e)) - ref(dict(sample, ngbars_=sample["ngbars_"] - e))) / (2 * h)
                print(f"  ngbars[{i}]: fd {fd:.6f} got {grad['ngbars_'][i]:.6f}")
                assert abs(fd - grad["ngbars_"][i]) < 1e-2 * abs(fd) + 1e-3, (k, i, fd, grad["ngbars_"])
            continue
        fd = (ref(dict(sample, **{k + "_": sample[k + "_"] + h})) - ref(dict(sample, **{k + "_": sample[k + "_"] - h}))) / (2 * h)
        print(f"  {k}: fd {fd:.6f} got {grad[k + '_']:.6f}")
        assert abs(fd - grad[k + "_"]) < 1e-2 * abs(fd) + 1e-3, (k, fd, grad[k + "_"])
    d = m["rng"].standard_normal((12, 12, 12))
    fd = (ref(dict(sample, white_mesh_=sample["white_mesh_"] + h * d)) - ref(dict(sample, white_mesh_=sample["white_mesh_"] - h * d))) / (2 * h)
    gw = grad["white_mesh_"].double().cpu().numpy()
    an = float((gw * d).sum())
    typical = np.linalg.norm(gw) * np.linalg.norm(d) / np.sqrt(d.size)
    print(f"  white_mesh_: fd {fd:.6f} got {an:.6f} typical {typical:.4f}")
    assert abs(fd - an) < 5e-3 * max(abs(fd), typical), ("white_mesh_", fd, an, typical)


def test_unread_stochastic_parameter_gets_the_prior_gradient_only(gpu):
    """A sampled parameter the family does not read (s_ed under 'poisson'): zero likelihood gradient, the prior term alone; and the flat
    adapter of the samplers sees every latent name of the new families."""
    from montecosmo_amd import samplers
    m = _model("lpt", "poisson", False, False)
    lat = dict(m["lat"], s_ed=_N(0., 1e-2))
    from montecosmo_amd import logdensity
    ld = logdensity.FieldLevelLogDensity(m["fwd"], m["obs"], lat, m["fixed"], precond="fourier", lik_type="poisson")
    s = m["dev_sample"](dict(m["sample"], s_ed_=0.7))
    _, grad = ld.logdensity_and_grad(s)
    mu, sd = 0., 10. / 1e-2
    assert grad["s_ed_"] == pytest.approx(-(0.7 - mu) / sd ** 2, rel=1e-12)
    flat = samplers.FlatLogDensity(ld)
    assert abs(flat(flat.pack(s))[0] - ld(s)) < 1e-3 * abs(ld(s)) + 0.05


def _normal_cells(obs, count, selec, s_e, dtype):
    """The Gaussian limit both known answers reduce to, per cell: lp, d/d count, d/d s_e (s_ed = 0)."""
    obs, count = np.asarray(obs, dtype=dtype), np.asarray(count, dtype=dtype)
    b = (np.abs(dtype(s_e)) + dtype(1e-9)) * np.sqrt(dtype(selec))
    z = (obs - count) / b
    return np.stack([dtype(-0.5 * L.LOG2PI) - np.log(b) - dtype(0.5) * z * z, z / b, (z * z - 1) / b * np.sign(dtype(s_e)) * np.sqrt(dtype(selec))])


def _fourier_cells(obs, count, box, los, selec, s_e, dtype):
    """The same three per-cell quantities along the Fourier route, transforms included, in `dtype` (scipy.fft keeps float32).  The map
    count -> cgh2rg(rfftn(count)) is orthogonal, so the cotangent of count is its inverse applied to that of the location."""
    import scipy.fft
    cdt = np.complex128 if dtype == np.float64 else np.complex64
    Y, org = scipy.fft.rfftn(np.asarray(count, dtype=dtype)).astype(cdt), o.cgh2rg(scipy.fft.rfftn(np.asarray(obs, dtype=dtype)).astype(cdt))
    t = L.fourier_terms(Y, org.astype(dtype), box, los, selec, s_e, 0., 0., dtype=dtype, adjoint=False)
    cb = scipy.fft.irfftn(o.rg2cgh(t["loc_bar"].astype(dtype)).astype(cdt), s=np.shape(count))
    return np.stack([t["cells"][0], cb.astype(np.float64), t["cells"][1]])


@pytest.mark.parametrize("lik_type", ["fourier_gauss", "shash"])
def test_known_answer_against_quad_gauss(gpu, lik_type):
    """'fourier_gauss' with s_k2e = s_kmu2e = 0 (cgh2rg o rfftn is orthogonal, so the Gaussian is the same one) and 'shash' with s_e2 = 0
    (skewness 0, tailweight 1) both equal 'quad_gauss' with s_ed = 0, s_e2 = 0: lp, the white_mesh_ gradient and the s_e gradient agree to
    float32 round-off.  Round-off is measured as at kernel level: each route's restatement in float32 against float64 on the device's own mean
    counts (transforms included on the Fourier route), per-cell deviations added in quadrature for the sums, and the two routes' deviations
    added; the gate is 4 x that.  Both routes push their count cotangent through the same adjoint kernels, a fixed linear map, so the
    white_mesh_ gradients (prior term removed) are held to 4 x the relative deviation of the count cotangent."""
    stoch_fixed = dict(s_ed=0., s_e2=0.) if lik_type == "shash" else dict(s_k2e=0., s_kmu2e=0.)
    m = _model("lpt", lik_type, False, False, stoch_fixed=stoch_fixed)
    from montecosmo_amd import logdensity
    fixed_q = dict(m["fixed"], s_ed=0., s_e2=0.)
    ld_new = m["mk"](m["obs"])
    ld_q = logdensity.FieldLevelLogDensity(m["fwd"], m["obs"], m["lat"], fixed_q, precond="fourier")
    s = m["dev_sample"](m["sample"])
    lp_n, g_n = ld_new.logdensity_and_grad(s)
    lp_q, g_q = ld_q.logdensity_and_grad(s)
    cm, selec = ld_new.mean_counts(s)
    cm = cm.cpu().numpy()
    s_e = ld_new.base_params(s)["s_e"]
    route = (lambda dt: _fourier_cells(m["obs"], cm, m["cfg"]["box_size"], ld_new.los_fid, selec, s_e, dt)) if lik_type == "fourier_gauss" \
        else (lambda dt: np.stack([L.shash_cells(m["obs"], cm, selec, s_e, 0., 0., dt)[k].astype(np.float64) for k in ("lp", "count_bar", "s_e")]))
    n64, n32 = route(np.float64), route(np.float32)
    q64, q32 = _normal_cells(m["obs"], cm, selec, s_e, np.float64), _normal_cells(m["obs"], cm, selec, s_e, np.float32).astype(np.float64)
    assert np.allclose(n64[0].sum(), q64[0].sum(), rtol=0, atol=1e-7 * abs(q64[0].sum())) and np.allclose(n64[1], q64[1], rtol=1e-7, atol=0)      # (the 1e-9 of scale1)
    dev = _dev_sum(n32, n64) + _dev_sum(q32, q64)
    print(f"\n{lik_type} vs quad_gauss: lp {lp_n:.6f} / {lp_q:.6f}, float32 deviation {dev[0]:.3e}")
    assert abs(lp_n - lp_q) <= 4 * dev[0], (lp_n, lp_q, dev[0])
    dbase = m["lat"]["s_e"]["scale_fid"]
    lik = lambda g: g["s_e_"] - g_q["s_e_"] + 0.      # the prior term of s_e_ is the same number on both routes
    print(f"  s_e_: {g_n['s_e_']:.6f} / {g_q['s_e_']:.6f}, float32 deviation {dev[2] * dbase:.3e}")
    assert abs(lik(g_n)) <= 4 * dev[2] * dbase
    rel_cb = (np.linalg.norm(n32[1] - n64[1]) + np.linalg.norm(q32[1] - q64[1])) / np.linalg.norm(q64[1])
    w = np.asarray(s["white_mesh_"], dtype=np.float64)
    gn, gq = g_n["white_mesh_"].double().cpu().numpy() + w, g_q["white_mesh_"].double().cpu().numpy() + w
    err = np.linalg.norm(gn - gq) / np.linalg.norm(gq)
    print(f"  white_mesh_: relative difference {err:.3e}, float32 deviation of the count cotangent {rel_cb:.3e}")
    assert err <= 4 * rel_cb
