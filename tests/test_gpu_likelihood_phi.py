"""'two_quad_gauss', the term s_ep phi of scale1 and the temperature of the likelihood on the HIP path (csrc/likelihood.hip:
mcpm_lik_real_phi_f32, mcpm_lik_fourier_temp_f32; model.py: ctx.phi, phi_final, evolve_vjp(phi_bar=); logdensity.py) against the
float64 restatement tests/_lik_phi_f64.py.

Kernel level: the TOLERANCE RULE of tests/test_gpu_likelihood.py, unchanged -- the restatement runs in float64 and in float32 on the same
float32-rounded inputs, the kernel is held to 4 x the float32 run's deviation (a mesh: max |x32 - x64|; a sum: max(|sum d_i|,
sqrt(sum d_i^2)) of the per-cell deviations).  At n = 1 that measurement is one draw of one cell's rounding error, which can be nothing
by chance (the argument tests/test_gpu_likelihood.py makes for the signed sum): on the MI355X the float32 restatement of the single cell
deviated 1.2e-8 in d s_e = 4.893, a fortieth of a float32 unit in the last place, where the kernel, whose per-cell gradients are float32,
was 4.6e-7 (one unit) off.  So the single cell is the first observed cell of the 240-cell inputs and its deviation is measured on those
240 cells: their rms for a sum of one cell, their maximum for a mesh.  The factor 4 and the restatement stay.  Model level: the gates of tests/test_gpu_png_model.py::test_log_density_png -- lp within
2e-4 |lp| + 0.05, a sampled scalar against central differences (h = 1e-4) within 1e-2 |fd| + 1e-3, the field gradient along a random
direction within 5e-3 max(|fd|, typical)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _lik_f64 as L  # noqa: E402
import _lik_phi_f64 as P  # noqa: E402
import _png_f64 as pf  # noqa: E402
from oracle import pm_oracle as o, background as obg  # noqa: E402  (checker only)

FAMILY = {"shash": 0, "poisson": 1, "two_quad_gauss": 2}


def _gate(name, got, want, dev):
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))
    print(f"  {name}: float32 restatement deviates {float(dev):.3e}, kernel errs {err:.3e} (|value| <= {float(np.max(np.abs(want))):.3e})")
    assert err <= 4 * float(dev), (name, err, float(dev))


def _dev_sum(c32, c64):
    d = (c32 - c64).reshape(c64.shape[0], -1)
    return np.maximum(np.abs(d.sum(1)), np.sqrt((d ** 2).sum(1)))


def _inputs(n, mesh_sel, with_phi, seed=7):
    """n cells; about a third of them unobserved, holding what an unobserved cell may hold: a NaN observation, a NaN phi, an exactly
    zero selection.  n = 1: the first observed cell of the 240-cell inputs."""
    if n == 1:
        obs, count, selec, mask, phi = _inputs(240, mesh_sel, with_phi, seed)
        i = slice(int(np.argmax(mask)), int(np.argmax(mask)) + 1)
        return obs[i], count[i], selec[i] if mesh_sel else selec, mask[i], phi[i] if with_phi else None
    rng = np.random.default_rng(seed + n)
    count = rng.uniform(35., 95., n).astype(np.float32)
    obs = np.rint(count + 8. * rng.standard_normal(n)).clip(0).astype(np.float32)
    selec = rng.uniform(50., 80., n).astype(np.float32) if mesh_sel else np.float32(64.5)
    phi = (3e-5 * rng.standard_normal(n)).astype(np.float32) if with_phi else None
    mask = rng.uniform(size=n) < 2 / 3
    obs[~mask] = np.nan
    if mesh_sel:
        selec[~mask] = 0.
    if with_phi:
        phi[~mask] = np.nan
    return obs, count, selec, mask, phi


_RULE = {}


def _rule(dev):
    import torch
    if dev not in _RULE:
        z, lw = P.quad_rule()
        _RULE[dev] = (torch.from_numpy(z).to(dev), torch.from_numpy(lw).to(dev))
    return _RULE[dev]


def _call_phi(family, obs, count, selec, mask, phi, st, s_ep, temp, want_sq=True):
    import torch
    from montecosmo_amd import nbody
    plan = nbody.get_plan((8, 8, 8))      # lends its stream and reduction scratch: n need not be its mesh size
    ob, ct = nbody._f32(obs), nbody._f32(count)
    sel = nbody._f32(selec) if np.ndim(selec) else None
    mk = None if mask is None else torch.from_numpy(mask).to(ob.device)
    ph = None if phi is None else nbody._f32(phi)
    nan = lambda: torch.full_like(ct, float("nan"))
    cb, qb, pb = nan(), (nan() if want_sq else None), (nan() if phi is not None else None)
    sums = torch.full((6,), float("nan"), dtype=torch.float64, device=ob.device)
    z, lw = _rule(ob.device) if family == "two_quad_gauss" else (None, None)
    plan.call("mcpm_lik_real_phi_f32", FAMILY[family], C.c_int64(ct.numel()), ob, ct, sel, 1.0 if sel is not None else float(selec), mk, ph,
              *[float(v) for v in st], float(s_ep), float(temp), z, lw, P.N_QUAD if z is not None else 0, cb, pb, qb, sums)
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(cb), host(pb), host(qb), sums.cpu().numpy()


def _call_old(family, obs, count, selec, mask, st):
    import torch
    from montecosmo_amd import nbody
    plan = nbody.get_plan((8, 8, 8))
    ob, ct = nbody._f32(obs), nbody._f32(count)
    sel = nbody._f32(selec) if np.ndim(selec) else None
    mk = None if mask is None else torch.from_numpy(mask).to(ob.device)
    cb, qb = torch.full_like(ct, float("nan")), torch.full_like(ct, float("nan"))
    sums = torch.full((5,), float("nan"), dtype=torch.float64, device=ob.device)
    plan.call("mcpm_lik_real_f32", FAMILY[family], C.c_int64(ct.numel()), ob, ct, sel, 1.0 if sel is not None else float(selec), mk,
              *[float(v) for v in st], cb, qb, sums)
    return cb.cpu().numpy(), qb.cpu().numpy(), sums.cpu().numpy()


SIZES = [240, 1680, 1]      # below one workgroup of 256; several with a ragged tail; one cell


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", ["shash", "two_quad_gauss"])
def test_kernel_against_restatement(gpu, family, n):
    """mcpm_lik_real_phi_f32 through the ABI, mesh and scalar selection x phi given and NULL x temp 1 and 2.5, always masked: the six sums
    and the three meshes within 4 x the float32 restatement's deviation, bitwise equal across two calls, exact zeros in unobserved cells."""
    for mesh_sel in (True, False):
        for with_phi in (True, False):
            for temp in (1., 2.5):
                obs, count, selec, mask, phi = _inputs(n, mesh_sel, with_phi)
                st = tuple(float(np.float32(v)) for v in (0.9, 0.4, 0.08 if mesh_sel else -0.08))
                s_ep, temp = float(np.float32(4e3)), float(np.float32(temp))
                a64 = (family, obs, count, selec, mask, phi, *st, s_ep, temp)
                r64, r32 = P.real_terms(*a64), P.real_terms(*a64, dtype=np.float32)
                cb, pb, qb, sums = _call_phi(family, obs, count, selec, mask, phi, st, s_ep, temp)
                cb2, pb2, qb2, sums2 = _call_phi(family, obs, count, selec, mask, phi, st, s_ep, temp)
                assert np.array_equal(cb, cb2) and np.array_equal(qb, qb2) and np.array_equal(sums, sums2)      # bitwise
                assert np.isfinite(cb).all() and np.isfinite(qb).all() and np.isfinite(sums).all()
                assert not cb[~mask].any() and not qb[~mask].any()
                print(f"\n{family} n={n} mesh_sel={mesh_sel} phi={with_phi} temp={temp}")
                if n == 1:      # (see the docstring) the deviation of one cell: the rms over the 240 cells this one is taken from
                    a240 = (family, *_inputs(240, mesh_sel, with_phi), *st, s_ep, temp)
                    d64, d32 = P.real_terms(*a240), P.real_terms(*a240, dtype=np.float32)
                    dev = np.sqrt(((d32["cells"] - d64["cells"]) ** 2).mean(1))
                else:
                    d64, d32 = r64, r32
                    dev = _dev_sum(r32["cells"], r64["cells"])
                for i, k in enumerate(("lp", "d s_e", "d s_ed", "d s_e2", "sum sqsel_bar", "d s_ep")):
                    _gate(k, sums[i], r64["sums"][i], dev[i])
                _gate("count_bar", cb, r64["count_bar"], np.abs(d32["count_bar"] - d64["count_bar"]).max())
                _gate("sqsel_bar", qb, r64["sqsel_bar"], np.abs(d32["sqsel_bar"] - d64["sqsel_bar"]).max())
                if with_phi:
                    assert np.array_equal(pb, pb2) and np.isfinite(pb).all() and not pb[~mask].any()
                    _gate("phi_bar", pb, r64["phi_bar"], np.abs(d32["phi_bar"] - d64["phi_bar"]).max())
                else:
                    assert pb is None and sums[5] == 0.
                cb3, _, qb3, sums3 = _call_phi(family, obs, count, selec, mask, phi, st, s_ep, temp, want_sq=False)
                assert qb3 is None and np.array_equal(cb, cb3) and np.array_equal(sums, sums3)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", ["shash", "poisson"])
def test_without_phi_and_temperature_the_old_entry_point_bit_for_bit(gpu, family, n):
    """phi NULL, s_ep = 0, temp = 1: the families of mcpm_lik_real_f32 return its meshes and its five sums bit for bit (a sixth sum of 0)."""
    for mesh_sel in (True, False):
        obs, count, selec, mask, _ = _inputs(n, mesh_sel, False)
        if family == "poisson":
            count[::7] *= -1.
        st = tuple(float(np.float32(v)) for v in (0.9, 0.4, 0.08)) if family == "shash" else (0., 0., 0.)
        cb, _, qb, sums = _call_phi(family, obs, count, selec, mask, None, st, 0., 1.)
        cb0, qb0, sums0 = _call_old(family, obs, count, selec, mask, st)
        assert np.array_equal(cb, cb0) and np.array_equal(qb, qb0) and np.array_equal(sums[:5], sums0) and sums[5] == 0.
        assert np.isfinite(sums0).all()


def test_poisson_with_a_temperature(gpu):
    """Poisson(|count|^(1 / temp)) at temp = 2.5 (negative mean counts among them: the rate is a power of |count|, the gradient carries the
    sign): value (formed in float64 by the kernel) and count_bar under the same rule."""
    obs, count, selec, mask, _ = _inputs(1680, False, False)
    count[::97] *= -1.
    a64 = ("poisson", obs, count, selec, mask, None, 0., 0., 0., 0., 2.5)
    r64, r32 = P.real_terms(*a64), P.real_terms(*a64, dtype=np.float32)
    cb, _, qb, sums = _call_phi("poisson", obs, count, selec, mask, None, (0., 0., 0.), 0., 2.5)
    assert not cb[~mask].any() and not qb.any() and not sums[1:].any()
    print("\npoisson temp=2.5")
    _gate("lp", sums[0], r64["sums"][0], _dev_sum(r32["cells"], r64["cells"])[0])
    _gate("count_bar", cb, r64["count_bar"], np.abs(r32["count_bar"] - r64["count_bar"]).max())


def test_fourier_with_a_temperature(gpu):
    """mcpm_lik_fourier_temp_f32: temp = 1 is mcpm_lik_fourier_f32 bit for bit.  The scale at (selec, temp) is the scale of the selection
    selec * temp, and the entry point rounds sqrt(selec temp) once: with selec = 60, temp = 2.5 (an exact product) the value, the three
    scalar sums and Y_bar are those of mcpm_lik_fourier_f32 at selec = 150 bit for bit -- numbers tests/test_gpu_likelihood.py holds to the
    restatement.  d / d sqrt(selec) = sqrt(temp) d / d sqrt(selec temp), multiplied per term in float32 before the float64 sum: one more
    rounding per term and the rounding of sqrt(temp), so within 2 x 2^-24 x sqrt(temp) x sum |term|, the terms from the restatement."""
    import torch
    from montecosmo_amd import nbody
    shape = (6, 8, 10)
    rng = np.random.default_rng(11)
    box = tuple(float(np.float32(25. * n * f)) for n, f in zip(shape, (1.0, 1.2, 0.9)))
    los = np.array([0.3, -0.5, 0.81])
    los = (los / np.linalg.norm(los)).astype(np.float32).astype(np.float64)
    count = rng.uniform(40., 90., shape)
    obs = count + 8. * rng.standard_normal(shape)
    Y = np.fft.rfftn(count).astype(np.complex64)
    org = o.cgh2rg(np.fft.rfftn(obs)).astype(np.float32)
    st = tuple(float(np.float32(v)) for v in (-1.1, -8., -10.))      # s_e, s_k2e, s_kmu2e
    plan = nbody.get_plan(shape)
    Yd, od = nbody._c64(Y), nbody._f32(org)

    def call(name, selec, *temp):
        Yb = torch.full_like(Yd, complex(float("nan"), float("nan")))
        sums = torch.full((5,), float("nan"), dtype=torch.float64, device=Yd.device)
        plan.call(name, Yd, od, *[float(b) for b in box], *[float(v) for v in los], selec, *st, *temp, Yb, sums)
        return Yb.cpu().numpy().view(np.float32), sums.cpu().numpy()
    Yb0, s0 = call("mcpm_lik_fourier_f32", 60.)
    Yb1, s1 = call("mcpm_lik_fourier_temp_f32", 60., 1.0)
    assert np.array_equal(Yb0, Yb1) and np.array_equal(s0, s1)
    temp = 2.5
    Yb, sums = call("mcpm_lik_fourier_temp_f32", 60., temp)
    Ybw, want = call("mcpm_lik_fourier_f32", 60. * temp)
    assert np.isfinite(sums).all() and np.array_equal(Yb, Ybw) and np.array_equal(sums[:4], want[:4])
    assert not np.array_equal(Yb, Yb0)      # (and the temperature does something)
    terms = L.fourier_terms(Y, org, box, los, 60. * temp, *st, adjoint=False)["cells"][4]
    bound = 2 * 2. ** -24 * np.sqrt(temp) * np.abs(terms).sum()
    print(f"\nfourier_gauss temp=2.5: d sqrt(selec) {sums[4]:.9f}, sqrt(temp) x the untempered sum {np.sqrt(temp) * want[4]:.9f}, bound {bound:.3e}")
    assert abs(sums[4] - np.sqrt(temp) * want[4]) <= bound


# ---- model level -------------------------------------------------------------------------------------------------------------------
def _kpow():
    ks = np.logspace(-3, 1, 128)
    return ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6)


FWD_KW = dict(final_shape=(8, 8, 8), cell_length=40., box_center=(60., -40., 1400.), box_rotvec=(0.1, 0.2, -0.1), evolution="lpt", lpt_order=2,
              a_obs=0.65, curved_sky=True, png_type="fNL")      # the default oversampling: init 12^3, evol / ptcl / paint 14^3
S_EP_FID = 3e3      # phi ~ 2e-5 on this mesh: s_ep phi reaches 0.2 beside s_e = 1
LAT = {"fNL": dict(loc=0., scale=1e3, loc_fid=200., scale_fid=50.),
       "sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2, low=0., high=np.inf),
       "s_ep": dict(loc=0., scale=1e5, loc_fid=S_EP_FID, scale_fid=1e3)}
FIXED = dict(Omega_m=0.3111, b1=1., b2=0.2, bs2=-0.15, bn2=20., bnpar=5., b3=0.1, bds2=0.1, bs3=-0.05, ngbars=1e-3, s_e=1.0, s_ed=0.3,
             s_e2=0.03, fNL_bpd2=-20., fNL_bps2=30., fNL_bn2p=2.0e3)


def make_cosmo(base):
    c = obg.Planck18(Omega_c=base["Omega_m"] - 0.0490)
    c.sigma8 = base["sigma8"]
    c.png_params = {k: base.get(k, 0.) for k in pf.PNG_KEYS}
    return c


def host_case(cfg, lik_type, seed=41):
    """The sample the test evaluates and an observation drawn on the host (float64) from the likelihood itself at another sample: the
    restated mean counts and scales of that truth, obs = count + scale1 eps1 + scale2 (eps^2 - 1) with eps = eps1 ('quad_gauss', and
    'shash', whose moments it matches) or an independent eps2 ('two_quad_gauss')."""
    rng = np.random.default_rng(seed)
    sample = {k + "_": float(rng.normal(0, 1.0)) for k in LAT}
    sample["white_mesh_"] = rng.standard_normal(cfg["init_shape"])
    truth = dict(sample, fNL_=sample["fNL_"] + 1., s_ep_=sample["s_ep_"] - 0.5, white_mesh_=rng.standard_normal(cfg["init_shape"]))
    info = {}
    P.log_density(cfg, LAT, FIXED, truth, np.zeros(cfg["final_shape"]), make_cosmo, "two_quad_gauss", "fNL", info=info)
    sc = P.scales(info["count"], info["selec"], info["phi"], FIXED["s_e"], FIXED["s_ed"], FIXED["s_e2"], info["base"]["s_ep"], 1.)
    e1 = rng.standard_normal(cfg["final_shape"])
    e2 = rng.standard_normal(cfg["final_shape"]) if lik_type == "two_quad_gauss" else e1
    return sample, info["count"] + sc["b"] * e1 + sc["a"] * (e2 ** 2 - 1.), rng


def _cfg(fwd):
    return dict(fwd.config(), final_shape=(8, 8, 8), cell_length=40., precond="fourier")


def _s32(sample):
    return {k: (v if np.ndim(v) == 0 else v.astype(np.float32)) for k, v in sample.items()}


@pytest.mark.parametrize("lik_type,temp", [("quad_gauss", 1.), ("shash", 1.), ("two_quad_gauss", 1.), ("two_quad_gauss", 2.5)])
def test_log_density_with_s_ep(gpu, lik_type, temp):
    """8^3 final mesh, 14^3 evolution mesh (a non-trivial chreshape for phi), png_type 'fNL', 'lpt', s_ep sampled: the log density against
    the float64 composition, d/d s_ep_, d/d fNL_, d/d sigma8_ and the field gradient against its central differences."""
    from montecosmo_amd import model, logdensity
    fwd = model.FieldLevelForward(lin_kpow=_kpow(), **FWD_KW)
    assert tuple(fwd.evol_shape) == (14, 14, 14) and tuple(fwd.init_shape) == (12, 12, 12)
    cfg = _cfg(fwd)
    sample, obs, rng = host_case(cfg, lik_type)
    ld = logdensity.FieldLevelLogDensity(fwd, obs, LAT, FIXED, precond="fourier", lik_type=lik_type)
    lp, grad = ld.logdensity_and_grad(_s32(sample), temp_lik=temp)
    lp2, grad2 = ld.logdensity_and_grad(_s32(sample), temp_lik=temp)
    assert lp == lp2 and all(grad[k + "_"] == grad2[k + "_"] for k in LAT) and bool((grad["white_mesh_"] == grad2["white_mesh_"]).all())
    assert ld.logdensity_and_grad(_s32(sample), need_grad=False, temp_lik=temp)[0] == lp
    info = {}
    ref = lambda s, info=None: P.log_density(cfg, LAT, FIXED, s, obs, make_cosmo, lik_type, "fNL", temp=temp, info=info)
    lp_o = ref(sample, info)
    print(f"\n{lik_type} temp={temp}: lp {lp:.6f} float64 {lp_o:.6f}; max |s_ep phi| {np.abs(info['s_ep_phi']).max():.3f}")
    assert np.abs(info["s_ep_phi"]).max() > 0.05      # the term is there: scale1 moves by several per cent in some cells
    if lik_type == "quad_gauss":      # every cell inside the support: a cell at -inf would show nothing
        print(f"  smallest D = b^2 + 4 a (obs - loc + a): {info['D'].min():.3f}")
        assert info["D"].min() > 0
    assert np.isfinite(lp_o) and abs(lp - lp_o) < 2e-4 * abs(lp_o) + 0.05, (lp, lp_o)
    assert set(grad) == set(ld.names())
    h = 1e-4
    for k in LAT:
        fd = (ref(dict(sample, **{k + "_": sample[k + "_"] + h})) - ref(dict(sample, **{k + "_": sample[k + "_"] - h}))) / (2 * h)
        print(f"  {k}: fd {fd:.6f} got {grad[k + '_']:.6f}")
        assert abs(fd - grad[k + "_"]) < 1e-2 * abs(fd) + 1e-3, (k, fd, grad[k + "_"])
    d = rng.standard_normal(cfg["init_shape"])
    fd = (ref(dict(sample, white_mesh_=sample["white_mesh_"] + h * d)) - ref(dict(sample, white_mesh_=sample["white_mesh_"] - h * d))) / (2 * h)
    gw = grad["white_mesh_"].double().cpu().numpy()
    an = float((gw * d).sum())
    typical = np.linalg.norm(gw) * np.linalg.norm(d) / np.sqrt(d.size)
    print(f"  white_mesh_: fd {fd:.6f} got {an:.6f} typical {typical:.4f}")
    assert abs(fd - an) < 5e-3 * max(abs(fd), typical), ("white_mesh_", fd, an, typical)


def test_evolve_phi_and_its_cotangent(gpu):
    """ctx.phi of evolve is the restated Gaussian potential on the evolution mesh and phi_final brings it to the final mesh (2e-5 relative
    L2, the forward gate of tests/test_gpu_png_model.py); a phi_bar alone (zero gxy_bar) comes back as the restated adjoint pushed through
    the same linear steps: <white_bar, d white> against the float64 phi_final of the perturbed field (3e-3 of the quotient)."""
    import torch
    from montecosmo_amd import model, bricks
    fwd = model.FieldLevelForward(lin_kpow=_kpow(), **FWD_KW)
    cfg = _cfg(fwd)
    rng = np.random.default_rng(31)
    cosmo, cosmo_o = bricks.Planck18(), obg.Planck18()
    cosmo_o.sigma8 = cosmo.sigma8
    white = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * (12 ** 3 / np.prod(cfg["box_size"])) ** .5
    bias = {k: FIXED[k] for k in ("b1", "b2", "bs2", "b3", "bds2", "bs3", "bn2", "bnpar")}
    png = dict(fNL=300., fNL_bpd2=-20., fNL_bps2=30., fNL_bn2p=2.0e3)
    gxy, ctx = fwd.evolve(cosmo, bias, white.astype(np.complex64), png=png, return_ctx=True)
    table = pf.trans_table(cosmo_o)
    phi_o = lambda w: P.phi_final(table, P.evol_mesh(cfg, cosmo_o, w), cfg["box_size"], (8, 8, 8))
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    e_evol = rel(ctx.phi.double().cpu().numpy(), pf.png_fields(table, P.evol_mesh(cfg, cosmo_o, white), cfg["box_size"])[0])
    e_final = rel(fwd.phi_final(ctx.phi).double().cpu().numpy(), phi_o(white))
    print(f"\nphi rel L2: evolution mesh {e_evol:.3e}, final mesh {e_final:.3e}")
    assert e_evol < 2e-5 and e_final < 2e-5
    pb = rng.standard_normal((8, 8, 8))
    g = fwd.evolve_vjp(ctx, torch.zeros_like(gxy), phi_bar=pb.astype(np.float32))      # a zero gxy_bar: every other path carries exact zeros
    wb = g["white_mesh"].cpu().numpy().astype(np.complex128)
    dw = np.fft.rfftn(rng.standard_normal((12, 12, 12))) * (12 ** 3 / np.prod(cfg["box_size"])) ** .5
    want = float((pb * phi_o(dw)).sum())      # phi_final is linear in the white field
    got = float((wb.real * dw.real + wb.imag * dw.imag).sum())
    print(f"phi_bar pulled back to the white field: {got:.6e} float64 {want:.6e}")
    assert abs(got - want) < 3e-3 * abs(want)
    plain = model.FieldLevelForward(lin_kpow=_kpow(), **dict(FWD_KW, png_type=None))
    _, c0 = plain.evolve(cosmo, bias, white.astype(np.complex64), return_ctx=True)
    assert c0.phi is None
    with pytest.raises(ValueError, match="png_type"):
        plain.evolve_vjp(c0, torch.zeros_like(gxy), phi_bar=pb.astype(np.float32))


def test_s_ep_fixed_at_zero_is_the_old_entry_point_bit_for_bit(gpu):
    """temp_lik = 1 and no s_ep (fixed at 0): 'shash' gives the log density and the gradient of the old entry point mcpm_lik_real_f32,
    called here directly on the same mean counts, bit for bit -- the likelihood value and the count cotangent are its own, so the prior
    + likelihood total and every gradient entry are the same floats as a run that passes s_ep = 0 explicitly or through png_type None."""
    import torch
    from montecosmo_amd import model, logdensity, nbody, _lib
    fwd = model.FieldLevelForward(lin_kpow=_kpow(), **FWD_KW)
    sample, obs, _ = host_case(_cfg(fwd), "shash")
    lat = {k: v for k, v in LAT.items() if k != "s_ep"}
    s = _s32({k: v for k, v in sample.items() if k != "s_ep_"})
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, FIXED, precond="fourier", lik_type="shash")
    lp, grad = ld.logdensity_and_grad(s)
    ld0 = logdensity.FieldLevelLogDensity(fwd, obs, lat, dict(FIXED, s_ep=0.), precond="fourier", lik_type="shash")
    lp0, grad0 = ld0.logdensity_and_grad(s, temp_lik=1.)
    assert lp == lp0 and all(grad[k] == grad0[k] for k in grad if k != "white_mesh_") and bool((grad["white_mesh_"] == grad0["white_mesh_"]).all())
    # the likelihood stage against the old entry point
    base = ld.base_params(s)
    f = ld._forward(base, s["white_mesh_"], need_ctx=True, need_phi=True)
    assert f.phi is None
    lpl, cm_bar, stoch_bar, _ = ld._lik_hip(base, f, True)
    cm = f.cm.contiguous()
    cb = torch.empty_like(cm)
    sums = torch.empty(5, dtype=torch.float64, device=cm.device)
    nbody.get_plan((8, 8, 8)).call("mcpm_lik_real_f32", _lib.LIK_SHASH, C.c_int64(cm.numel()), ld.count_obs, cm, None, float(f.selec), None,
                                   float(base["s_e"]), float(base["s_ed"]), float(base["s_e2"]), cb, None, sums)
    v = sums.cpu().numpy()
    assert lpl == float(v[0]) and bool((cm_bar == cb).all())
    assert [stoch_bar[k] for k in ("s_e", "s_ed", "s_e2")] == [float(x) for x in v[1:4]]


def test_two_quad_gauss_constructs_and_evaluates(gpu):
    """Without png_type as well: phi = 0, the term vanishes and a sampled s_ep has the gradient of its prior alone."""
    from montecosmo_amd import model, logdensity
    fwd = model.FieldLevelForward(lin_kpow=_kpow(), **dict(FWD_KW, png_type=None))
    rng = np.random.default_rng(3)
    obs = 64. + 8. * rng.standard_normal((8, 8, 8))
    lat = {"s_ep": {}, "sigma8": LAT["sigma8"]}
    ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, FIXED, precond="fourier", lik_type="two_quad_gauss")
    assert ld.latents["s_ep"]["scale"] == 1e5 and ld.latents["s_ep"]["scale_fid"] == 1e2      # the reference's defaults
    s = {"s_ep_": 0.7, "sigma8_": 0.2, "white_mesh_": rng.standard_normal((12, 12, 12)).astype(np.float32)}
    lp, grad = ld.logdensity_and_grad(s)
    assert np.isfinite(lp) and grad["s_ep_"] == pytest.approx(-0.7 / (1e5 / 1e2) ** 2, rel=1e-12)
    ld_fixed = logdensity.FieldLevelLogDensity(fwd, obs, {"sigma8": LAT["sigma8"]}, FIXED, precond="fourier", lik_type="two_quad_gauss")
    lp_f, grad_f = ld_fixed.logdensity_and_grad({k: v for k, v in s.items() if k != "s_ep_"})
    prior = -0.5 * np.log(2 * np.pi) - np.log(1e3) - 0.5 * (0.7 / 1e3) ** 2
    assert lp == pytest.approx(lp_f + prior, abs=1e-9 * abs(lp)) and grad["sigma8_"] == grad_f["sigma8_"]


def test_sampled_s_ep_with_the_kaiser_model_raises(gpu):
    from montecosmo_amd import model, logdensity
    fwd = model.FieldLevelForward(lin_kpow=_kpow(), **dict(FWD_KW, evolution="kaiser"))
    with pytest.raises(ValueError, match="s_ep"):
        logdensity.FieldLevelLogDensity(fwd, np.zeros((8, 8, 8)), LAT, FIXED, precond="fourier", lik_type="two_quad_gauss")


def test_draw_counts_two_quad_gauss_with_phi(gpu):
    """One draw over the 512 cells, standardised by the restated scales at the device's own mean counts and phi:
    (obs - count) / sqrt(scale1^2 + 2 scale2^2) has mean 0 and variance 1 within 5 standard errors (those of a unit-variance sample whose
    fourth moment is at most that of the largest scale2 / scale1 on the mesh), and it is not the single-field draw of 'quad_gauss'."""
    from montecosmo_amd import model, logdensity
    fwd = model.FieldLevelForward(lin_kpow=_kpow(), **FWD_KW)
    rng = np.random.default_rng(9)
    fixed = dict(FIXED, s_ep=S_EP_FID, s_e2=0.3)
    lat = {"sigma8": LAT["sigma8"]}
    s = {"sigma8_": 0.1, "white_mesh_": rng.standard_normal((12, 12, 12)).astype(np.float32)}
    ld = logdensity.FieldLevelLogDensity(fwd, np.zeros((8, 8, 8)), lat, fixed, precond="fourier", lik_type="two_quad_gauss")
    obs = ld.draw_counts(s, seed=5).double().cpu().numpy()
    f = ld._forward(ld.base_params(s), s["white_mesh_"], need_phi=True)
    cm, phi = f.cm.double().cpu().numpy(), f.phi.double().cpu().numpy()
    sc = P.scales(cm, float(f.selec), phi, fixed["s_e"], fixed["s_ed"], fixed["s_e2"], fixed["s_ep"], 1.)
    assert np.abs(fixed["s_ep"] * phi).max() > 0.05
    var = sc["b"] ** 2 + 2 * sc["a"] ** 2
    x = (obs - cm) / np.sqrt(var)
    n, r = x.size, float((sc["a"] / sc["b"]).max())
    mu4 = (3 + 12 * r ** 2 + 60 * r ** 4) / (1 + 2 * r ** 2) ** 2
    print(f"\ndraw_counts two_quad_gauss: mean {x.mean():.4f}, variance {x.var():.4f}, largest scale2 / scale1 {r:.3f}")
    assert abs(x.mean()) < 5 / np.sqrt(n) and abs(x.var() - 1) < 5 * np.sqrt((mu4 - 1) / n)
    ld_q = logdensity.FieldLevelLogDensity(fwd, np.zeros((8, 8, 8)), lat, fixed, precond="fourier", lik_type="quad_gauss")
    obs_q = ld_q.draw_counts(s, seed=5).double().cpu().numpy()
    e1 = np.random.default_rng(5).standard_normal((8, 8, 8))
    assert np.allclose(obs_q, cm + sc["b"] * e1 + sc["a"] * (e1 ** 2 - 1), rtol=0, atol=1e-4 * np.sqrt(var).max())      # float32 output
    assert np.abs(obs - obs_q).max() > 0.1 * np.sqrt(var).min()
