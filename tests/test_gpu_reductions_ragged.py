"""The particle-side kernels through the ABI at ragged particle counts: a single lane, a partial wave, one lane over a wave, a partial
block, one over a block, and the counts at which the fixed-order float64 fold of csrc/reduce_dev.h goes from one workgroup to two and three
(R = clamp((nblk + 511) / 512, 1, 128): n = 131072 is the last size with R = 1, 131073 gives R = 2 with a last block of one particle, 262221
gives R = 3 with a shorter last range).  Reference: tests/_bias_f64.py, tests/_lik_f64.py, np.interp, the float64 observation chain.

TOLERANCE RULE (tests/test_gpu_likelihood.py): the restatement runs in float64 and in float32 on the same float32 inputs; the kernel is held
to 4 x the float32 run's deviation from the float64 one, per output (max over its elements; for a sum the sum of the absolute
per-term deviations).  Every measured error is printed as `ERR <case> <value> gate <gate>`.
Every input is a slice [:n] of a tensor 512 elements (rows) longer whose excess holds 1e30 (NaN for cotangents): a lane that read past n
would poison a sum.  Every output is a slice of a longer tensor prefilled with -7.25 whose excess must come back bit-identical.  All reads
and writes stay inside their allocations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _bias_f64 as bf  # noqa: E402
import _lik_f64 as L  # noqa: E402
import _ap_f64 as apo  # noqa: E402
from oracle import pm_oracle as o, bias_oracle as bo  # noqa: E402  (checker only)
from _sentinel import Buffers, gate as _gate, dev_sum as _dev_sum, dev_max as _dev, equal as _equal  # noqa: E402

SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 131072, 131073, 262221]
SUBSET = [65, 1000, 131073, 262221]
NMAX = max(SIZES)
F32 = np.float32
BIAS8 = tuple(float(F32(v)) for v in (1.1, 0.3, -0.2, 0.15, 0.25, -0.1, 2.0, 1.5))      # tests/test_gpu_bias.py, as the float32 the ABI takes
PNG5 = tuple(float(F32(v)) for v in (0.7, -0.4, 0.3, 0.2, -1.2))


@pytest.fixture(scope="module")
def data():
    """Seeded float32 standard-normal reads and cotangents of the largest count; a case of n particles takes the first n."""
    rng = np.random.default_rng(101)
    sn = lambda *s: rng.standard_normal(s).astype(F32)
    return dict(dr=sn(NMAX), s2r=sn(NMAX), s3r=sn(NMAX), lr=sn(NMAX), gr=sn(NMAX, 3), ph=sn(NMAX), lp=sn(NMAX),
                g=(0.4 + 0.5 * rng.uniform(size=NMAX)).astype(F32), wb=sn(NMAX), vb=sn(NMAX, 3), w0=sn(NMAX), pre=sn(3, NMAX),
                F1=sn(NMAX, 3), F2=sn(NMAX, 3), gt=sn(NMAX, 3), xb=sn(NMAX, 3))


@pytest.fixture(scope="module")
def plan(gpu):
    from montecosmo_amd import nbody
    return nbody.get_plan((8, 8, 8))


def _np(t):
    return t.cpu().numpy()


def _c5(v):
    import ctypes as C
    return (C.c_float * len(v))(*[float(x) for x in v])


# ---- Lagrangian bias weights -------------------------------------------------------------------------------------------------------
def _bias_inputs(data, n, per_particle, mesh_major):
    r = [data[k][:n] for k in ("dr", "s2r", "s3r", "lr", "gr")]
    g = data["g"][:n] if per_particle else F32(0.7)
    B = Buffers()
    d = [B.inp(x) for x in r[:4]]
    d.append(B.inp(np.ascontiguousarray(r[4].T).reshape(-1)) if mesh_major else B.inp(r[4]))      # (3, n) flat or (n, 3)
    gp = B.inp(g) if per_particle else None
    return r, g, B, d, gp, (n if mesh_major else 0)


def _bias_forward(plan, B, d, gp, gs, cs, n):
    sig = B.out((1,), np.float64)
    w, dv = B.out((n,)), B.out((n, 3))
    plan.call("mcpm_bias_weights_f32", n, d[0], d[1], d[2], d[3], d[4], cs, gp, gs, _c5(BIAS8), w, dv, sig)
    return w, dv, sig


def _bias_vjp(plan, B, d, gp, gs, cs, n, wb, vb, want_gbar):
    outs = [B.out((n,)) for _ in range(4)] + [B.out((3 * n,) if cs else (n, 3))]
    gbar = B.out((n,)) if want_gbar else None
    scal = B.out((10,), np.float64)
    plan.call("mcpm_bias_weights_vjp_f32", n, d[0], d[1], d[2], d[3], d[4], cs, gp, gs, _c5(BIAS8), wb, vb, *outs, gbar, scal)
    return outs, gbar, scal


def _check_bias_forward(errs, tag, got, r, g):
    w, dv, sig = got
    w64, dv64, s64, t64 = bf.bias_weights(*r, g, BIAS8, terms=True)
    w32, dv32, _, t32 = bf.bias_weights(*r, g, BIAS8, dtype=F32, terms=True)
    _gate(errs, f"{tag}-w", _np(w), w64, _dev(w32, w64))
    _gate(errs, f"{tag}-dvel", _np(dv), dv64, _dev(dv32, dv64))
    _gate(errs, f"{tag}-sigma2", _np(sig), s64, _dev_sum(t32["sigma2"][None], t64["sigma2"][None])[0])


def _check_bias_vjp(errs, tag, got, r, g, wb, vb, cs):
    outs, gbar, scal = got
    n = len(wb)
    r64 = bf.bias_weights_vjp(*r, g, BIAS8, wb, vb, terms=True)
    r32 = bf.bias_weights_vjp(*r, g, BIAS8, wb, vb, dtype=F32, terms=True)
    for i, k in enumerate(("drb", "s2rb", "s3rb", "lrb", "grb")):
        x = _np(outs[i])
        if k == "grb" and cs:
            x = x.reshape(3, n).T
        _gate(errs, f"{tag}-{k}", x, r64[i], _dev(r32[i], r64[i]))
    if gbar is not None:
        _gate(errs, f"{tag}-gbar", _np(gbar), r64[5], _dev(r32[5], r64[5]))
    s = _np(scal)
    dev = _dev_sum(r32[8]["scalars"], r64[8]["scalars"])
    for i, k in enumerate(bo.BIAS_KEYS):
        _gate(errs, f"{tag}-{k}_bar", s[i], r64[6][i], dev[i])
    _gate(errs, f"{tag}-growth_bar_sum", s[8], r64[7], dev[8])
    _gate(errs, f"{tag}-sigma2", s[9], r64[8]["sigma2"].sum(), _dev_sum(r32[8]["sigma2"][None], r64[8]["sigma2"][None])[0])


@pytest.mark.parametrize("mesh_major", [False, True], ids=["gr_particle_major", "gr_mesh_major"])
@pytest.mark.parametrize("per_particle", [False, True], ids=["scalar_growth", "particle_growth"])
@pytest.mark.parametrize("n", SIZES)
def test_bias_weights_and_vjp(plan, data, n, per_particle, mesh_major):
    """mcpm_bias_weights_f32 and mcpm_bias_weights_vjp_f32: every per-particle output and all ten scalars against float64, growth_bar
    present and NULL, two calls bitwise equal, nothing read or written behind n."""
    r, g, B, d, gp, cs = _bias_inputs(data, n, per_particle, mesh_major)
    gs = 0.0 if per_particle else float(g)
    wbn, vbn = data["wb"][:n], data["vb"][:n]
    wb, vb = B.cot(wbn), B.cot(vbn)
    tag = f"bias[n{n}-{'pp' if per_particle else 'sc'}-{'mm' if mesh_major else 'pm'}]"
    errs = []
    fwd = _bias_forward(plan, B, d, gp, gs, cs, n)
    _check_bias_forward(errs, tag + "-fwd", fwd, r, g)
    assert _equal(fwd, _bias_forward(plan, B, d, gp, gs, cs, n))
    vjp = _bias_vjp(plan, B, d, gp, gs, cs, n, wb, vb, True)
    _check_bias_vjp(errs, tag + "-vjp", vjp, r, g, wbn, vbn, cs)
    again = _bias_vjp(plan, B, d, gp, gs, cs, n, wb, vb, True)
    assert _equal(vjp[0] + [vjp[1], vjp[2]], again[0] + [again[1], again[2]])
    nog = _bias_vjp(plan, B, d, gp, gs, cs, n, wb, vb, False)      # growth_bar = NULL: the same numbers
    assert nog[1] is None and _equal(vjp[0] + [vjp[2]], nog[0] + [nog[2]])
    B.check_tails()
    assert not errs, errs


# ---- PNG terms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_particle", [False, True], ids=["scalar_growth", "particle_growth"])
@pytest.mark.parametrize("n", SUBSET)
def test_png_weights_and_vjp(plan, data, n, per_particle):
    """mcpm_png_weights_f32 (adds to the weights) and mcpm_png_weights_vjp_f32 (adds to drb, s2rb, growth_bar; writes phb, lpb; ten scalars)."""
    r = [data[k][:n] for k in ("dr", "s2r", "ph", "lp")]
    g = data["g"][:n] if per_particle else F32(0.7)
    gs = 0.0 if per_particle else float(g)
    w0, pre, wbn = data["w0"][:n], data["pre"][:, :n], data["wb"][:n]
    B = Buffers()
    d = [B.inp(x) for x in r]
    gp = B.inp(g) if per_particle else None
    wb = B.cot(wbn)
    tag = f"png[n{n}-{'pp' if per_particle else 'sc'}]"
    errs = []

    def forward():
        w, mom = B.out((n,), init=w0), B.out((2,), np.float64)
        plan.call("mcpm_png_weights_f32", n, *d, gp, gs, _c5(PNG5), w, mom)
        return [w, mom]

    def vjp(want_gbar=True):
        acc = [B.out((n,), init=pre[0]), B.out((n,), init=pre[1])]
        new = [B.out((n,)), B.out((n,))]
        gbar = B.out((n,), init=pre[2]) if want_gbar else None
        scal = B.out((10,), np.float64)
        plan.call("mcpm_png_weights_vjp_f32", n, *d, gp, gs, _c5(PNG5), wb, acc[0], acc[1], new[0], new[1], gbar, scal)
        return acc + new + [gbar, scal]

    f1 = forward()
    w64, m64, t64 = bf.png_weights(*r, g, PNG5, w0, terms=True)
    w32, _, t32 = bf.png_weights(*r, g, PNG5, w0, dtype=F32, terms=True)
    _gate(errs, f"{tag}-fwd-w", _np(f1[0]), w64, _dev(w32, w64))
    mdev = _dev_sum(t32["moments"], t64["moments"])
    for i, k in enumerate(("sigma2", "phi_delta")):
        _gate(errs, f"{tag}-fwd-{k}", _np(f1[1])[i], m64[i], mdev[i])
    assert _equal(f1, forward())
    v1 = vjp()
    r64 = bf.png_weights_vjp(*r, g, PNG5, wbn, *pre, terms=True)
    r32 = bf.png_weights_vjp(*r, g, PNG5, wbn, *pre, dtype=F32, terms=True)
    for i, k in enumerate(("drb", "s2rb", "phb", "lpb", "gbar")):
        _gate(errs, f"{tag}-vjp-{k}", _np(v1[i]), r64[i], _dev(r32[i], r64[i]))
    s = _np(v1[5])
    dev = _dev_sum(r32[9]["scalars"], r64[9]["scalars"])
    want = list(r64[5]) + [r64[6], r64[7], r64[8]]
    for i, k in enumerate(("bp", "bpd", "bpd2", "bps2", "bn2p", "phi_delta_mean", "sigma2_mean", "growth_sum")):
        _gate(errs, f"{tag}-vjp-{k}_bar", s[i], want[i], dev[i])
    for i, k in enumerate(("sigma2", "phi_delta")):
        _gate(errs, f"{tag}-vjp-{k}", s[8 + i], m64[i], mdev[i])
    assert _equal(v1, vjp())
    nog = vjp(False)
    assert nog[4] is None and _equal(v1[:4] + [v1[5]], nog[:4] + [nog[5]])
    B.check_tails()
    assert not errs, errs


# ---- no reduction: only the tail guard can fail ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_f2", [True, False], ids=["F2", "F2_null"])
@pytest.mark.parametrize("n", SUBSET)
def test_lpt_combine_and_vjp(plan, data, n, with_f2):
    F1n, F2n, gtn, xbn, vbn = data["F1"][:n], (data["F2"][:n] if with_f2 else None), data["gt"][:n], data["xb"][:n], data["vb"][:n]
    B = Buffers()
    F1, gt = B.inp(F1n), B.inp(gtn)
    F2 = B.inp(F2n) if with_f2 else None
    tag = f"lpt_combine[n{n}-{'F2' if with_f2 else 'noF2'}]"
    errs = []

    def forward():
        dp, v = B.out((n, 3)), B.out((n, 3))
        plan.call("mcpm_lpt_combine_f32", F1, F2, gt, n, dp, v)
        return [dp, v]

    def vjp():
        xb, vb, gtb = B.cot(xbn), B.cot(vbn), B.out((n, 3))      # xb, vb are overwritten in place; NaN stays behind their ends
        plan.call("mcpm_lpt_combine_vjp_f32", F1, F2, gt, n, xb, vb, gtb)
        return [xb, vb, gtb]

    f1, v1 = forward(), vjp()
    a64, a32 = bf.lpt_combine(F1n, F2n, gtn), bf.lpt_combine(F1n, F2n, gtn, dtype=F32)
    b64, b32 = bf.lpt_combine_vjp(F1n, F2n, gtn, xbn, vbn), bf.lpt_combine_vjp(F1n, F2n, gtn, xbn, vbn, dtype=F32)
    for k, got, w64, w32 in zip(("dpos", "vel", "F2_bar", "F1_bar", "gt_bar"), f1 + v1, a64 + b64, a32 + b32):
        _gate(errs, f"{tag}-{k}", _np(got), w64, _dev(w32, w64))
    assert _equal(f1 + v1, forward() + vjp())
    B.check_tails()
    assert not errs, errs


@pytest.mark.parametrize("n", SUBSET)
def test_interp(plan, n):
    """mcpm_interp_f32 against np.interp in float64: below and above the table, exactly on the first, the last and an interior node, and
    between two nodes one float32 ulp apart (a slope of 4e6)."""
    import torch
    rng = np.random.default_rng(103)
    ulp = float(np.spacing(F32(1.5)))
    xp = np.sort(np.concatenate([np.linspace(0.5, 2.5, 33)[np.linspace(0.5, 2.5, 33) != 1.5], [1.5 - ulp / 2, 1.5 + ulp / 2]]))
    fp = np.cos(3 * xp) + np.where(xp > 1.5, 0.5, 0.)      # the two close nodes differ by 0.5
    x = rng.uniform(0.3, 2.7, n).astype(F32)
    x[:7] = [0.25, 2.75, 0.5, 2.5, 1.0, 1.5, np.nextafter(F32(0.5), F32(1))]
    x[-1] = 1.5
    scale = F32(1.7)
    B = Buffers()
    xd = B.inp(x)
    tab = torch.from_numpy(np.concatenate([xp, fp])).cuda()
    nt = len(xp)

    def call():
        out = B.out((n,))
        plan.call("mcpm_interp_f32", xd, n, tab, tab[nt:], nt, float(scale), out)
        return out
    got = call()
    r64 = np.interp(x.astype(np.float64), xp, fp)
    errs = []
    _gate(errs, f"interp[n{n}]", _np(got), float(scale) * r64, _dev(scale * r64.astype(F32), float(scale) * r64))
    g = _np(got)
    assert g[0] == scale * F32(fp[0]) and g[1] == scale * F32(fp[-1]) and g[2] == g[0] and g[3] == g[1] and g[4] == scale * F32(np.cos(3.0))
    assert abs(g[-1] / float(scale) - (fp[xp < 1.5][-1] + 0.25 + 0.5 * (np.cos(3 * (1.5 + ulp / 2)) - np.cos(3 * (1.5 - ulp / 2))))) < 1e-6
    assert torch.equal(got, call())
    B.check_tails()
    assert not errs, errs


@pytest.mark.parametrize("n", [1000, 131073])
def test_lik_real_shash(plan, n):
    """mcpm_lik_real_f32, 'shash' with a mesh selection and a mask, on flat arrays of n cells against tests/_lik_f64.real_terms.
    The d s_e2 sum is the one with a one-signed per-cell error on the device: 2.2e-8 of sum |terms| at every size (3.892e-3 at n = 65536,
    9.221e-3 at 131072, 8.521e-3 at 131073, 1.613e-2 at 262221, with one fold workgroup as with two or three), where the per-term deviations
    of the restatement add to 7.97e-4 .. 1.55e-3 in quadrature and to 1.39e-1 in absolute value at n = 131073 (profiles/reductions_ragged_err.txt)."""
    from montecosmo_amd import _lib
    rng = np.random.default_rng(7)
    count = rng.uniform(35., 95., n).astype(F32)
    obs = np.rint(np.abs(count) + 8. * rng.standard_normal(n)).clip(0).astype(F32)
    selec = rng.uniform(50., 80., n).astype(F32)
    mask = rng.uniform(size=n) < 0.8
    assert mask.mean() >= 0.7
    obs[~mask], selec[~mask] = np.nan, 0.      # what an unobserved cell may hold
    st = tuple(float(F32(v)) for v in (0.9, 0.4, -0.08))
    r64 = L.real_terms("shash", obs, count, selec, mask, *st)
    r32 = L.real_terms("shash", obs, count, selec, mask, *st, dtype=F32)
    B = Buffers()
    ob, ct, sel, mk = B.inp(obs), B.inp(count), B.inp(selec), B.inp(mask)

    def call():
        cb, qb, sums = B.out((n,)), B.out((n,)), B.out((5,), np.float64)
        plan.call("mcpm_lik_real_f32", _lib.LIK_SHASH, n, ob, ct, sel, 1.0, mk, *st, cb, qb, sums)
        return [cb, qb, sums]
    got = call()
    errs = []
    dev = _dev_sum(r32["cells"], r64["cells"])
    for i, k in enumerate(("lp", "s_e_bar", "s_ed_bar", "s_e2_bar", "sqsel_bar_sum")):
        _gate(errs, f"lik_real[n{n}]-{k}", _np(got[2])[i], r64["sums"][i], dev[i])
    _gate(errs, f"lik_real[n{n}]-count_bar", _np(got[0]), r64["count_bar"], _dev(r32["count_bar"], r64["count_bar"]))
    _gate(errs, f"lik_real[n{n}]-sqsel_bar", _np(got[1]), r64["sqsel_bar"], _dev(r32["sqsel_bar"], r64["sqsel_bar"]))
    assert not _np(got[0])[~mask].any() and not _np(got[1])[~mask].any()
    assert _equal(got, call())
    B.check_tails()
    assert not errs, errs


# ---- the observation pass: gf_bar, and with AP_PARAM the two alpha cotangents, are grid sums -------------------------------------------
EVOL, PAINT = (16, 16, 16), (24, 20, 16)      # the set-up of tests/test_gpu_bias.py and tests/test_gpu_ap.py
BOX, CENTER, ROTVEC = (640., 640., 640.), (100., -50., 1500.), (0.2, -0.1, 0.3)
AP = {"alpha_iso": 1.03, "alpha_ap": 0.97}


@pytest.mark.parametrize("ap", [False, True], ids=["plain", "ap_param"])
@pytest.mark.parametrize("n", SUBSET)
def test_observe_pos_vjp_sums(gpu, n, ap):
    """mcpm_observe_pos_vjp_f32 / mcpm_observe_pos_ap_vjp_f32 (AP_PARAM: three reduced values) on n absolute positions, flat sky, fixed
    a_obs, against central differences of the float64 chain: the steps and gates of tests/test_gpu_bias.py::test_observe_pos_forward_and_vjp
    and tests/test_gpu_ap.py (eps 1e-4, h 1e-5, 2e-3)."""
    import torch
    from montecosmo_amd import bricks
    rng = np.random.default_rng(21)
    cosmo, cosmo_fid = bricks.Planck18(), bricks.Planck18()
    R = bo.rotvec_matrix(ROTVEC)
    pos = rng.uniform(0., 16., (n, 3)).astype(F32)
    vel = (3.0 * rng.standard_normal((n, 3))).astype(F32)
    dvel = (0.5 * rng.standard_normal((n, 3))).astype(F32)
    ob = rng.standard_normal((n, 3)).astype(F32)
    B = Buffers()
    kw = dict(ap_auto=False, ap=AP, cosmo_fid=cosmo_fid) if ap else {}
    got, ctx = bricks.observe_pos(cosmo, B.inp(pos), B.inp(vel), CENTER, ROTVEC, BOX, EVOL, PAINT, a_obs=0.7, curved_sky=False, dvel=B.inp(dvel),
                                  return_ctx=True, **kw)
    x64, v64, dv64, ob64 = (a.astype(np.float64) for a in (pos, vel, dvel, ob))
    if ap:
        f = lambda x, v, dv, a=AP: apo.observe_pos_ap(cosmo, x, v, CENTER, R, BOX, EVOL, PAINT, 0.7, False, dv, False, a, cosmo_fid)
    else:
        f = lambda x, v, dv: bo.observe_pos(cosmo, x, v, CENTER, R, BOX, EVOL, PAINT, 0.7, False, dv)
    ref = f(x64, v64, dv64)
    err_abs = np.abs(_np(got).astype(np.float64) - ref).max()
    tag = f"observe_pos[n{n}-{'ap_param' if ap else 'plain'}]"
    print(f"ERR {tag}-forward {err_abs:.3e} gate {2e-4:.3e}")
    assert err_abs < 2e-4
    obd = B.cot(ob)
    r1, r2 = bricks.observe_pos_vjp(ctx, obd), bricks.observe_pos_vjp(ctx, obd)
    assert all(torch.equal(a, b) for a, b in zip(r1[:3], r2[:3])) and r1[3:] == r2[3:]      # particle bars and the float64 sums, bitwise
    eps = 1e-4
    for name, bar, idx in (("pos", r1[0], 0), ("vel", r1[1], 1), ("dvel", r1[2], 2)):
        d = rng.standard_normal((n, 3))
        args_p, args_m = [x64, v64, dv64], [x64, v64, dv64]
        args_p[idx], args_m[idx] = args_p[idx] + eps * d, args_m[idx] - eps * d
        fd = ((f(*args_p) - f(*args_m)) * ob64).sum() / (2 * eps)
        an = float((bar.double().cpu().numpy() * d).sum())
        gate = 2e-3 * max(abs(fd), np.linalg.norm(ob64) * np.linalg.norm(d) * 1e-2)
        print(f"ERR {tag}-{name}_bar {abs(fd - an):.3e} gate {gate:.3e}")
        assert abs(fd - an) < gate, (name, fd, an)
    gf = float(o.a2g(cosmo, 0.7) * o.a2f(cosmo, 0.7))
    fd = ((f(x64, v64 * (1 + eps), dv64) - f(x64, v64 * (1 - eps), dv64)) * ob64).sum() / (2 * eps * gf)
    print(f"ERR {tag}-gf_bar {abs(fd - r1[3]):.3e} gate {2e-3 * abs(fd):.3e}")
    assert np.isfinite(r1[3]) and abs(fd - r1[3]) < 2e-3 * abs(fd), ("gf", fd, r1[3])
    if ap:
        h = 1e-5
        for k in ("alpha_iso", "alpha_ap"):
            fd = ((f(x64, v64, dv64, dict(AP, **{k: AP[k] + h})) - f(x64, v64, dv64, dict(AP, **{k: AP[k] - h}))) * ob64).sum() / (2 * h)
            print(f"ERR {tag}-{k}_bar {abs(fd - r1[4][k]):.3e} gate {2e-3 * abs(fd):.3e}")
            assert np.isfinite(r1[4][k]) and abs(fd - r1[4][k]) < 2e-3 * abs(fd), (k, fd, r1[4][k])
    B.check_tails()


# ---- one plan, growing scratch, folds of different K back to back ------------------------------------------------------------------------
def test_scratch_growth_and_mixed_folds_on_one_plan(gpu, data):
    """A plan of its own (its reduction scratch starts small): n = 1000, then 262221 (the scratch is reallocated with a larger K * nblk), then
    1000 again, bitwise equal to the first; then the K = 9 VJP followed directly by the K = 1 forward at n = 131073, both against float64."""
    from montecosmo_amd import nbody
    plan = nbody.Plan((8, 8, 8))
    runs = []
    for n in (1000, 262221, 1000):
        r, g, B, d, gp, cs = _bias_inputs(data, n, True, False)
        wb, vb = B.cot(data["wb"][:n]), B.cot(data["vb"][:n])
        outs, gbar, scal = _bias_vjp(plan, B, d, gp, 0.0, cs, n, wb, vb, True)
        B.check_tails()
        runs.append(outs + [gbar, scal])
    assert _equal(runs[0], runs[2])
    errs = []
    _check_bias_vjp(errs, "growth[n262221]-vjp", (runs[1][:5], runs[1][5], runs[1][6]), [data[k][:262221] for k in ("dr", "s2r", "s3r", "lr", "gr")],
                    data["g"][:262221], data["wb"][:262221], data["vb"][:262221], 0)
    n = 131073
    r, g, B, d, gp, cs = _bias_inputs(data, n, False, False)
    wb, vb = B.cot(data["wb"][:n]), B.cot(data["vb"][:n])
    vjp = _bias_vjp(plan, B, d, gp, float(g), cs, n, wb, vb, True)
    fwd = _bias_forward(plan, B, d, gp, float(g), cs, n)
    _check_bias_vjp(errs, "mixed[n131073]-vjp", vjp, r, g, data["wb"][:n], data["vb"][:n], cs)
    _check_bias_forward(errs, "mixed[n131073]-fwd", fwd, r, g)
    B.check_tails()
    assert not errs, errs
