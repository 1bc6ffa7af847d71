"""The mesh-side model kernels (csrc/bias.hip, csrc/png.hip, csrc/kaiser_post.hip, csrc/eulerian.hip) through the ABI at odd nx, ny and half-spectrum sizes that are no multiple
of a workgroup: mcpm_plan_create takes any nx, ny >= 2 and an even nz, and the kernels' mode decode has a Nyquist branch
`!(n & 1) && i == n / 2` that no even mesh separates from `i == n / 2`.  Every axis has its own box length, so swapped axes cannot pass.
Reference: tests/_bias_f64.py, tests/_kaiser_post_f64.py and tests/_eulerian_f64.py in float64 (k = 2 pi fftfreq(n) n / box, numpy's irfftn:
an odd axis has no Nyquist plane).

Gates.  Forward: max |error| over a mesh / rms of that mesh (a single wrong mode is several percent of the rms on meshes this small) within
4 x the same quantity of the float32 restatement (float32 multipliers with their 1 / M, complex64 products, float64 transforms): the rule of
tests/test_gpu_likelihood.py.  VJPs: <bar, direction> in the real-pair convention against the central difference of the float64 restatement,
eps = 1e-4 and 2e-3 max(|fd|, 1e-2 bound) as in tests/test_gpu_bias.py::test_observe_pos_forward_and_vjp, where `bound` is the Cauchy-Schwarz
bound |cotangent| |J direction| of the difference quotient (there J is an isometry up to the cell ratio and the bound is |ob| |d|; here J
carries 1 / M and the wavevector factors, so |J direction| is taken from the same two float64 evaluations).
Outputs sit in buffers with 512 floats of excess that must come back unchanged; two calls are bitwise equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _bias_f64 as bf  # noqa: E402
import _eulerian_f64 as ef  # noqa: E402
import _kaiser_post_f64 as kpf  # noqa: E402
from _sentinel import Buffers, gate, dev_sum, equal  # noqa: E402

CASES = [((9, 15, 8), (90., 120., 100.)),      # both odd; Mh = 675: two full workgroups and a tail of 163
         ((15, 10, 12), (150., 80., 110.)),      # x odd only
         ((10, 9, 6), (70., 90., 80.)),      # y odd only
         ((12, 10, 8), (100., 120., 90.))]      # even control; Mh = 600
sid = lambda c: "x".join(map(str, c[0]))
F32, EPS = np.float32, 1e-4


def _setup(case, seed):
    from montecosmo_amd import nbody
    shape, box = case
    rng = np.random.default_rng(seed)
    X = np.fft.rfftn(rng.standard_normal(shape)).astype(np.complex64)
    kp = [float(F32(n / b)) for n, b in zip(shape, box)]      # kphys as the float32 the ABI takes ...
    box32 = tuple(n / k for n, k in zip(shape, kp))      # ... and the box the reference sees: the same numbers
    return nbody.get_plan(shape), rng, shape, box32, kp, X, int(np.prod(shape)), X.size


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got, dtype=want.dtype) - want)) / np.sqrt(np.mean(np.abs(want) ** 2)))


def _gate_rel(errs, name, got, w64, w32):
    rms = np.sqrt(np.mean(np.abs(w64) ** 2))
    gate(errs, name, np.abs(np.asarray(got).astype(w64.dtype) - w64) / rms, 0., _rel(w32, w64))


def _pair(a, b):
    return float((a.real * b.real + a.imag * b.imag).sum())


def _table(shape, box, lo, hi, nt=19):
    """A table over about [lo, hi] x the largest |k| of the mesh, each end halfway between two neighbouring |k| values of the mesh and no
    mode closer than 1e-4 (relative) to it: the float32 wavevectors of the kernels then put every mode on the same side of the ends as the
    reference does."""
    km = bf.kabs(shape, box)
    u = np.unique(km)
    mid = lambda f: 0.5 * (u[np.searchsorted(u, f * km.max()) - 1] + u[np.searchsorted(u, f * km.max())])
    ks = np.linspace(mid(lo), mid(hi), nt)
    assert np.abs(km / ks[0] - 1).min() > 1e-4 and np.abs(km / ks[-1] - 1).min() > 1e-4
    assert (km < ks[0]).sum() > 1 and (km > ks[-1]).sum() > 1 and ((km > ks[0]) & (km < ks[-1])).sum() > km.size // 4
    return ks, km


def _fd_check(errs, name, Lfun, x0, d, bar_dot, cot_norm):
    """Central difference of the float64 restatement along d against <bar, d>; Lfun returns (value, outputs)."""
    (lp, yp), (lm, ym) = Lfun(x0 + EPS * d), Lfun(x0 - EPS * d)
    fd = (lp - lm) / (2 * EPS)
    bound = cot_norm * np.linalg.norm((yp - ym).ravel()) / (2 * EPS)
    g = 2e-3 * max(abs(fd), 1e-2 * bound)
    print(f"ERR {name} {abs(fd - bar_dot):.3e} gate {g:.3e}")
    if not abs(fd - bar_dot) < g:
        errs.append(f"{name}: fd {fd:.6e} bar {bar_dot:.6e}")


@pytest.mark.parametrize("case", CASES, ids=sid)
def test_bias_fields_and_vjps(gpu, case):
    """mcpm_bias_fields_f32, mcpm_bias_fields_save_f32, mcpm_bias_fields_vjp_f32 and mcpm_bias_fields_vjp_saved_f32.
    The multipliers of the restatement carry the 1 / M of the device's unnormalised C2R as a float32 number, as the kernels' do: 1 / 540 or
    1 / 960 rounded to float32 is off by up to 6e-8, the same in every cell, which is half of what float32 delivers for delta, the plain C2R
    of the input (measured: 3.9e-7 .. 4.6e-7 of the rms against gates of 7.0e-7 .. 9.5e-7, profiles/reductions_ragged_err.txt)."""
    plan, rng, shape, box, kp, X, M, Mh = _setup(case, 31)
    B = Buffers()
    Xd = B.inp(X)
    errs = []

    def forward(save):
        f7 = B.out((7 * M,))
        h6 = B.out((6 * M,)) if save else None
        if save:
            plan.call("mcpm_bias_fields_save_f32", Xd, *kp, f7, h6)
        else:
            plan.call("mcpm_bias_fields_f32", Xd, *kp, f7)
        return [f7, h6]
    plain, saved = forward(False), forward(True)
    assert equal(plain, forward(False)) and equal(saved, forward(True)) and equal(plain[:1], saved[:1])
    f64, h64 = bf.bias_fields(X, box)
    f32, h32 = bf.bias_fields(X, box, dtype=F32)
    got7, got6 = plain[0].cpu().numpy().reshape((7,) + shape), saved[1].cpu().numpy().reshape((6,) + shape)
    fwd_dev = 0.
    for i, k in enumerate(("delta", "shear2", "shear3", "laplacian", "grad_x", "grad_y", "grad_z")):
        _gate_rel(errs, f"bias_fields[{sid(case)}]-{k}", got7[i], f64[i], f32[i])
        fwd_dev = max(fwd_dev, _rel(f32[i], f64[i]))
    for i, k in enumerate(("delta", "h00", "h11", "h01", "h02", "h12")):
        _gate_rel(errs, f"bias_fields_save[{sid(case)}]-{k}", got6[i], h64[i], h32[i])
    # adjoints
    fb = rng.standard_normal((7,) + shape).astype(F32)
    fbd = B.cot(fb.reshape(-1))

    def vjp(use_saved):
        out = B.out(X.shape, np.complex64)
        if use_saved:
            plan.call("mcpm_bias_fields_vjp_saved_f32", *kp, saved[1], fbd, out)
        else:
            plan.call("mcpm_bias_fields_vjp_f32", Xd, *kp, fbd, out)
        return out
    rec, sav = vjp(False), vjp(True)
    assert equal([rec, sav], [vjp(False), vjp(True)])
    rec, sav = rec.cpu().numpy().astype(np.complex128), sav.cpu().numpy().astype(np.complex128)
    assert np.isfinite(rec.view(np.float64)).all() and np.isfinite(sav.view(np.float64)).all()
    gate(errs, f"bias_fields_vjp[{sid(case)}]-saved_vs_recomputed", np.abs(sav - rec) / np.sqrt(np.mean(np.abs(rec) ** 2)), 0., fwd_dev)
    fb64 = fb.astype(np.float64)
    X64 = X.astype(np.complex128)

    def Lfun(x):
        y = bf.bias_fields(x, box)[0]
        return float((y * fb64).sum()), y
    for j in range(3):
        d = np.fft.rfftn(rng.standard_normal(shape))      # a real field's half-spectrum: a variation numpy's irfftn sees as it is
        for name, bar in (("recomputed", rec), ("saved", sav)):
            _fd_check(errs, f"bias_fields_vjp[{sid(case)}]-{name}-dir{j}", Lfun, X64, d, _pair(bar, d), np.linalg.norm(fb64))
    B.check_tails()
    assert not errs, errs


@pytest.mark.parametrize("case", CASES, ids=sid)
def test_power_mult(gpu, case):
    """mcpm_power_mult_f32 mode by mode, with a table over part of the mesh's |k| range: exact zeros below ks[0] (k = 0 among them) and above
    ks[-1]; every covered mode within 4 x the float32 restatement's relative per-mode deviation."""
    import torch
    plan, rng, shape, box, kp, X, M, Mh = _setup(case, 32)
    ks, km = _table(shape, box, 0.31, 0.79)
    pows = 3.0e2 * (ks / ks[4]) / (1 + (ks / ks[4]) ** 2.6)
    amp = 0.64
    B = Buffers()
    Xd = B.inp(X)
    tab = torch.from_numpy(np.concatenate([ks, pows])).cuda()

    def call():
        out = B.out(X.shape, np.complex64)
        plan.call("mcpm_power_mult_f32", Xd, *kp, amp, tab, tab[len(ks):], len(ks), out)
        return out
    got_t = call()
    assert torch.equal(got_t, call())
    got = got_t.cpu().numpy().astype(np.complex128)
    w64, w32 = bf.power_mult(X, box, ks, pows, amp), bf.power_mult(X, box, ks, pows, amp, dtype=F32)
    outside = (km < ks[0]) | (km > ks[-1])
    assert outside[0, 0, 0] and not w64[outside].any() and (np.abs(w64[~outside]) > 0).all()
    assert not got[outside].any(), "modes outside the table must be exactly zero"
    errs = []
    rel = lambda a: np.abs(a[~outside] - w64[~outside]) / np.abs(w64[~outside])
    gate(errs, f"power_mult[{sid(case)}]-per_mode", rel(got), 0., rel(w32).max())
    B.check_tails()
    assert not errs, errs


@pytest.mark.parametrize("case", CASES, ids=sid)
def test_png_phi_add_and_vjp(gpu, case):
    """mcpm_png_phi_f32, mcpm_png_add_f32 and mcpm_png_add_vjp_f32 with a transfer table over part of the |k| range (t = 0 outside: those
    modes, k = 0 among them, drop out of phi and of the output)."""
    import torch
    plan, rng, shape, box, kp, X, M, Mh = _setup(case, 33)
    ks, km = _table(shape, box, 0.17, 0.83)
    trans = 0.5 + (ks / ks[-1]) ** 2
    table, fNL = (ks, trans), float(F32(0.3))
    nt = len(ks)
    B = Buffers()
    Xd = B.inp(X)
    tab = torch.from_numpy(np.concatenate([ks, trans])).cuda()
    errs = []

    def phi_call():
        phi, lap = B.out((M,)), B.out((M,))
        plan.call("mcpm_png_phi_f32", Xd, *kp, tab, tab[nt:], nt, phi, lap)
        return [phi, lap]

    def add_call():
        phi, out, mean = B.out((M,)), B.out(X.shape, np.complex64), B.out((1,), np.float64)
        plan.call("mcpm_png_add_f32", Xd, *kp, tab, tab[nt:], nt, fNL, 0, phi, out, mean)
        return [phi, out, mean]
    p1, a1 = phi_call(), add_call()
    assert equal(p1 + a1, phi_call() + add_call()) and torch.equal(p1[0], a1[0])
    p64, p32 = bf.png_phi(table, X, box), bf.png_phi(table, X, box, dtype=F32)
    for i, k in enumerate(("phi", "lap_phi")):
        _gate_rel(errs, f"png_phi[{sid(case)}]-{k}", p1[i].cpu().numpy().reshape(shape), p64[i], p32[i])
    (o64, m64), (o32, m32) = bf.add_png(table, fNL, X, box), bf.add_png(table, fNL, X, box, dtype=F32)
    got = a1[1].cpu().numpy().astype(np.complex128)
    outside = (km < ks[0]) | (km > ks[-1])
    assert not got[outside].any() and not o64[outside].any()
    _gate_rel(errs, f"png_add[{sid(case)}]-out", got, o64, o32)
    sq = lambda p: (p.astype(np.float64) ** 2 / M).reshape(1, -1)
    gate(errs, f"png_add[{sid(case)}]-mean", a1[2].cpu().numpy()[0], m64, dev_sum(sq(p32[0].astype(F32)), sq(p64[0]))[0])
    # adjoint: a generic (non-Hermitian) cotangent of the output
    ob = (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)).astype(np.complex64)
    obd = B.cot(ob)

    def vjp():
        lin_bar, scal = B.out(X.shape, np.complex64), B.out((1 + nt,), np.float64)
        plan.call("mcpm_png_add_vjp_f32", Xd, a1[1], a1[0], a1[2], *kp, tab, tab[nt:], nt, fNL, obd, None, None, lin_bar, scal, scal[1:])
        return [lin_bar, scal]
    v1 = vjp()
    assert equal(v1, vjp())
    lb, scal = v1[0].cpu().numpy().astype(np.complex128), v1[1].cpu().numpy()
    assert np.isfinite(lb.view(np.float64)).all() and np.isfinite(scal).all()
    ob64, X64 = ob.astype(np.complex128), X.astype(np.complex128)
    cn = np.linalg.norm(ob64)

    def Lx(x, f=fNL, tr=trans):
        y = bf.add_png((ks, tr), f, x, box)[0]
        return _pair(ob64, y), y
    for j in range(3):
        d = np.fft.rfftn(rng.standard_normal(shape))
        _fd_check(errs, f"png_add_vjp[{sid(case)}]-lin_mesh-dir{j}", Lx, X64, d, _pair(lb, d), cn)
    _fd_check(errs, f"png_add_vjp[{sid(case)}]-fNL", lambda f: Lx(X64, f=f), fNL, 1.0, float(scal[0]), cn)
    dirn = trans * rng.standard_normal(nt)
    _fd_check(errs, f"png_add_vjp[{sid(case)}]-table", lambda tr: Lx(X64, tr=tr), trans, dirn, float((scal[1:] * dirn).sum()), cn)
    B.check_tails()
    assert not errs, errs


def _kaiser_post32(d, noise, shape, box, ks, pows, amp, los, g, f, b1E, var_noise, temp, scale_field, cell_power):
    """The float32 restatement of kaiser_post_kernel: float32 wavevector components, their norm and every per-mode factor in float64, the
    factors rounded to float32 and applied to the complex64 fields in float32.  -> white (chains first), means, stds."""
    k = [c.astype(np.float64) for c in bf.kvec(shape, box, F32)]
    kn = np.sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2])
    mu = kpf.o.safe_div(k[0] * los[0] + k[1] * los[1] + k[2] * los[2], kn)
    P = amp * np.interp(kn, ks, pows, left=0., right=0.)
    p, boost = P * cell_power, g * (b1E + f * mu * mu)
    s2 = p / (1. + boost * boost / var_noise * p)
    sd, mfac = np.sqrt(s2), s2 * boost / var_noise
    wfac = kpf.o.safe_div(scale_field, np.sqrt(P))
    cm, cn = (wfac * mfac).astype(F32), (wfac * np.sqrt(temp) * sd).astype(F32)
    return cm * d + cn * noise, mfac.astype(F32) * d, sd.astype(F32)


@pytest.mark.parametrize("case", CASES, ids=sid)
def test_kaiser_post(gpu, case):
    """mcpm_kaiser_post_c64 with two chains, a line of sight along no axis and a power table over part of the mesh's |k| range: white, means
    and stds exactly zero outside the table (k = 0 among the modes below it), within 4 x the float32 restatement elsewhere."""
    import torch
    from oracle import background as obg
    plan, rng, shape, box, kp, X, M, Mh = _setup(case, 34)
    ks, km = _table(shape, box, 0.31, 0.79)
    pows = 3.0e2 * (ks / ks[4]) / (1 + (ks / ks[4]) ** 2.6)
    cosmo, a, sigma8, b1E, var_noise, temp, sf, nc = obg.Planck18(), 0.7, 0.8, 1.6, 0.35, 0.5, 7 / 8, 2
    los = np.array([0.48, -0.6, 0.64])
    g, f, cell_power = float(kpf.o.a2g(cosmo, a)), float(kpf.o.a2f(cosmo, a)), float(np.prod(kp))
    noise = (rng.standard_normal((nc,) + X.shape) + 1j * rng.standard_normal((nc,) + X.shape)).astype(np.complex64)
    B = Buffers()
    Xd, Nd = B.inp(X), B.inp(noise)
    tab = torch.from_numpy(np.concatenate([ks, pows])).cuda()

    def call():
        white, means, stds = B.out(noise.shape, np.complex64), B.out(X.shape, np.complex64), B.out(X.shape)
        plan.call("mcpm_kaiser_post_c64", Xd, Nd, nc, *kp, sigma8 ** 2, tab, tab[len(ks):], len(ks), *[float(l) for l in los], g, f, b1E,
                  var_noise, temp, sf, cell_power, white, means, stds)
        return [white, means, stds]
    got_t = call()
    assert equal(got_t, call())
    white, means, stds = (t.cpu().numpy() for t in got_t)
    X64 = X.astype(np.complex128)
    m64, s64 = kpf.kaiser_posterior(X64, cosmo, a, np.array(box), var_noise, b1E, los, sigma8, (ks, pows))
    w64 = np.stack([sf * kpf.lin2white(sigma8, temp ** .5 * s64 * noise[b].astype(np.complex128) + m64, shape, np.array(box), (ks, pows))
                    for b in range(nc)])
    w32, m32, s32 = _kaiser_post32(X, noise, shape, box, ks, pows, sigma8 ** 2, los, g, f, b1E, var_noise, temp, sf, cell_power)
    outside = (km < ks[0]) | (km > ks[-1])
    assert outside[0, 0, 0] and not s64[outside].any() and (s64[~outside] > 0).all()
    assert not white[:, outside].any() and not means[outside].any() and not stds[outside].any(), "modes outside the table must be exactly zero"
    errs = []
    _gate_rel(errs, f"kaiser_post[{sid(case)}]-white", white, w64, w32)
    _gate_rel(errs, f"kaiser_post[{sid(case)}]-means", means, m64, m32)
    _gate_rel(errs, f"kaiser_post[{sid(case)}]-stds", stds, s64, s32)
    B.check_tails()
    assert not errs, errs


@pytest.mark.parametrize("case", CASES, ids=sid)
def test_eulerian_bias_and_vjp(gpu, case):
    """mcpm_eulerian_bias_f32 and mcpm_eulerian_bias_vjp_f32, without and with phi_k."""
    import ctypes as C
    plan, rng, shape, box, kp, X, M, Mh = _setup(case, 35)
    Pk = np.fft.rfftn(rng.standard_normal(shape)).astype(np.complex64)
    coef = [float(F32(c)) for c in (1.7, 0.4, -0.3, 0.2, 0.5, 0.35)]
    coef_c = (C.c_float * 6)(*coef)
    wb = rng.standard_normal(shape).astype(F32)
    wb64, X64, P64 = wb.astype(np.float64), X.astype(np.complex128), Pk.astype(np.complex128)
    cn = np.linalg.norm(wb64)
    B = Buffers()
    Xd, Pd, wbd = B.inp(X), B.inp(Pk), B.cot(wb.reshape(-1))
    errs = []
    for phi in (False, True):
        tag = f"eulerian[{sid(case)}]-{'phi' if phi else 'nophi'}"
        P, P_64 = (Pk, P64) if phi else (None, None)

        def forward():
            w, saved, mom = B.out((M,)), B.out(((8 if phi else 7) * M,)), B.out((2,), np.float64)
            plan.call("mcpm_eulerian_bias_f32", Xd, Pd if phi else None, *kp, coef_c, w, saved, mom)
            return [w, saved, mom]

        def vjp(fw):
            mb, pb, cb = B.out(X.shape, np.complex64), B.out(X.shape, np.complex64) if phi else None, B.out((6,), np.float64)
            plan.call("mcpm_eulerian_bias_vjp_f32", fw[1], fw[2], int(phi), *kp, coef_c, wbd, mb, pb, cb)
            return [mb, pb, cb]
        fw = forward()
        assert equal(fw, forward())
        (w64, mom64), (w32, _) = ef.eulerian_bias(X, P, box, coef), ef.eulerian_bias(X, P, box, coef, dtype=F32)
        _gate_rel(errs, f"{tag}-w", fw[0].cpu().numpy().reshape(shape), w64, w32)
        (f64, p64), (f32, p32) = ef.fields(X, P, box), ef.fields(X, P, box, dtype=F32)
        row = lambda a, b: (a.astype(np.float64) * b.astype(np.float64) / M).reshape(1, -1)
        mom = fw[2].cpu().numpy()
        gate(errs, f"{tag}-d2", mom[0], mom64[0], dev_sum(row(f32[0], f32[0]), row(f64[0], f64[0]))[0])
        if phi:
            gate(errs, f"{tag}-phid", mom[1], mom64[1], dev_sum(row(p32, f32[0]), row(p64, f64[0]))[0])
        else:
            assert mom[1] == 0.
        bar = vjp(fw)
        assert equal(bar, vjp(fw))
        mb, cb = bar[0].cpu().numpy().astype(np.complex128), bar[2].cpu().numpy()
        assert np.isfinite(mb.view(np.float64)).all() and np.isfinite(cb).all() and mb[0, 0, 0] == 0
        if not phi:
            assert cb[4] == 0. and cb[5] == 0.

        def L(x=X64, p=P_64, c=coef):
            y = ef.eulerian_bias(x, p, box, c)[0]
            return float((y * wb64).sum()), y
        for j in range(2):
            d = np.fft.rfftn(rng.standard_normal(shape))
            _fd_check(errs, f"{tag}-matter_k-dir{j}", lambda x: L(x=x), X64, d, _pair(mb, d), cn)
            if phi:
                pb = bar[1].cpu().numpy().astype(np.complex128)
                assert np.isfinite(pb.view(np.float64)).all()
                _fd_check(errs, f"{tag}-phi_k-dir{j}", lambda p: L(p=p), P64, d, _pair(pb, d), cn)
        dirn = rng.standard_normal(6) * ([1, 1, 1, 1, 1, 1] if phi else [1, 1, 1, 1, 0, 0])
        _fd_check(errs, f"{tag}-coef", lambda c: L(c=c), np.array(coef), dirn, float((cb * dirn).sum()), cn)
    B.check_tails()
    assert not errs, errs
