"""The chained reverse sweep carries u = v_bar + tau' x_bar in v_bar's place instead of writing the force cotangent
F_bar' = beta' u (csrc/composite.hip, step_adjoint_kernel; include/mcpm.h, mcpm_plan_hint_next_adjoint), and the three-component
paint takes beta' as a weight scale (mcpm_paint3_scaled_f32).  Held here against the MATERIALISED sweep built from the public pieces
that keep F_bar' in memory (mcpm_step_adjoint_particles_il_f32 + mcpm_plan_chained_fb + mcpm_paint3_f32): same arithmetic on the
same registers, so everything a caller can see after the sweep is bitwise equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runner(n, K):
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    r = bench.Runner(n, K, torch.device("cuda", 0))
    r.forward(K)
    torch.cuda.synchronize()
    return r


def _sptr(r, j):
    return C.c_void_p(r.sbar.data_ptr() + 8 * j)


def _tau(r, i, K):
    return r.dg / 2 if i == K - 1 else r.dg


def driver_step(r, i, K, first, hint=None, tau=None):
    """One adjoint step through the composite driver, as bench.py issues it; hint = (beta', tau') or None."""
    if hint is not None:
        r.plan.call("mcpm_plan_hint_next_adjoint", float(hint[0]), float(hint[1]))
    tau = _tau(r, i, K) if tau is None else tau
    r.plan.call("mcpm_bullfrog_step_vjp_from_f32", r.p(r.states[i, 0]), r.p(r.states[i, 1]), r.p(r.fmesh[i]), float(r.alphas[i]),
                float(r.betas[i]), float(tau), 2, r.p(r.pos_bar if first else r.xb), r.p(r.vel_bar if first else r.vb), r.p(r.xb), r.p(r.vb),
                _sptr(r, i), _sptr(r, K + i), 0.5 if i == K - 1 else 1.0, _sptr(r, 2 * K))


class Pieces:
    """The adjoint step composed from the public pieces, F_bar in memory (what the slab stepper does on one rank)."""

    def __init__(self, r):
        import torch
        n = r.n
        f32 = dict(dtype=torch.float32, device=r.device)
        self.fb = torch.empty((r.N, 3), **f32)
        self.fm3 = torch.empty((3, n, n, n), **f32)
        self.rho = torch.empty((n, n, n), **f32)

    def step(self, r, i, K, hint=None, tau=None):
        tau = _tau(r, i, K) if tau is None else tau
        b, t = np.float32(r.betas[i]), np.float32(tau)
        fbp = C.c_void_p()
        r.plan.call("mcpm_plan_chained_fb", float(r.betas[i]), float(tau), r.p(r.xb), r.p(r.vb), C.byref(fbp))
        if not fbp.value:       # not chained: F_bar = beta v_bar + (beta tau) x_bar, as the driver's own pass forms it
            r.plan.call("mcpm_axpby_f32", r.p(r.vb), r.p(r.xb), 3 * r.N, float(b), float(np.float32(b * t)), r.p(self.fb))
            fbp = r.p(self.fb)
        r.plan.call("mcpm_paint3_f32", r.p(r.states[i, 0]), r.N, 1, fbp, 2, r.p(self.fm3), 0)
        r.plan.call("mcpm_force_meshes_vjp_f32", r.p(self.fm3), r.p(self.rho))
        if hint is not None:
            r.plan.call("mcpm_plan_hint_next_adjoint", float(hint[0]), float(hint[1]))
        r.plan.call("mcpm_step_adjoint_particles_il_f32", r.p(r.states[i, 0]), r.p(r.states[i, 1]), r.p(r.fmesh[i]), r.p(self.rho),
                    float(r.alphas[i]), float(r.betas[i]), float(tau), 2, r.p(r.xb), r.p(r.vb), _sptr(r, i), _sptr(r, K + i),
                    0.5 if i == K - 1 else 1.0, _sptr(r, 2 * K))


def _start(r):
    r.sbar.zero_()
    r.xb.copy_(r.pos_bar)
    r.vb.copy_(r.vel_bar)


def _result(r):
    import torch
    torch.cuda.synchronize()
    return r.xb.clone(), r.vb.clone(), r.sbar.clone()


def materialised_sweep(r, K, steps, chained=True):
    pc = Pieces(r)
    _start(r)
    for i in range(K - 1, K - 1 - steps, -1):
        hint = (r.betas[i - 1], r.dg) if (chained and i > K - steps) else None
        pc.step(r, i, K, hint=hint)
    return _result(r)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def two_steps(r, K, hint_tau, call_tau):
    """Steps K-1 and K-2 through the driver: the first hinted with (beta_{K-2}, hint_tau) (None: not hinted), the second called with
    tau = call_tau and no hint."""
    r.sbar.zero_()
    driver_step(r, K - 1, K, True, hint=None if hint_tau is None else (r.betas[K - 2], hint_tau))
    driver_step(r, K - 2, K, False, tau=call_tau)
    return _result(r)


@pytest.mark.parametrize("n", [64, 256])
def test_carried_sweep_equals_materialised_sweep_bitwise(gpu, n):
    """bench.py's chain (mcpm_plan_hint_next_adjoint + mcpm_bullfrog_step_vjp_from_f32: u carried, no F_bar array) against the
    materialised chain of the public pieces, K = 4: final x_bar, v_bar and the 2 K + 1 scalar cotangents torch.equal.  64^3 runs the
    plain loads and stores, 256^3 (N = 2^24) the streaming ones.

    (The first, unchained step of both sweeps forms F_bar = beta v_bar + (beta tau) x_bar with the library's axpby: by the driver in
    a capped grid-stride launch, by the pieces through mcpm_axpby_f32 with one element per thread.  The two agree bit for bit only
    because that kernel states its arithmetic, fma(a, x, b y), instead of leaving the contraction to the compiler's unrolling.)"""
    import torch
    K = 4
    r = _runner(n, K)
    r.sbar.zero_()
    r.backward(K)
    xb1, vb1, sb1 = _result(r)
    assert bool(torch.isfinite(xb1).all()) and bool(torch.isfinite(vb1).all()) and float(xb1.abs().max()) > 0 and float(sb1.abs().max()) > 0
    xb2, vb2, sb2 = materialised_sweep(r, K, K)
    assert torch.equal(xb1, xb2)
    assert torch.equal(vb1, vb2)
    assert torch.equal(sb1, sb2)


def test_vel_bar_between_chained_calls_holds_the_carried_sum(gpu):
    """After ONE hinted driver call vel_bar is u = v_bar + tau' pos_bar (one fma): within one float32 ulp of max(|v_bar|, |tau' x_bar|)
    of the float64 restatement on the materialised step's (x_bar, v_bar); pos_bar is the true cotangent, bitwise."""
    import torch
    K = 4
    r = _runner(64, K)
    r.sbar.zero_()
    driver_step(r, K - 1, K, True, hint=(r.betas[K - 2], r.dg))
    xb1, vb1, _ = _result(r)                    # (read only: the chain goes on below)
    for i in range(K - 2, -1, -1):              # the next call consumes the sum; the unhinted last call leaves the true v_bar
        driver_step(r, i, K, False, hint=(r.betas[i - 1], r.dg) if i > 0 else None)
    xb2, vb2, sb2 = _result(r)
    xbm, vbm, _ = materialised_sweep(r, K, 1, chained=False)
    assert torch.equal(xb1, xbm)
    tau = float(np.float32(r.dg))
    a, b = vbm.double(), tau * xbm.double()
    ulp = torch.from_numpy(np.spacing(torch.maximum(a.abs(), b.abs()).float().cpu().numpy())).to(a.device).double()
    err = (vb1.double() - (a + b)).abs()
    print("max err / ulp:", float((err / ulp).max()))
    assert bool((err <= ulp).all())
    assert not torch.equal(vb1, vbm)
    xb3, vb3, sb3 = materialised_sweep(r, K, K)
    assert torch.equal(xb2, xb3) and torch.equal(vb2, vb3) and torch.equal(sb2, sb3)


# Measured on the parent commit (64^3, K = 4, steps K-1 and K-2, the second with tau = 0.75 dg): its own hinted sweep against its own
# unhinted sweep, relative L2.  x_bar: 4.93674355100986e-08 (5.49e-08 at 256^3); v_bar and the scalar cotangents: exactly 0 -- after
# two steps they do not depend on the paint, the only place where the parent's two forms differ.  The one non-zero figure is the bound.
PARENT_CHAIN_REL_L2 = 4.93674355100986e-08


def test_a_broken_chain_is_repaired(gpu):
    """Hint (beta', dg), call, then call with ANOTHER tau and no hint: the pending carry is turned back (vel_bar -= tau' pos_bar) and the
    call proceeds unchained: no error, and x_bar, v_bar and the scalar cotangents agree with the never-hinted sweep of the same two steps.
    Bound: twice what the parent commit shows between its own hinted and unhinted sweep of these two steps (there the force cotangent
    is beta (v + tau x) from the kernel, beta v + (beta tau) x from axpby): relative L2 4.94e-08 on x_bar (and exactly 0 on v_bar and
    the scalars, which the parent's two forms do not touch), so 9.87e-08 is allowed on each of the three.  Measured here with the
    repair: x_bar 4.91e-08, v_bar 3.53e-08 (the rounding of u and of u - tau' x_bar), scalars 8.8e-08 as largest relative difference."""
    import torch
    K = 4
    r = _runner(64, K)
    tau2 = 0.75 * r.dg
    xb0, vb0, sb0 = two_steps(r, K, None, tau2)
    xb1, vb1, sb1 = two_steps(r, K, r.dg, tau2)          # hinted for tau' = dg, continued with tau2: not a continuation
    ex, ev, es = rel_l2(xb1, xb0), rel_l2(vb1, vb0), rel_l2(sb1, sb0)
    print("broken chain against unchained: x_bar", ex, "v_bar", ev, "scalars", es)
    assert bool(torch.isfinite(xb1).all()) and bool(torch.isfinite(vb1).all())
    assert ex <= 2 * PARENT_CHAIN_REL_L2
    assert ev <= 2 * PARENT_CHAIN_REL_L2
    assert es <= 2 * PARENT_CHAIN_REL_L2
    # a particle-step call of the composing API repairs a pending carry in the same way
    r.sbar.zero_()
    driver_step(r, K - 1, K, True, hint=(r.betas[K - 2], r.dg))
    Pieces(r).step(r, K - 2, K, tau=tau2)
    xb2, vb2, _ = _result(r)
    assert rel_l2(xb2, xb0) <= 2 * PARENT_CHAIN_REL_L2 and rel_l2(vb2, vb0) <= 2 * PARENT_CHAIN_REL_L2


def _paint3_case(case):
    """(mesh size, displacements, set-up of the plan, what the paint must have exercised)"""
    rng = np.random.default_rng(41)
    n = 40 if case == "fallback" else 64
    N = n ** 3
    disp = np.clip(rng.standard_normal((N, 3)) * 1.5, -3.9, 3.9).astype(np.float32)
    if case == "buckets":      # a few hundred tame particles far outside their tile's window: the integer bucket kernel deposits them
        idx = rng.choice(N, 300, replace=False)
        disp[idx] = (rng.uniform(6.0, 9.0, (300, 3)) * rng.choice([-1.0, 1.0], (300, 3))).astype(np.float32)
    if case == "wild":         # two particles beyond the tame range, far apart: the global-atomic leftover kernel deposits them
        disp[1234] = (20000.25, 0.5, -0.25)
        disp[N // 2 + 77] = (0.75, -17000.5, 1.25)
    return n, disp


@pytest.mark.parametrize("case", ["fixed", "f64", "fallback", "buckets", "wild"])
@pytest.mark.parametrize("s", [0.37109375 * 1.0009765625, -3.3])
def test_paint3_weight_scale_equals_scaled_weights(gpu, case, s):
    """mcpm_paint3_scaled_f32(w, wscale = s) against mcpm_paint3_scaled_f32(s * w formed in f32 on the device, wscale = 1) and
    against mcpm_paint3_f32(s * w): torch.equal meshes on the fixed-point tiles (s rides in the power-of-two scale), the f64
    tiles (MCPM_PAINT3_VARIANT=2), a mesh that takes the per-component fallback (40^3), and with the epilogue's consumers at
    work: bucketed particles, wild particles."""
    import torch
    from montecosmo_amd import nbody as nb
    n, disp = _paint3_case(case)
    N, shape = n ** 3, (n, n, n)
    rng = np.random.default_rng(43)
    s = float(np.float32(s))
    w3 = (rng.standard_normal((N, 3)) * np.exp(1.5 * rng.standard_normal((N, 1)))).astype(np.float32)      # heavy-tailed
    plan = nb.get_plan(shape)
    d = torch.from_numpy(disp).to(gpu)
    w = torch.from_numpy(w3).to(gpu)
    sw = w * torch.tensor(s, dtype=torch.float32, device=gpu)          # f32 products
    assert sw.dtype == torch.float32
    p = lambda t: C.c_void_p(t.data_ptr())

    def paint(wt, wscale, accumulate=0, out=None):
        out = torch.empty((3,) + shape, dtype=torch.float32, device=gpu) if out is None else out
        if wscale is None:
            plan.call("mcpm_paint3_f32", p(d), N, 1, p(wt), 2, p(out), accumulate)
        else:
            plan.call("mcpm_paint3_scaled_f32", p(d), N, 1, p(wt), wscale, 2, p(out), accumulate)
        torch.cuda.synchronize()
        return out

    try:
        plan.call("mcpm_plan_set_paint3_fixed", 0 if case == "f64" else 1)
        a = paint(w, s)
        if case == "buckets":
            print("bucketed", plan.last_bucketed(), "outliers", plan.last_outliers())
            assert plan.last_bucketed() > 0 and plan.last_outliers() == 0      # (a full bucket would bring in float atomics)
        if case == "wild":
            assert plan.last_outliers() >= 2
        b = paint(sw, 1.0)
        c = paint(sw, None)
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        assert torch.equal(a, b)
        assert torch.equal(b, c)
        if case != "wild":      # (float atomics onto a non-zero mesh are not order-independent)
            assert torch.equal(paint(w, s, 1, a.clone()), paint(sw, 1.0, 1, a.clone()))
    finally:
        plan.call("mcpm_plan_set_paint3_fixed", 1)
        plan.call("mcpm_plan_set_halo", 0)
