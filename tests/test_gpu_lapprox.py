"""GPU checks of the MAP and Laplace passes (csrc/lapprox.hip) against the numpy float64 restatement tests/_lapprox_f64.py, which
tests/test_lapprox_host.py pins: the four entry points through the ABI at ragged sizes, aligned and as views offset by one element,
then `samplers.optimize` and `lapprox.cov_x_from_pot_x_y` through backend='hip' on quadratics with known answers and on the model."""
import math

import numpy as np
import pytest

import _lapprox_f64 as ref

pytestmark = pytest.mark.gpu

F32 = np.float32


def _plan():
    from montecosmo_amd import nbody
    return nbody.get_plan((8, 8, 8))


def _dev(x, offset=0):
    """A device copy of the numpy vector x whose data pointer is `offset` elements past an allocation's (16-byte aligned) start."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    buf = torch.empty(x.size + offset, dtype=t.dtype, device="cuda")
    buf[offset:].copy_(t)
    out = buf[offset:]
    assert out.data_ptr() % 16 == (offset * t.element_size()) % 16 and out.is_contiguous()
    return out


def _within_one_ulp(got, want):
    """Both float32: |got - want| at most one unit in the last place of the larger."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))))


# ---- mcpm_adam_step_f32 -------------------------------------------------------------------------------------------------------------
def _adam_chain(plan, d, offset, seed):
    """Epochs 0, 1, 50 chained on the device.  Returns, per epoch, (state in, g, state out) as numpy float32."""
    rng = np.random.default_rng(seed)
    q, m, v = (_dev(a, offset) for a in (rng.standard_normal(d).astype(F32), np.zeros(d, F32), np.zeros(d, F32)))
    out = []
    for i in (0, 1, 50):
        g_h = (rng.standard_normal(d) * 10.0 ** rng.uniform(-3, 1, d)).astype(F32)
        g = _dev(g_h, offset)
        before = [t.cpu().numpy().copy() for t in (q, m, v)]
        lr, c1, c2 = 0.1 / math.sqrt(1.0 + i), 1.0 / (1.0 - 0.9 ** (i + 1)), 1.0 / (1.0 - 0.999 ** (i + 1))
        plan.call("mcpm_adam_step_f32", q, m, v, g, d, lr, 0.9, 0.999, 1e-8, c1, c2)
        assert np.array_equal(g.cpu().numpy(), g_h)      # the gradient is read only
        out.append((i, before, g_h, [t.cpu().numpy().copy() for t in (q, m, v)]))
    return out


@pytest.mark.parametrize("d", [2, 3, 5, 255, 1027, 2 ** 21 + 5])      # the last passes one grid stride (2048 workgroups x 256 lanes x 4)
def test_adam_step(gpu, d):
    """q, m and v within one float32 ulp of the float64 restatement rounded once (the kernel forms each product and sum on its own, as numpy
    does; the bound leaves room for the last bit of the division and the root), bitwise the same call after call, and the scalar path of
    a view offset by one element agrees bitwise with the 16-byte path."""
    plan = _plan()
    runs = [_adam_chain(plan, d, 0, seed=d), _adam_chain(plan, d, 0, seed=d), _adam_chain(plan, d, 1, seed=d)]
    for i, before, g, after in runs[0]:
        want = ref.adam_step(*before, g, i)
        for name, got, w in zip("qmv", after, want):
            assert _within_one_ulp(got, w.astype(F32)), (name, i, d)
        if i == 0:      # from m = v = 0 every coordinate moves by lr0 g / (|g| + eps)
            step = after[0].astype(np.float64) - before[0].astype(np.float64)
            assert np.allclose(step, 0.1 * g.astype(np.float64) / (np.abs(g.astype(np.float64)) + 1e-8), rtol=0, atol=3e-7)      # half a float32 ulp of |q'| < 8
    for other in runs[1:]:
        for (_, _, _, a), (_, _, _, b) in zip(runs[0], other):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    from montecosmo_amd import _lib
    with pytest.raises(_lib.McpmError):
        plan.call("mcpm_adam_step_f32", None, None, None, None, d, 0.1, 0.9, 0.999, 1e-8, 1., 1.)


# ---- mcpm_probe_shift_f32 / mcpm_hutchinson_accum_f64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("d", [2, 63, 64, 1027, 2 ** 17 + 3])
def test_probe_shift_and_hutchinson_accum(gpu, d, offset):
    import torch
    plan = _plan()
    rng = np.random.default_rng(d + offset)
    seed, eps = 42, 0.5
    q_h = (rng.integers(-256, 257, d) / 256.0).astype(F32)      # a 2^-8 grid in [-1, 1]: q +- 0.5 is exact in float32
    q = _dev(q_h, offset)
    for start, stop in ((0, d), (d // 3, d - d // 4)):
        for probe in (0, 5):
            r = ref.rademacher(seed, probe, d, start, stop)
            want_p, want_m = q_h.astype(np.float64) + eps * r, q_h.astype(np.float64) - eps * r
            assert np.array_equal(want_p.astype(F32).astype(np.float64), want_p) and np.array_equal(want_m.astype(F32).astype(np.float64), want_m)
            qp, qm = _dev(np.full(d, 9, F32), offset), _dev(np.full(d, 9, F32), offset)
            plan.call("mcpm_probe_shift_f32", q, d, start, stop, seed, probe, eps, qp, qm)
            qp_h, qm_h = qp.cpu().numpy().astype(np.float64), qm.cpu().numpy().astype(np.float64)
            assert np.array_equal(qp_h - q_h, eps * r) and np.array_equal(q_h - qm_h, eps * r)      # the numpy hash, bit for bit
            assert np.array_equal(q.cpu().numpy(), q_h)
            # either output may be NULL
            only = _dev(np.full(d, 9, F32), offset)
            plan.call("mcpm_probe_shift_f32", q, d, start, stop, seed, probe, eps, None, only)
            assert torch.equal(only, qm)
            plan.call("mcpm_probe_shift_f32", q, d, start, stop, seed, probe, eps, only, None)
            assert torch.equal(only, qp)
        # the accumulation: one probe bitwise, then 64 probes
        gp_h, gm_h = rng.standard_normal(d).astype(F32), rng.standard_normal(d).astype(F32)
        gp, gm = _dev(gp_h, offset), _dev(gm_h, offset)
        diag_h = rng.standard_normal(d)
        diag = _dev(diag_h, offset)
        coef = -1.0 / (2.0 * 0.03 * 64)
        want = diag_h.copy()
        for probe in range(64):
            plan.call("mcpm_hutchinson_accum_f64", gp, gm, d, start, stop, seed, probe, coef, diag)
            want = ref.hutchinson_accumulate(want, gp_h, gm_h, ref.rademacher(seed, probe, d, start, stop), coef)
            if probe == 0:
                assert np.array_equal(diag.cpu().numpy(), want)
        got = diag.cpu().numpy()
        assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want))
        assert np.array_equal(got[:start], diag_h[:start]) and np.array_equal(got[stop:], diag_h[stop:])      # untouched outside start:stop
    from montecosmo_amd import _lib
    with pytest.raises(_lib.McpmError):      # stop past the end
        plan.call("mcpm_probe_shift_f32", q, d, 1, d + 1, seed, 0, eps, _dev(q_h, offset), None)


def test_hutchinson_accum_on_a_diag_that_is_8_byte_aligned_only(gpu):
    """diag one float64 past a 16-byte boundary with 16-byte aligned gradients: the scalar path, same bits."""
    plan = _plan()
    d, rng = 1027, np.random.default_rng(9)
    gp_h, gm_h, diag_h = rng.standard_normal(d).astype(F32), rng.standard_normal(d).astype(F32), rng.standard_normal(d)
    outs = []
    for off in (0, 1):
        diag = _dev(diag_h, off)
        plan.call("mcpm_hutchinson_accum_f64", _dev(gp_h), _dev(gm_h), d, 3, d - 2, 7, 2, -0.25, diag)
        outs.append(diag.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], ref.hutchinson_accumulate(diag_h, gp_h, gm_h, ref.rademacher(7, 2, d, 3, d - 2), -0.25))


# ---- mcpm_schur_f64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 2 ** 17 + 3])
@pytest.mark.parametrize("m", [1, 2, 5, 16])
def test_schur(gpu, m, n):
    """out = B (D + eps_diag)^-1 B^T against the restatement with extended-precision sums.  The bound 1e-13 sqrt(n) is relative to the sum
    of the absolute terms of an entry, sum_k |B_ik B_jk| / (D_k + eps_diag): that is the entry itself on the diagonal, and off it the
    scale against which the rounding of a sum taken in another order is measured (an off-diagonal entry can cancel to nothing)."""
    import torch
    plan = _plan()
    rng = np.random.default_rng(100 * m + n % 97)
    ldb = n + 3
    B_h = rng.standard_normal((m, ldb)).astype(F32)
    D_h = rng.uniform(0.5, 2.0, n)
    eps_diag = 1e-9
    B, D = torch.from_numpy(B_h).cuda(), torch.from_numpy(D_h).cuda()
    outs = []
    for _ in range(2):
        out = torch.full((m * m,), math.nan, dtype=torch.float64, device="cuda")
        plan.call("mcpm_schur_f64", B, m, n, ldb, D, eps_diag, out)
        outs.append(out.cpu().numpy().reshape(m, m))
    got = outs[0]
    want = ref.schur_sum(B_h[:, :n], D_h, eps_diag)
    scale = ref.schur_sum(np.abs(B_h[:, :n]), D_h, eps_diag)
    err = np.abs(got - want) / scale
    print(f"m = {m}, n = {n}: max relative error {err.max():.2e}, bound {1e-13 * math.sqrt(n):.2e}")
    assert np.all(np.isfinite(got)) and err.max() < 1e-13 * math.sqrt(n)
    assert np.array_equal(got, got.T)                 # exactly symmetric
    assert np.array_equal(outs[0], outs[1])           # bitwise repeatable


def test_schur_refuses_m_above_16(gpu):
    import torch
    from montecosmo_amd import _lib
    plan = _plan()
    B, D = torch.zeros((17, 8), dtype=torch.float32, device="cuda"), torch.ones(8, dtype=torch.float64, device="cuda")
    out = torch.zeros(17 * 17, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.McpmError, match="m <= 16"):
        plan.call("mcpm_schur_f64", B, 17, 8, 8, D, 0.0, out)
    with pytest.raises(_lib.McpmError):
        plan.call("mcpm_schur_f64", B, 0, 8, 8, D, 0.0, out)


# ---- optimize(backend='hip') --------------------------------------------------------------------------------------------------------
def _diag_quadratic_dev(d=1000):
    """tests/test_lapprox_host.py's diagonal quadratic: float32 state on the device, the closure computes in float64 and rounds the gradient."""
    import torch
    rng = np.random.default_rng(0)
    a, c = 10.0 ** rng.uniform(-1, 1, d), rng.standard_normal(d)
    at, ct = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()

    def fn(q):
        r = q.double() - ct
        return float(-0.5 * (at * r * r).sum()), (-at * r).float()
    return fn, (lambda q: (float(-0.5 * (a * (q - c) ** 2).sum()), -a * (q - c)))


def test_optimize_hip_follows_the_restatement_and_converges(gpu):
    import torch
    from montecosmo_amd import samplers
    fn, fn_n = _diag_quadratic_dev()
    q0 = torch.zeros(1000, dtype=torch.float32, device="cuda")
    _, pots_r, _ = ref.optimize(fn_n, np.zeros(1000), lr0=0.1, n_epochs=500)
    q, pots = samplers.optimize(fn, q0, lr0=0.1, n_epochs=500, backend="hip")
    assert len(pots) == 500 and q.dtype == torch.float32 and q.is_cuda and not q0.any()
    rel = np.abs(np.array(pots[:50]) - np.array(pots_r[:50])) / np.array(pots_r[:50])
    print(f"optimize hip: max relative deviation of pots over 50 epochs {rel.max():.2e}; pots[499] / pots[0] = {pots[499] / pots[0]:.3e}")
    assert rel.max() < 1e-5
    assert pots[499] / pots[0] < 1e-3
    q2, pots2 = samplers.optimize(fn, q0, lr0=0.1, n_epochs=500)      # 'auto' is 'hip' here
    assert torch.equal(q, q2) and pots == pots2
    qt, pots_t = samplers.optimize(fn, q0, lr0=0.1, n_epochs=50, backend="torch")      # the same formulas through torch ops
    assert np.allclose(pots_t, pots[:50], rtol=1e-5)


# ---- cov_x_from_pot_x_y(backend='hip') ----------------------------------------------------------------------------------------------
def test_cov_x_hip_on_a_dyadic_coupled_quadratic(gpu):
    """U = 1/2 x^T Q x + 1/2 z^T R z + 2 x^T M z with dyadic coefficients: every gradient the finite differences ask for is exact in float32
    (asserted in the closure), so A = Q, B = 2 M and D = R come out exactly and cov_x is the closed form up to the float64 Schur sum."""
    import torch
    from montecosmo_amd import lapprox
    m, n = 3, 4096
    rng = np.random.default_rng(11)
    Q = np.array([[4., 1., 0.], [1., 5., -1.], [0., -1., 6.]])
    M = np.zeros((m, n))
    for i in range(m):
        M[i, rng.choice(n, 16, replace=False)] = rng.choice([-1., 1.], 16) / 8.0
    R = rng.integers(1, 5, n).astype(np.float64)
    Qt, Mt, Rt = (torch.from_numpy(a).cuda() for a in (Q, M, R))
    exact = []

    def fn(q):
        x, z = q[:m].double(), q[m:].double()
        gx, gz = Qt @ x + 2 * (Mt @ z), 2 * (Mt.T @ x) + Rt * z
        g64 = -torch.cat([gx, gz])
        g = g64.float()
        exact.append(bool(torch.equal(g.double(), g64)))
        return float(-0.5 * (x @ gx + z @ gz)), g
    q = torch.from_numpy((rng.integers(-32, 33, m + n) / 16.0).astype(F32)).cuda()      # a 2^-4 grid in [-2, 2]
    cov, schur = lapprox.cov_x_from_pot_x_y(fn, q, m, method="hutchinson", chunk_size=8, fd_step=0.5, backend="hip")
    assert len(exact) == 2 * m + 2 * 8 and all(exact)      # the rounding of every gradient was exact
    eps_diag = 1e-9
    want_schur = Q - 4 * (M / (R + eps_diag)) @ M.T
    want = np.linalg.inv(want_schur)
    print(f"cov_x hip: max |cov - closed form| = {np.abs(cov - want).max():.2e}, max |schur - closed form| = {np.abs(schur - want_schur).max():.2e}")
    assert np.abs(cov - want).max() < 1e-10 and np.array_equal(schur, schur.T)
    D = lapprox.hess_diag_hutchinson(fn, q, n_probes=8, fd_step=0.5, start=m, backend="hip")
    assert np.array_equal(D.cpu().numpy(), np.r_[np.zeros(m), R])


# ---- on the model -------------------------------------------------------------------------------------------------------------------
def test_map_and_laplace_on_the_model(gpu):
    """The 8^3 LPT model of tests/test_gpu_samplers.py from its `kaiser_post` start: Adam lowers the potential over the first 30 epochs, and at
    the end point the Laplace approximation of the scalars is finite, symmetric, has a positive Schur diagonal, and repeats bit for bit.
    100 epochs, not 30: after 30 (potential 5563.00 -> 5462.34, one MI355X) the Schur diagonal of (sigma8_, b1_, b2_) with 8 probes and
    fd_step = 0.05 was [1.76e-2, 1.19e-3, -4.9e-6]: b2_, which this model's data (pure noise) do not constrain, was not yet at a mode.
    After 100 (potential 5447.39) it is [2.11e-2, 1.71e-3, 4.33e-6], and positive for fd_step 0.05 .. 1 with 8 or 32 probes."""
    import torch
    from test_gpu_samplers import _setup
    from montecosmo_amd import lapprox
    samplers, flat, _, _ = _setup("lpt")
    q0 = flat.pack(flat.ld.kaiser_post(1, scale_field=7 / 8))
    n_epochs = 100
    q, pots = samplers.optimize(flat, q0, lr0=0.1, n_epochs=n_epochs)
    print(f"model: potential {pots[0]:.2f} -> {pots[29]:.2f} (30 epochs) -> {pots[-1]:.2f} ({n_epochs} epochs), dimension {q.numel()}")
    assert len(pots) == n_epochs and all(math.isfinite(p) for p in pots) and pots[29] < pots[0] and pots[-1] < pots[0]
    q2, pots2 = samplers.optimize(flat, q0, lr0=0.1, n_epochs=n_epochs)
    assert torch.equal(q, q2) and pots == pots2
    run = lambda: lapprox.cov_x_from_pot_x_y(flat, q, flat.ns, method="hutchinson", chunk_size=8, seed=42, fd_step=0.05)
    cov, schur = run()
    print("model: schur diagonal", np.diag(schur), "Laplace std of the scalars (sample space)", np.sqrt(np.abs(np.diag(cov))))
    assert cov.shape == schur.shape == (flat.ns, flat.ns)
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(schur))
    assert np.array_equal(schur, schur.T) and np.allclose(cov, cov.T, rtol=1e-9, atol=0)
    assert np.all(np.diag(schur) > 0)
    cov2, schur2 = run()
    assert np.array_equal(cov, cov2) and np.array_equal(schur, schur2)
