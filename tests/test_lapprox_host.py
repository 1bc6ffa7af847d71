"""MAP optimisation and the Laplace approximation, host side (no GPU): `samplers.optimize` and `lapprox` through backend='torch' in
float64 against the numpy restatement (_lapprox_f64.py) and closed forms, the Rademacher hash, and the four exported symbols."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import _lapprox_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _diag_quadratic(d=1000):
    """U = 1/2 sum a_i (q_i - c_i)^2, a_i = 10^U(-1, 1), c ~ N(0, 1); as (torch closure, numpy closure)."""
    rng = np.random.default_rng(0)
    a, c = 10.0 ** rng.uniform(-1, 1, d), rng.standard_normal(d)
    at, ct = torch.from_numpy(a), torch.from_numpy(c)
    fn_t = lambda q: (float(-0.5 * (at * (q - ct) ** 2).sum()), -at * (q - ct))
    fn_n = lambda q: (float(-0.5 * (a * (q - c) ** 2).sum()), -a * (q - c))
    return fn_t, fn_n


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
def test_first_adam_step_moves_every_coordinate_by_lr0_g_over_abs_g():
    from montecosmo_amd import samplers
    g = torch.tensor([3.0, -0.25, 1e-3, -40.0, 1e-9], dtype=F64)
    lr0, eps = 0.1, 1e-8
    q0 = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.0], dtype=F64)
    q, pots = samplers.optimize(lambda q: (-1.5, g), q0, lr0=lr0, n_epochs=1, eps=eps, backend="torch")
    assert pots == [1.5]
    assert torch.allclose(q - q0, lr0 * g / (g.abs() + eps), rtol=1e-14, atol=0)


def test_optimize_follows_the_numpy_restatement_and_converges():
    from montecosmo_amd import samplers
    fn_t, fn_n = _diag_quadratic()
    starts = []
    orig = fn_t
    def fn(q):
        starts.append(q.clone())
        return orig(q)
    q, pots = samplers.optimize(fn, torch.zeros(1000, dtype=F64), lr0=0.1, n_epochs=500, backend="torch")
    q_r, pots_r, traj_r = ref.optimize(fn_n, np.zeros(1000), lr0=0.1, n_epochs=500)
    assert len(pots) == 500 and q.dtype == F64
    assert max(np.abs(s.numpy() - t).max() for s, t in zip(starts, traj_r)) < 1e-12
    assert np.abs(q.numpy() - q_r).max() < 1e-12
    assert np.allclose(pots, pots_r, rtol=1e-12, atol=1e-12)
    print("pots[499] / pots[0] =", pots[499] / pots[0], "restatement", pots_r[499] / pots_r[0])
    assert pots[499] / pots[0] < 1e-3
    # nothing is random: a second run is the same run
    q2, pots2 = samplers.optimize(fn_t, torch.zeros(1000, dtype=F64), lr0=0.1, n_epochs=500, backend="torch")
    assert torch.equal(q, q2) and pots == pots2
    # 'auto' on a CPU tensor is 'torch'
    q3, _ = samplers.optimize(fn_t, torch.zeros(1000, dtype=F64), lr0=0.1, n_epochs=3)
    q4, _ = samplers.optimize(fn_t, torch.zeros(1000, dtype=F64), lr0=0.1, n_epochs=3, backend="torch")
    assert torch.equal(q3, q4)
    with pytest.raises(ValueError):
        samplers.optimize(fn_t, torch.zeros(1000, dtype=F64), backend="hip")
    with pytest.raises(ValueError):
        samplers.optimize(fn_t, torch.zeros(1000, dtype=F64), backend="eager")


def test_optimize_stops_at_the_edge_of_the_support_and_raises_on_nan():
    """-inf (what FlatLogDensity returns outside the support): the last point with a finite potential comes back, pots up to there."""
    from montecosmo_amd import samplers
    seen = []

    def fn(q):      # support q_0 < 0.25: the first steps of size 0.1, 0.1 / sqrt 2, ... cross it during the third update
        seen.append(q.clone())
        if float(q[0]) >= 0.25:
            return -math.inf, torch.zeros_like(q)
        return float(q.sum()), torch.ones_like(q)
    q, pots = samplers.optimize(fn, torch.zeros(3, dtype=F64), lr0=0.1, n_epochs=20, backend="torch")
    assert 1 <= len(pots) < 20 and len(seen) == len(pots) + 1
    assert torch.equal(q, seen[len(pots) - 1]) and float(q[0]) < 0.25 and all(math.isfinite(p) for p in pots)
    calls = []
    cb_q, cb_pots = samplers.optimize(fn, torch.zeros(3, dtype=F64), lr0=0.1, n_epochs=2, backend="torch", callback=lambda i, info: calls.append((i, info)))
    assert [c[0] for c in calls] == [0, 1] and calls[1][1]["lr"] == 0.1 / math.sqrt(2.0) and calls[0][1]["potential"] == cb_pots[0]
    with pytest.raises(FloatingPointError):
        samplers.optimize(lambda q: (math.nan, q), torch.zeros(3, dtype=F64), n_epochs=2, backend="torch")


# ---- the hash -----------------------------------------------------------------------------------------------------------------------
def test_splitmix64_known_answers():
    """The first outputs of the published splitmix64 generator seeded with 0 (state advances by the golden-ratio increment): the
    function here adds the increment itself, so output k is splitmix64(k * increment)."""
    inc = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [int(ref.splitmix64(np.uint64((k * inc) % 2 ** 64))) for k in range(3)]
    assert got == want


@pytest.mark.parametrize("d", [64, 4099, 2 ** 18])
def test_hash_is_rademacher_balanced_and_uncorrelated(d):
    from montecosmo_amd import lapprox
    rs = [ref.rademacher(42, p, d) for p in range(8)]
    for p, r in enumerate(rs):
        assert np.all(np.abs(r) == 1.0)
        assert np.array_equal(r, lapprox.rademacher(42, p, d))      # the product's numpy hash is the restatement's
        assert abs(r.sum()) <= 4 * math.sqrt(d), (p, r.sum())
    worst = max(abs(rs[a] @ rs[b]) for a in range(8) for b in range(a))
    print(f"d = {d}: max |sum r| = {max(abs(r.sum()) for r in rs) / math.sqrt(d):.3f} sqrt d, max |r_p . r_p'| = {worst / math.sqrt(d):.3f} sqrt d")
    assert worst <= 5 * math.sqrt(d)
    sub = lapprox.rademacher(42, 3, d, 5, d - 7)
    assert np.array_equal(sub[5:d - 7], rs[3][5:d - 7]) and not sub[:5].any() and not sub[d - 7:].any()      # a function of the index alone
    assert not np.array_equal(ref.rademacher(43, 0, d), rs[0])


# ---- the Laplace approximation ------------------------------------------------------------------------------------------------------
def _coupled_quadratic(m, n, seed=0):
    """The reference's commented check (lapprox.py:104-141): U = 1/2 x^T Q x + 1/2 z^T R z + 2 x^T M z, R diagonal."""
    rng = np.random.default_rng(seed)
    M = 0.01 * rng.standard_normal((m, n))
    c = rng.standard_normal((m, m))
    Q = c @ c.T + np.eye(m)
    R = np.abs(rng.standard_normal(n)) + 0.05
    H = np.block([[Q, 2 * M], [2 * M.T, np.diag(R)]])
    Qt, Mt, Rt = torch.from_numpy(Q), torch.from_numpy(M), torch.from_numpy(R)

    def fn(q):      # the blocks, not the dense matrix: a gradient costs O(m n)
        x, z = q[:m], q[m:]
        gx, gz = Qt @ x + 2 * (Mt @ z), 2 * (Mt.T @ x) + Rt * z
        return float(-0.5 * (x @ gx + z @ gz)), -torch.cat([gx, gz])
    return fn, H


_WANT = {}


def _block_of_inverse(n, H, m, eps_diag):
    """Top-left m x m block of the inverse of the full Hessian with eps_diag added to D (computed once per size: both methods share it)."""
    if (n, eps_diag) not in _WANT:
        Hr = H + eps_diag * np.diag(np.r_[np.zeros(m), np.ones(n)])
        _WANT[n, eps_diag] = np.linalg.solve(Hr, np.eye(m + n)[:, :m])[:m]
    return _WANT[n, eps_diag]


@pytest.mark.parametrize("n", [6, 4096])
@pytest.mark.parametrize("method", ["exact", "hutchinson"])
def test_cov_x_is_the_top_left_block_of_the_inverse_hessian(n, method):
    """D is diagonal here and central differences of a quadratic are exact, so both methods give the block of the full inverse."""
    from montecosmo_amd import lapprox
    m = 3
    fn, H = _coupled_quadratic(m, n)
    q = torch.from_numpy(np.random.default_rng(1).standard_normal(m + n) * 0.1)
    cov, schur = lapprox.cov_x_from_pot_x_y(fn, q, m, method=method, chunk_size=4, eps_diag=0.0, fd_step=0.5, backend="torch")
    want = _block_of_inverse(n, H, m, 0.0)
    assert cov.shape == schur.shape == (m, m) and cov.dtype == np.float64
    assert np.abs(cov - want).max() < 1e-9, np.abs(cov - want).max()
    assert np.array_equal(schur, schur.T)
    # the default eps_diag = 1e-9 is added to D: the block of the inverse of the Hessian with that D
    cov2, _ = lapprox.cov_x_from_pot_x_y(fn, q, m, method=method, chunk_size=4, fd_step=0.5)
    want2 = _block_of_inverse(n, H, m, 1e-9)
    assert np.abs(cov2 - want2).max() < 1e-9


def _rank_one(d=257, seed=3):
    rng = np.random.default_rng(seed)
    a, u = 10.0 ** rng.uniform(-1, 1, d), rng.standard_normal(d) / math.sqrt(d)
    H = np.diag(a) + np.outer(u, u)
    Ht = torch.from_numpy(H)
    return (lambda q: (float(-0.5 * q @ Ht @ q), -(Ht @ q))), (lambda q: H @ q), H


def test_hutchinson_equals_the_restatement_with_the_same_probes():
    from montecosmo_amd import lapprox
    fn, grad_U, H = _rank_one()
    d = H.shape[0]
    q = np.random.default_rng(4).standard_normal(d)
    got = lapprox.hess_diag_hutchinson(fn, torch.from_numpy(q), n_probes=16, seed=42, fd_step=0.25, backend="torch")
    want = ref.hess_diag_hutchinson(grad_U, q, 16, 42, 0.25)
    assert got.dtype == F64 and np.abs(got.numpy() - want).max() < 1e-12
    # an estimate of the diagonal: the error of an entry is its row's off-diagonal mass over sqrt(n_probes)
    off = np.sqrt((H ** 2).sum(1) - np.diag(H) ** 2)
    assert np.all(np.abs(want - np.diag(H)) < 6 * off / math.sqrt(16) + 1e-12)
    # start / stop: the other entries are held fixed and stay exactly 0
    sub = lapprox.hess_diag_hutchinson(fn, torch.from_numpy(q), n_probes=8, seed=7, fd_step=0.25, start=3, stop=200, backend="torch")
    want = ref.hess_diag_hutchinson(grad_U, q, 8, 7, 0.25, 3, 200)
    assert np.abs(sub.numpy() - want).max() < 1e-12
    assert not sub[:3].any() and not sub[200:].any() and sub[3:200].abs().min() > 0
    with pytest.raises(ValueError):
        lapprox.hess_diag_hutchinson(fn, torch.from_numpy(q), start=5, stop=3, backend="torch")


def test_exact_diagonal_on_indices_and_its_alias():
    from montecosmo_amd import lapprox
    fn, _, H = _rank_one(d=40)
    q = torch.from_numpy(np.random.default_rng(5).standard_normal(40))
    full = lapprox.hess_diag_exact(fn, q, fd_step=0.5)
    assert full.shape == (40,) and np.abs(full.numpy() - np.diag(H)).max() < 1e-12
    some = lapprox.hess_diag_in_chunks(fn, q, chunk_size=7, indices=[39, 0, 17], fd_step=0.5)
    assert np.abs(some.numpy() - np.diag(H)[[39, 0, 17]]).max() < 1e-12
    with pytest.raises(FloatingPointError):      # a step that leaves the support is an error, not a zero gradient
        lapprox.hess_diag_exact(lambda x: (-math.inf, torch.zeros_like(x)), q, indices=[0], fd_step=0.5)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_version_is_unchanged_and_the_new_symbols_resolve():
    from montecosmo_amd import _lib
    assert _lib.lib.mcpm_version() == b"mcpm 0.12 (gfx950)"
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    n_args = {"mcpm_adam_step_f32": 12, "mcpm_probe_shift_f32": 10, "mcpm_hutchinson_accum_f64": 10, "mcpm_schur_f64": 8}
    for name, n in n_args.items():
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(raw, name) and len(_lib.SIGNATURES[name][1]) == n
        decl = re.search(name + r"\(([^)]*)\)", header).group(1)
        assert len(decl.split(",")) == n, name
    assert "splitmix64" in header
    # argument errors come back as codes without a device: a NULL plan
    assert raw.mcpm_schur_f64(None, None, 17, 1, 1, None, C.c_double(0.), None) == -6
