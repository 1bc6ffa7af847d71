"""Kaiser model on the curved sky and on the light cone on the GPU (bricks.kaiser_sky / kaiser_sky_vjp: mcpm_kspace_hessian_f32 or the mu^2
multiply, batched C2R, mcpm_kaiser_sky_f32 and its two VJPs) against the float64 restatement tests/_kaiser_f64.py, which takes the
reference's harmonic route.  Both sides read the same tables (the package's), so this is a check of the kernels alone.  Gates: the
kernel-level 2e-5 of tests/test_gpu_png.py forward and for the transpose in `lin` (the map is linear in it); 3e-3 of central differences of
the restatement for the scalar and table cotangents (tests/test_gpu_png.py, tests/test_gpu_bias.py::test_lightcone_table_cotangents)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _kaiser_f64 as kf  # noqa: E402
from oracle import pm_oracle as o  # noqa: E402  (checker only)

# mesh -> the final mesh (cells of 40 Mpc/h) whose box it spans.  (14, 20, 28): (8, 12, 16) at 7/4, non-cubic cells, nz % 4 = 0;
# (10, 6, 14): 840 cells (no multiple of a workgroup), non-cubic, nz % 4 = 2; (64, 64, 64): the smallest cube the hand-written transforms take
SHAPES = [(14, 20, 28), (10, 6, 14), (64, 64, 64)]
FINAL = {(14, 20, 28): (8, 12, 16), (10, 6, 14): (6, 4, 8), (64, 64, 64): (36, 36, 36)}
BRANCHES = {"C-fixed": (True, 0.65), "C-lightcone": (True, None), "F-lightcone": (False, None)}
CENTER, ROTVEC, CELL = (60., -40., 1400.), (0.1, 0.2, -0.1), 40.
B1E = 1.0      # 1 + b1 with b1 = 0: the l = 2 share is then about 0.19 (E[mu^4] = 1/5, Planck18 growth rate)
_REF = {}


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def setup(shape, branch, with_phi):
    """Inputs and the restatement's answers for one case, computed once and shared by the tests (read-only)."""
    key = (shape, branch, with_phi)
    if key in _REF:
        return _REF[key]
    from montecosmo_amd import bricks, nbody
    curved, a_obs = BRANCHES[branch]
    rng = np.random.default_rng(101)
    cosmo = bricks.Planck18()
    cfg = dict(box_size=np.multiply(FINAL[shape], CELL), box_center=np.array(CENTER), box_rotvec=np.array(ROTVEC), a_obs=a_obs, curved_sky=curved)
    d, gt = nbody._dist_cache(cosmo), nbody._growth_cache(cosmo)
    tables = {"chi": d["chi"][::-1].copy(), "a_chi": d["a"][::-1].copy(), "a": gt["a"].copy(), "g": gt["g"].copy(), "f": gt["f"].copy()}
    trans = bricks.trans_phi2delta_table(cosmo) if with_phi else None
    X = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    X[0, 0, 0] = 0.                                     # a linear field has no k = 0 mode: the contract of kaiser_sky
    lin = X.astype(np.complex64)
    lin64 = lin.astype(np.complex128)
    fNL_bp = 0.
    if with_phi:      # fNL_bp such that the phi term is 0.3 of the norm of the rest
        rest, p1 = kf.kaiser_sky(cfg, None, lin64, B1E, tables=tables), kf.kaiser_sky(cfg, None, lin64, B1E, 1., trans, tables=tables)
        fNL_bp = 0.3 * float(np.linalg.norm(rest - 1.) / np.linalg.norm(p1 - rest))
    F = lambda **kw: kf.kaiser_sky(cfg, None, kw.pop("lin", lin64), kw.pop("b1E", B1E), kw.pop("fNL_bp", fNL_bp), kw.pop("trans", trans),
                                   tables=kw.pop("tables", tables), **kw)
    want, parts = F(return_parts=True)
    ob = rng.standard_normal(shape).astype(np.float32)
    _REF[key] = dict(cfg=cfg, cosmo=cosmo, tables=tables, trans=trans, lin=lin, fNL_bp=fNL_bp, F=F, want=want, parts=parts, ob=ob, rng=rng,
                     kw=dict(box_size=cfg["box_size"], box_center=CENTER, box_rot=ROTVEC, b1E=B1E, fNL_bp=fNL_bp if with_phi else None, a_obs=a_obs,
                             curved_sky=curved))
    return _REF[key]


CASES = [(s, b, p) for s in SHAPES for b in BRANCHES for p in (False, True)]
cid = lambda c: f"{'x'.join(map(str, c[0]))}-{c[1]}-{'phi' if c[2] else 'nophi'}"


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_forward(gpu, case):
    from montecosmo_amd import bricks
    S = setup(*case)
    want, parts = S["want"], S["parts"]
    # conditions under which a wrong term cannot hide
    n = np.linalg.norm(want - 1.)
    assert np.linalg.norm(parts["l2"]) >= 0.1 * n, ("l = 2 share", np.linalg.norm(parts["l2"]) / n)
    if case[2]:
        assert np.linalg.norm(parts["phi"]) >= 0.1 * n, ("phi share", np.linalg.norm(parts["phi"]) / n)
    if BRANCHES[case[1]][1] is None:
        assert np.ptp(parts["g"]) > 0.01 * np.mean(parts["g"])
    assert parts["r"].min() > 0.
    out = bricks.kaiser_sky(S["cosmo"], S["lin"], **S["kw"])
    again = bricks.kaiser_sky(S["cosmo"], S["lin"], **S["kw"])
    assert tuple(out.shape) == case[0] and str(out.dtype) == "torch.float32"
    assert bool((out == again).all()), "repeat calls must be bitwise equal"
    got = out.cpu().numpy().astype(np.float64)
    scale = np.abs(want - 1.).max()
    e2, em = rel_l2(got - 1., want - 1.), np.abs(got - want).max() / scale
    print(f"kaiser_sky[{cid(case)}] rel L2 {e2:.3e} max {em:.3e} (l2 share {np.linalg.norm(parts['l2']) / n:.3f})")
    assert np.isfinite(got).all()
    assert e2 < 2e-5 and em < 2e-5


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_vjp(gpu, case):
    """The transpose in `lin` against the restatement's exact transpose; scalar, table and transfer-table cotangents against central
    differences of the restatement along random directions; a second call bitwise equal."""
    from montecosmo_amd import bricks
    S = setup(*case)
    shape, (curved, a_obs), with_phi = case[0], BRANCHES[case[1]], case[2]
    rng, ob, F = np.random.default_rng(202), S["ob"], S["F"]
    ob64 = ob.astype(np.float64)
    L = lambda **kw: float((ob64 * F(**kw)).sum())
    _, ctx = bricks.kaiser_sky(S["cosmo"], S["lin"], return_ctx=True, **S["kw"])
    r, r2 = bricks.kaiser_sky_vjp(ctx, ob), bricks.kaiser_sky_vjp(ctx, ob)
    assert bool((r["lin_mesh"] == r2["lin_mesh"]).all()) and r["b1E"] == r2["b1E"] and r["fNL_bp"] == r2["fNL_bp"], "repeat calls must be bitwise equal"
    # linear in lin: the exact transpose.  Both cotangents are brought to the real field whose spectrum lin is (the adjoint of rfftn), which
    # removes the freedom the real-pair convention leaves on the Hermitian-redundant kz = 0 / Nyquist planes
    want = kf.kaiser_sky_lin_vjp(S["cfg"], None, ob64, B1E, S["fNL_bp"], S["trans"], tables=S["tables"])
    got = r["lin_mesh"].cpu().numpy().astype(np.complex128)
    if curved:      # delta is taken as the trace of the six meshes, which carry no k = 0 mode: the contract is for `lin` without one, and
        assert got[0, 0, 0] == 0.      # the transpose is compared on that subspace (white2lin multiplies the k = 0 entry by P(0) = 0 anyway)
        want[0, 0, 0] = 0.
    gx, wx = o.rfftn_vjp(got, shape), o.rfftn_vjp(want, shape)
    e2, em = rel_l2(gx, wx), np.abs(gx - wx).max() / np.abs(wx).max()
    print(f"kaiser_sky_vjp[{cid(case)}] lin rel L2 {e2:.3e} max {em:.3e}")
    assert e2 < 2e-5 and em < 2e-5
    # scalars
    eps = 1e-5
    fd = (L(b1E=B1E + eps) - L(b1E=B1E - eps)) / (2 * eps)
    print(f"kaiser_sky_vjp[{cid(case)}] b1E fd {fd:.6e} an {r['b1E']:.6e}")
    assert abs(fd - r["b1E"]) < 3e-3 * abs(fd)
    if with_phi:
        h = eps * S["fNL_bp"]
        fd = (L(fNL_bp=S["fNL_bp"] + h) - L(fNL_bp=S["fNL_bp"] - h)) / (2 * h)
        print(f"kaiser_sky_vjp[{cid(case)}] fNL_bp fd {fd:.6e} an {r['fNL_bp']:.6e}")
        assert abs(fd - r["fNL_bp"]) < 3e-3 * abs(fd)
        ks, tr = S["trans"]
        dirn = tr * rng.standard_normal(len(tr))
        fd = (L(trans=(ks, tr + eps * dirn)) - L(trans=(ks, tr - eps * dirn))) / (2 * eps)
        an = float(np.dot(r["trans_bar"], dirn))
        print(f"kaiser_sky_vjp[{cid(case)}] transfer table fd {fd:.6e} an {an:.6e}")
        assert abs(fd - an) < 3e-3 * max(abs(fd), np.linalg.norm(r["trans_bar"] * dirn))
        assert np.array_equal(r["trans_bar"], r2["trans_bar"])
    else:
        assert r["fNL_bp"] == 0. and r["trans_bar"] is None
    T = S["tables"]
    if a_obs is not None:
        assert "tables" not in r and r["g"] == r2["g"] and r["f"] == r2["f"]
        g0, f0 = np.interp(a_obs, T["a"], T["g"]), np.interp(a_obs, T["a"], T["f"])
        for k, base, other in (("g", g0, lambda v: (v, f0)), ("f", f0, lambda v: (g0, v))):
            fd = (L(gf=other(base + eps)) - L(gf=other(base - eps))) / (2 * eps)
            print(f"kaiser_sky_vjp[{cid(case)}] {k} fd {fd:.6e} an {r[k]:.6e}")
            assert abs(fd - r[k]) < 3e-3 * abs(fd)
    else:
        assert "g" not in r
        for k in ("chi", "g", "f"):
            assert np.array_equal(r["tables"][k], r2["tables"][k]) and np.isfinite(r["tables"][k]).all()
            # a random direction per node; steps of 1e-6 of a node spacing (chi) or of the entry keep every cell inside its bracket: no
            # sample crosses a kink of the piecewise-linear look-ups
            dirn = rng.standard_normal(len(T[k])) * (np.abs(np.gradient(T[k])) if k == "chi" else np.abs(T[k]))
            e = 1e-6
            fd = (L(tables=dict(T, **{k: T[k] + e * dirn})) - L(tables=dict(T, **{k: T[k] - e * dirn}))) / (2 * e)
            an = float(np.dot(r["tables"][k], dirn))
            print(f"kaiser_sky_vjp[{cid(case)}] table {k} fd {fd:.6e} an {an:.6e}")
            assert abs(fd - an) < 3e-3 * max(abs(fd), np.linalg.norm(r["tables"][k] * dirn))


def test_cell_at_the_observer_is_finite(gpu):
    """A cell exactly at the observer (r = 0): direction 0, a the clamped end of the table, a finite output (no reference value there)."""
    from montecosmo_amd import bricks
    shape = (8, 8, 8)
    rng = np.random.default_rng(303)
    X = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    X[0, 0, 0] = 0.
    box = np.multiply(shape, CELL)
    for a_obs in (0.65, None):      # centre = box / 2 - 3 cells: cell (3, 3, 3) sits at the origin
        out = bricks.kaiser_sky(bricks.Planck18(), X.astype(np.complex64), box, box / 2 - 3 * CELL, (0., 0., 0.), B1E, a_obs=a_obs, curved_sky=True)
        assert bool(out.isfinite().all())
