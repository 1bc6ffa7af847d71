"""Alcock-Paczynski remapping fused into the observation pass (mcpm_observe_pos_ap_f32 and its two VJPs; model.py:787-794,
bricks.py:795-814 ap_auto, :848-857 ap_param) against the float64 restatement tests/_ap_f64.py: forward, the particle and alpha
cotangents against central differences, the cotangent of the chi nodes against a directional difference, and the bitwise
guarantees (mode none = the old entry points; repeat calls equal)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pm_oracle as o, bias_oracle as bo  # noqa: E402  (checker only)
import _ap_f64 as apo  # noqa: E402


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


EVOL, PAINT = (16, 16, 16), (24, 20, 16)
BOX, CENTER, ROTVEC = (640., 640., 640.), (100., -50., 1500.), (0.2, -0.1, 0.3)
AP = {"alpha_iso": 1.03, "alpha_ap": 0.97}
AP_WIDE = {"alpha_iso": 1.03, "alpha_ap": 0.90}      # flat sky: alpha_par = 0.960, alpha_perp = 1.067 (see _condition)
CASES = [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]


def _setup(lattice, seed=21):
    from montecosmo_amd import bricks, nbody
    rng = np.random.default_rng(seed)
    cosmo, cosmo_fid = bricks.Planck18(Omega_c=0.25 - 0.0490), bricks.Planck18()      # sampled Omega_m = 0.25 against the fiducial
    N = 16 ** 3
    disp = (1.5 * rng.standard_normal((N, 3))).astype(np.float32)
    vel = (3.0 * rng.standard_normal((N, 3))).astype(np.float32)
    dvel = (0.5 * rng.standard_normal((N, 3))).astype(np.float32)
    lp = nbody.LatticePos(disp, EVOL)
    x64 = lp.to_absolute().cpu().numpy()
    pos_in = lp if lattice else x64.astype(np.float32)
    if not lattice:
        x64 = pos_in.astype(np.float64)
    return rng, cosmo, cosmo_fid, pos_in, x64, vel, dvel


def _condition(cosmo, cosmo_fid, x64, vel, dvel, a_obs, curved, auto, ap=AP, per_axis=False):
    """From the restatement alone: Alcock-Paczynski moves some particle by more than one cell, and every r' is inside the
    distance table (so that a pass with the step absent, or clamped, cannot satisfy the comparisons below).
    "One cell" is the edge of the finest paint cell, 640 / 24 = 26.7 Mpc/h, against the length of the displacement.  Measured on the
    CPU: 41 Mpc/h and more in six of the eight cases (1.48 .. 1.55 cells along one axis), 28.7 Mpc/h for the two flat-sky `param` cases
    (alpha_par = 1.009, alpha_perp = 1.041: 0.73 cells along one axis, 0.85 cells in the per-axis cell metric) -- 4000 times the
    forward tolerance in every case.  `per_axis`: also ask for more than one cell along one axis of the paint mesh, which AP_WIDE gives on the
    flat sky (84 Mpc/h, 2.0 cells along one axis; measured on the CPU)."""
    R = bo.rotvec_matrix(ROTVEC)
    los, p = apo.observe_phys(cosmo, x64, vel.astype(np.float64), CENTER, R, BOX, EVOL, a_obs, curved, dvel.astype(np.float64))
    p2 = apo.apply_ap(p, los, cosmo, curved, auto, ap, cosmo_fid)
    moved = np.linalg.norm(p2 - p, axis=-1).max() / np.divide(BOX, PAINT).min()
    cells = np.abs(bo.phys2cell_pos(p2, CENTER, R, BOX, PAINT) - bo.phys2cell_pos(p, CENTER, R, BOX, PAINT)).max()
    print("condition", curved, a_obs, auto, moved, cells)
    assert moved > 1.0, moved
    assert not per_axis or cells > 1.0, cells
    rp = apo.ap_rpos(p, los, curved)
    c = o._dist_table(cosmo)
    assert c["chi"].min() < rp.min() and rp.max() < c["chi"].max()


@pytest.mark.parametrize("auto", [True, False])
@pytest.mark.parametrize("curved,lightcone,lattice", CASES)
def test_observe_pos_ap_forward_and_vjp(gpu, curved, lightcone, lattice, auto):
    """Forward at the tolerances of test_observe_pos_forward_and_vjp (2e-4 cells absolute, 2e-5 relative L2 of the displacement);
    VJP w.r.t. pos, vel, dvel, alpha_iso, alpha_ap against central differences of the restatement (2e-3 rule of that test)."""
    _forward_and_vjp(curved, lightcone, lattice, auto, AP, per_axis=auto or curved)


@pytest.mark.parametrize("lightcone,lattice", [(True, False), (False, True)])
def test_observe_pos_ap_param_flat_sky_wide(gpu, lightcone, lattice):
    """The two flat-sky `param` cases once more with alpha_ap = 0.90, so that some particle moves by more than one cell along one
    axis of the paint mesh as well (same gates)."""
    _forward_and_vjp(False, lightcone, lattice, False, AP_WIDE, per_axis=True)


def _forward_and_vjp(curved, lightcone, lattice, auto, AP, per_axis):
    from montecosmo_amd import bricks
    rng, cosmo, cosmo_fid, pos_in, x64, vel, dvel = _setup(lattice)
    R = bo.rotvec_matrix(ROTVEC)
    a_obs = None if lightcone else 0.7
    _condition(cosmo, cosmo_fid, x64, vel, dvel, a_obs, curved, auto, AP, per_axis)
    got, ctx = bricks.observe_pos(cosmo, pos_in, vel, CENTER, ROTVEC, BOX, EVOL, PAINT, a_obs=a_obs, curved_sky=curved, dvel=dvel,
                                  return_ctx=True, ap_auto=auto, ap=AP, cosmo_fid=cosmo_fid)
    got_abs = got.to_absolute().cpu().numpy() if lattice else got.cpu().numpy().astype(np.float64)
    f = lambda x, v, dv, ap=AP: apo.observe_pos_ap(cosmo, x, v, CENTER, R, BOX, EVOL, PAINT, a_obs, curved, dv, auto, ap, cosmo_fid)
    v64, dv64 = vel.astype(np.float64), dvel.astype(np.float64)
    ref = f(x64, v64, dv64)
    x0 = x64 * np.divide(PAINT, EVOL)
    err_abs, err_rel = np.abs(got_abs - ref).max(), rel_l2(got_abs - x0, ref - x0)
    print("forward", curved, lightcone, lattice, auto, err_abs, err_rel)
    assert err_abs < 2e-4 and err_rel < 2e-5, (err_abs, err_rel)
    ob = rng.standard_normal((len(x64), 3))
    pb, vb, db, gfb, ab = bricks.observe_pos_vjp(ctx, ob.astype(np.float32))
    eps = 1e-4
    for name, bar, idx in (("pos", pb, 0), ("vel", vb, 1), ("dvel", db, 2)):
        d = rng.standard_normal(x64.shape)
        args_p = [x64, v64, dv64]
        args_m = [a.copy() for a in args_p]
        args_p[idx] = args_p[idx] + eps * d
        args_m[idx] = args_m[idx] - eps * d
        fd = ((f(*args_p) - f(*args_m)) * ob).sum() / (2 * eps)
        an = float((bar.double().cpu().numpy() * d).sum())
        print(name, fd, an)
        assert abs(fd - an) < 2e-3 * max(abs(fd), np.linalg.norm(ob) * np.linalg.norm(d) * 1e-2), (name, fd, an)
    if not lightcone:    # scalar growth product, now also through r'
        gf = float(o.a2g(cosmo, 0.7) * o.a2f(cosmo, 0.7))
        fd = ((f(x64, v64 * (1 + eps), dv64) - f(x64, v64 * (1 - eps), dv64)) * ob).sum() / (2 * eps * gf)
        assert abs(fd - gfb) < 2e-3 * abs(fd), ("gf", fd, gfb)
    else:
        assert gfb == 0.0
    if auto:
        assert ab == {"alpha_iso": 0.0, "alpha_ap": 0.0}
        return
    h = 1e-5
    for k in ("alpha_iso", "alpha_ap"):
        fd = ((f(x64, v64, dv64, dict(AP, **{k: AP[k] + h})) - f(x64, v64, dv64, dict(AP, **{k: AP[k] - h}))) * ob).sum() / (2 * h)
        print(k, fd, ab[k])
        if curved and k == "alpha_ap":
            assert fd == 0.0 and ab[k] == 0.0          # exactly: a curved sky reads alpha_iso alone (bricks.py:852-853)
        else:
            assert abs(fd - ab[k]) < 2e-3 * abs(fd), (k, fd, ab[k])


@pytest.mark.parametrize("curved,lightcone,lattice", CASES)
def test_ap_auto_table_cotangent(gpu, curved, lightcone, lattice):
    """chi_bar of mcpm_observe_pos_ap_tables_vjp_f32 against a float64 directional finite difference of the chi NODES of the
    sampled cosmology's chi -> a table (in the manner of test_lightcone_table_cotangents), with the light-cone bit (the growth
    look-up at r and the Alcock-Paczynski look-up at r' share the accumulator) and without it (Alcock-Paczynski alone)."""
    from montecosmo_amd import bricks, nbody
    rng, cosmo, cosmo_fid, pos_in, x64, vel, dvel = _setup(lattice, seed=23)
    R = bo.rotvec_matrix(ROTVEC)
    a_obs = None if lightcone else 0.7
    _, ctx = bricks.observe_pos(cosmo, pos_in, vel, CENTER, ROTVEC, BOX, EVOL, PAINT, a_obs=a_obs, curved_sky=curved, dvel=dvel,
                                return_ctx=True, ap_auto=True, cosmo_fid=cosmo_fid)
    ob = rng.standard_normal((len(x64), 3)).astype(np.float32)
    bar = bricks.observe_pos_tables_vjp(ctx, ob)
    bar2 = bricks.observe_pos_tables_vjp(ctx, ob)
    assert bar.dtype.is_floating_point and bool((bar == bar2).all())          # bitwise repeatable
    bar = bar.cpu().numpy()
    d, df = nbody._dist_cache(cosmo), nbody._dist_cache(cosmo_fid)
    chi, aoc = d["chi"][::-1].copy(), d["a"][::-1].copy()
    nchi = len(chi)
    assert len(bar) == (nchi + 2 * ctx.ngrow if lightcone else nchi)
    v64, dv64 = vel.astype(np.float64), dvel.astype(np.float64)

    def L(chi_nodes):
        chi2a = lambda r: np.interp(r, chi_nodes, aoc)
        P = bo.cell2phys_pos(x64, CENTER, R, BOX, EVOL)
        if curved:
            r = np.linalg.norm(P, axis=-1, keepdims=True)
            los = P / r
        else:
            los = o.safe_div(np.asarray(CENTER), np.linalg.norm(CENTER))
            r = np.abs((P * los).sum(-1, keepdims=True))
        a = chi2a(r) if lightcone else a_obs
        V = bo.cell2phys_vel(v64, R, BOX, EVOL) * (o.a2g(cosmo, a) * o.a2f(cosmo, a)) + dv64
        Pp = P + (V * los).sum(-1, keepdims=True) * los
        Pp = apo.ap_auto(Pp, los, cosmo, cosmo_fid, curved, chi2a=chi2a, a2chi_fid=lambda a_: np.interp(a_, df["a"], df["chi"]))
        return float((bo.phys2cell_pos(Pp, CENTER, R, BOX, PAINT) * ob).sum())

    dirn = rng.standard_normal(nchi) * np.abs(np.gradient(chi))
    eps = 1e-6
    fd = (L(chi + eps * dirn) - L(chi - eps * dirn)) / (2 * eps)
    an = float(np.dot(bar[:nchi], dirn))
    scale = np.linalg.norm(bar[:nchi] * dirn) + 1e-30
    print("chi_bar", curved, lightcone, fd, an, scale)
    assert np.any(bar[:nchi]) and abs(fd - an) < 2e-3 * max(abs(fd), scale), (fd, an, scale)


@pytest.mark.parametrize("curved,lightcone,lattice", CASES)
def test_ap_none_is_bitwise_the_old_entry_points(gpu, curved, lightcone, lattice):
    """MCPM_AP_NONE through the new entry points = the old entry points, bit for bit (forward, VJP, tables VJP)."""
    import torch
    from montecosmo_amd import bricks, nbody, _lib
    rng, cosmo, cosmo_fid, pos_in, x64, vel, dvel = _setup(lattice)
    a_obs = None if lightcone else 0.7
    old, c = bricks.observe_pos(cosmo, pos_in, vel, CENTER, ROTVEC, BOX, EVOL, PAINT, a_obs=a_obs, curved_sky=curved, dvel=dvel, return_ctx=True)
    n, dev, P = c.n, c.p.device, nbody._ptr
    common = (P(c.p), P(c.v), P(c.dv), n, c.mode, c.geom, c.flags, P(c.tables), c.nchi, c.ngrow)
    none = (_lib.AP_NONE, 1.0, 1.0, None, 0, 0)
    new = torch.empty((n, 3), dtype=torch.float32, device=dev)
    c.plan.call("mcpm_observe_pos_ap_f32", *common, *none, P(new))
    assert torch.equal(new, old.disp if lattice else old)
    ob = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).to(dev)
    outs = []
    for name, extra in (("mcpm_observe_pos_vjp_f32", ()), ("mcpm_observe_pos_ap_vjp_f32", none)):
        pb, vb, db = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(3))
        gfb = torch.zeros(1, dtype=torch.float64, device=dev)
        tail = (None,) if extra else ()
        c.plan.call(name, *common, *extra, P(ob), P(pb), P(vb), P(db), P(gfb), *tail)
        outs.append((pb, vb, db, gfb))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    if lightcone:
        tbs = []
        for name, extra in (("mcpm_observe_pos_tables_vjp_f32", ()), ("mcpm_observe_pos_ap_tables_vjp_f32", none)):
            tb = torch.empty(c.nchi + 2 * c.ngrow, dtype=torch.float64, device=dev)
            c.plan.call(name, *common, *extra, P(ob), P(tb))
            tbs.append(tb)
        assert torch.equal(*tbs) and bool(tbs[0].any())


@pytest.mark.parametrize("auto", [True, False])
def test_ap_cotangents_bitwise_repeatable(gpu, auto):
    """Two calls give bitwise equal particle, scalar and table cotangents."""
    import torch
    from montecosmo_amd import bricks
    rng, cosmo, cosmo_fid, pos_in, x64, vel, dvel = _setup(True)
    for curved, a_obs in ((True, None), (False, 0.7)):
        _, ctx = bricks.observe_pos(cosmo, pos_in, vel, CENTER, ROTVEC, BOX, EVOL, PAINT, a_obs=a_obs, curved_sky=curved, dvel=dvel,
                                    return_ctx=True, ap_auto=auto, ap=AP, cosmo_fid=cosmo_fid)
        ob = rng.standard_normal((len(x64), 3)).astype(np.float32)
        r1, r2 = bricks.observe_pos_vjp(ctx, ob), bricks.observe_pos_vjp(ctx, ob)
        assert all(torch.equal(a, b) for a, b in zip(r1[:3], r2[:3])) and r1[3:] == r2[3:]
        if auto or a_obs is None:
            assert torch.equal(bricks.observe_pos_tables_vjp(ctx, ob), bricks.observe_pos_tables_vjp(ctx, ob))
