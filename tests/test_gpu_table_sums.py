"""The order-independent integer table sums (mcpm_tab_begin / mcpm_tab_finish with the device side of tables_dev.h) behind the four table
cotangents mcpm_lightcone_tables_vjp_f32, mcpm_observe_pos_ap_tables_vjp_f32, mcpm_kaiser_sky_tables_vjp_f32 and mcpm_png_add_vjp_f32:
what the shared path promises -- the result does not depend on the order of the elements, it resolves 2^-30 of a kind's largest
contribution per contribution, a non-finite contribution makes the whole table NaN and leaves nothing behind, an oversized table is
refused, and the kind boundaries of every caller are the right ones.  The derivatives themselves are checked by the entry points' own
tests (test_gpu_bias, test_gpu_ap, test_gpu_kaiser_sky, test_gpu_png).

THE BOUND.  Pass 1 rounds a contribution to units of 2^(e - 30), 2^e the power of two above the float (rounded up) of the kind's largest
|contribution| m_k: an error of at most 2^(e - 31) < m_k (1 + 2^-23) 2^-30 each, c_i m_k 2^-30 for an entry that received c_i
contributions.  Against a float64 restatement the tests allow c_i m_k 2^-29 (the factor 2 covers the evaluation-order difference between
numpy and the kernel); between a call and the sum of the same call on two halves of its elements the same figure holds because each
side is within c_i m_k 2^-30 of the exact sum (a half's own maximum is no larger, its units no coarser)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import bias_oracle as bo  # noqa: E402  (checker only)
import _ap_f64 as apo  # noqa: E402
import _kaiser_f64 as kf  # noqa: E402
import _png_f64 as pf  # noqa: E402

N_RAGGED = 1000                      # a ragged last workgroup
N_CAPPED = 2048 * 256 + 257          # the smallest count at which the capped grid's stride loop runs with a ragged tail
NEAR = 1e-9                          # a look-up this close (relative) to a node may take either bracket: its entries are not compared
_C = {}


def lc_tables():
    """chi ascending, a(chi), a, g, g2, f, f2 of Planck18 (as test_lightcone_table_cotangents takes them)."""
    if "T" not in _C:
        from montecosmo_amd import bricks, nbody
        cosmo = bricks.Planck18()
        d, gt = nbody._dist_cache(cosmo), nbody._growth_cache(cosmo)
        _C["T"] = dict(cosmo=cosmo, chi=d["chi"][::-1].copy(), aoc=d["a"][::-1].copy(), a=gt["a"].copy(),
                       **{k: gt[k].copy() for k in ("g", "g2", "f", "f2")})
    return _C["T"]


def lc_inputs(N):
    """r0 uniform in [800, 2600] with the four edge entries of test_lightcone_table_cotangents, and three cotangents."""
    key = ("in", N)
    if key not in _C:
        T = lc_tables()
        rng = np.random.default_rng(4100 + N)
        r0 = rng.uniform(800., 2600., N).astype(np.float32)
        r0[:4] = [1e-3, 5e5, 9e5, 0.5 * (T["chi"][5] + T["chi"][6])]
        _C[key] = (r0,) + tuple(rng.standard_normal(N).astype(np.float32) for _ in range(3))
    return _C[key]


def lc_call(dev, r0, gB, g2B, dB, tabs=None, nchi=None, ng=None, out=None):
    import torch
    from montecosmo_amd import nbody
    T = lc_tables()
    if tabs is None:
        tabs = np.concatenate([T[k] for k in ("chi", "aoc", "a", "g", "g2", "f", "f2")])
        nchi, ng = len(T["chi"]), len(T["a"])
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if out is None:
        out = torch.empty(nchi + 4 * ng, dtype=torch.float64, device=dev)
    nbody.get_plan((16, 16, 16)).call("mcpm_lightcone_tables_vjp_f32", t(r0), len(r0), t(tabs), nchi, ng, t(gB), t(g2B), t(dB), out)
    return out


def bracket(x, xp, fp):
    """The clamped look-up of tables_dev.h::interp_idx in float64: bracket lo, weight t, slope, value; near: within NEAR of a node."""
    n = len(xp)
    lo = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 2)
    dx = xp[lo + 1] - xp[lo]
    below, above = x <= xp[0], x >= xp[-1]
    slope = (fp[lo + 1] - fp[lo]) / dx
    t = np.where(below, 0., np.where(above, 1., (x - xp[lo]) / dx))
    y = np.where(below, fp[0], np.where(above, fp[-1], fp[lo] + slope * (x - xp[lo])))
    near = np.minimum(np.abs(x - xp[lo]), np.abs(x - xp[lo + 1])) <= NEAR * np.abs(x)
    return dict(lo=lo, t=t, slope=np.where(below | above, 0., slope), y=y, near=near, n=n)


def scatter(n, b, v, near):
    """Sum of v (1 - t), v t at the bracket's two nodes in float64, with the number of non-zero contributions per node, the largest
    |contribution| and the nodes a near-node look-up may have reached."""
    ref, cnt = np.zeros(n), np.zeros(n)
    big = 0.
    for idx, c in ((b["lo"], v * (1. - b["t"])), (b["lo"] + 1, v * b["t"])):
        np.add.at(ref, idx, c)
        np.add.at(cnt, idx, (c != 0.).astype(np.float64))
        big = max(big, float(np.abs(c).max()))
    keep = np.ones(n, bool)
    for j in range(-1, 3):
        keep[np.clip(b["lo"][near] + j, 0, n - 1)] = False
    return dict(ref=ref, cnt=cnt, m=big, keep=keep)


def lightcone_g_restatement(r0, gB):
    """g_bar alone: the g block and, through a = chi2a(r0) kept in float32, the chi block."""
    T = lc_tables()
    x = r0.astype(np.float64)
    ba = bracket(x, T["chi"], T["aoc"])
    a = np.interp(x, T["chi"], T["aoc"]).astype(np.float32).astype(np.float64)
    bg = bracket(a, T["a"], T["g"])
    gb = gB.astype(np.float64)
    near = ba["near"] | bg["near"]
    return dict(g=scatter(len(T["a"]), bg, gb, near), chi=scatter(len(T["chi"]), ba, -(gb * bg["slope"]) * ba["slope"], near),
                share=float(near.mean()))


def within_bound(tag, got, want, cnt, m, keep=None):
    keep = np.ones(len(got), bool) if keep is None else keep
    err, bound = np.abs(got - want)[keep], (cnt * m * 2. ** -29)[keep]
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{tag}: {int(keep.sum())} of {len(got)} entries, {int((cnt[keep] > 0).sum())} with contributions, m = {m:.3e}, largest error "
          f"{float(err.max()):.3e}, largest error / bound {worst:.3f}")
    assert np.all(err <= bound), (tag, worst)


@pytest.mark.parametrize("N", [N_RAGGED, N_CAPPED])
def test_order_independence(gpu, N):
    """A permutation of the particles leaves every bit of table_bar as it was."""
    import torch
    r0, gB, g2B, dB = lc_inputs(N)
    perm = np.random.default_rng(7).permutation(N)
    base = lc_call(gpu, r0, gB, g2B, dB)
    assert bool(torch.isfinite(base).all()) and int((base != 0).sum()) > 50
    assert torch.equal(base, lc_call(gpu, r0[perm], gB[perm], g2B[perm], dB[perm]))


def test_resolution(gpu):
    """The g and chi blocks of a g_bar-only call against the float64 restatement, entry by entry to c_i m_k 2^-29."""
    T = lc_tables()
    nchi, ng = len(T["chi"]), len(T["a"])
    r0, gB, _, _ = lc_inputs(N_CAPPED)
    R = lightcone_g_restatement(r0, gB)
    print("near-node share", R["share"])
    assert R["share"] <= 1e-3
    got = lc_call(gpu, r0, gB, None, None).cpu().numpy()
    assert not np.any(got[nchi + ng:])
    for k, sl in (("g", slice(nchi, nchi + ng)), ("chi", slice(0, nchi))):
        assert int((R[k]["cnt"][R[k]["keep"]] > 0).sum()) >= 10      # the comparison is not empty (0.45 < a < 0.8 spans 14 growth nodes, 800 < r0 < 2600 21 chi nodes)
        within_bound(f"resolution {k}", got[sl], R[k]["ref"], R[k]["cnt"], R[k]["m"], R[k]["keep"])


def test_zero_and_nonfinite_inputs_leave_nothing_behind(gpu):
    import torch
    r0, gB, g2B, dB = lc_inputs(N_RAGGED)
    base = lc_call(gpu, r0, gB, g2B, dB)
    z = np.zeros_like(gB)
    assert not bool(lc_call(gpu, r0, z, z, z).any())
    bad = g2B.copy()
    bad[N_RAGGED // 2] = np.nan
    assert bool(torch.isnan(lc_call(gpu, r0, gB, bad, dB)).all())      # the documented rule: the whole table
    assert torch.equal(base, lc_call(gpu, r0, gB, g2B, dB))


def test_tables_beyond_the_capacity_are_refused(gpu):
    import torch
    from montecosmo_amd import _lib
    nchi, ng = 3000, 100      # nchi + 4 ngrow = 3400 entries: more than the tables region holds
    tabs = np.concatenate([np.linspace(0., 3000., nchi), np.linspace(0.2, 1., nchi)] + [np.linspace(0.1, 1., ng)] * 5)
    r0, gB, g2B, dB = lc_inputs(N_RAGGED)
    out = torch.full((nchi + 4 * ng,), 7., dtype=torch.float64, device=gpu)
    with pytest.raises(_lib.McpmError, match="failed with code -6: mcpm_lightcone_tables_vjp_f32: tables exceed the accumulators"):
        lc_call(gpu, r0, gB, g2B, dB, tabs=tabs, nchi=nchi, ng=ng, out=out)
    assert bool((out == 7.).all())


PNG_SHAPE, PNG_BOX = (8, 6, 10), (100., 75., 125.)


def png_setup(nt):
    """A transfer table of nt nodes spanning the |k| range of the (8, 6, 10) mesh, a linear field and a generic cotangent."""
    from montecosmo_amd import bricks, power
    cosmo = bricks.Planck18()
    km = pf.kmesh(PNG_SHAPE, PNG_BOX)
    ks = np.geomspace((1. - 1e-4) * km[km > 0].min(), (1. + 1e-4) * km.max(), nt)      # the first and the last bracket are in use
    k0, p0 = power.lin_power_table(cosmo)
    assert k0[0] < ks[0] and ks[-1] < k0[-1]
    kpow = (ks, np.exp(np.interp(np.log(ks), np.log(k0), np.log(p0))))
    rng = np.random.default_rng(31)
    X = np.fft.rfftn(0.4 * rng.standard_normal(PNG_SHAPE))
    X[0, 0, 0] = 0.
    X = X.astype(np.complex64)
    ob = (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)).astype(np.complex64)
    return cosmo, kpow, X, ob, rng


def test_png_table_beyond_the_capacity_is_refused(gpu):
    from montecosmo_amd import _lib, bricks
    cosmo, kpow, X, ob, _ = png_setup(2049)
    _, ctx = bricks.add_png(cosmo, -300., X, PNG_BOX, kpow=kpow, return_ctx=True)
    assert ctx.nt == 2049
    with pytest.raises(_lib.McpmError, match="failed with code -6: mcpm_png_add_vjp_f32: table exceeds the accumulators"):
        bricks.add_png_vjp(ctx, ob)


def test_png_table_at_the_capacity(gpu):
    """ntab = 2048: the maxima sit directly behind the last accumulator.  Bitwise repeatable, and trans_bar against the directional
    differences of test_add_png_vjp (same restatement, same pairing, same 3e-3 gate)."""
    from montecosmo_amd import bricks
    fNL, nt = -300., 2048
    cosmo, kpow, X, ob, rng = png_setup(nt)
    ks, trans = bricks.trans_phi2delta_table(cosmo, kpow=kpow)
    _, ctx = bricks.add_png(cosmo, fNL, X, PNG_BOX, kpow=kpow, return_ctx=True)
    assert ctx.nt == nt
    lb, fb, tb = bricks.add_png_vjp(ctx, ob)
    lb2, fb2, tb2 = bricks.add_png_vjp(ctx, ob)
    assert bool((lb == lb2).all()) and fb == fb2 and np.array_equal(tb, tb2)
    assert tb.shape == (nt,) and np.isfinite(tb).all() and tb[0] != 0. and tb[-1] != 0.      # the last accumulator receives the Nyquist corner mode
    X64, ob64 = X.astype(np.complex128), ob.astype(np.complex128)
    pair = lambda a, b: float((a.real * b.real + a.imag * b.imag).sum())
    L = lambda tr: pair(ob64, pf.add_png((ks, tr), fNL, X64, PNG_BOX))
    eps = 1e-5
    lk = np.log(ks / ks[0]) / np.log(ks[-1] / ks[0])
    for name, dirn in (("tilt", trans * (0.5 + lk)), ("random", trans * rng.standard_normal(nt))):
        fdt = (L(trans + eps * dirn) - L(trans - eps * dirn)) / (2 * eps)
        ant = float((tb * dirn).sum())
        print(f"png table at capacity, {name}: fd {fdt:.6e} an {ant:.6e}")
        assert abs(fdt - ant) < 3e-3 * abs(fdt), (name, fdt, ant)


# geometry of tests/test_gpu_ap.py
EVOL, PAINT = (16, 16, 16), (24, 20, 16)
BOX, CENTER, ROTVEC = (640., 640., 640.), (100., -50., 1500.), (0.2, -0.1, 0.3)


def test_kind_boundaries_one_kind(gpu):
    """mcpm_observe_pos_ap_tables_vjp_f32 off the light cone with MCPM_AP_AUTO: chi_bar[nap] alone (one kind, ngrow = 0).  Bitwise
    repeatable, and equal to the sum of the same call on the two halves of the particles to c_i m 2^-29, c_i and m from a float64
    restatement of the contributions: a_bar = (D_bar . P') / r' d chi_fid / d a into the nodes of the chi -> a look-up at r'.
    The halves alone would not see a wrong kind boundary (a wrong exponent scales the full call and both halves by the same power of two):
    the comparison of the full call with the restatement does, at 1e4 times the bound (the kernel works from float32 positions, 1e-5 of a
    contribution; a wrong exponent is a factor 2 at least).  Keep both.  No look-up of this seed lies within 1e-7 of a node (asserted)."""
    import torch
    from montecosmo_amd import bricks, nbody
    rng = np.random.default_rng(23)
    cosmo, cosmo_fid = bricks.Planck18(Omega_c=0.25 - 0.0490), bricks.Planck18()
    N, a_obs = 16 ** 3, 0.7
    disp = (1.5 * rng.standard_normal((N, 3))).astype(np.float32)
    vel, dvel = (3.0 * rng.standard_normal((N, 3))).astype(np.float32), (0.5 * rng.standard_normal((N, 3))).astype(np.float32)
    pos = nbody.LatticePos(disp, EVOL).to_absolute().cpu().numpy().astype(np.float32)
    ob = rng.standard_normal((N, 3)).astype(np.float32)

    def bar(sl):
        _, ctx = bricks.observe_pos(cosmo, pos[sl], vel[sl], CENTER, ROTVEC, BOX, EVOL, PAINT, a_obs=a_obs, curved_sky=True, dvel=dvel[sl],
                                    return_ctx=True, ap_auto=True, cosmo_fid=cosmo_fid)
        assert not ctx.flags & 2 and ctx.ap_mode == 1
        b, b2 = bricks.observe_pos_tables_vjp(ctx, ob[sl]), bricks.observe_pos_tables_vjp(ctx, ob[sl])
        assert torch.equal(b, b2)
        return b.cpu().numpy()

    full, h0, h1 = bar(slice(None)), bar(slice(0, N // 2)), bar(slice(N // 2, N))
    d, df = nbody._dist_cache(cosmo), nbody._dist_cache(cosmo_fid)
    chi, aoc = d["chi"][::-1].copy(), d["a"][::-1].copy()
    assert full.shape == (len(chi),) and np.isfinite(full).all()
    R = bo.rotvec_matrix(ROTVEC)
    los, Pp = apo.observe_phys(cosmo, pos.astype(np.float64), vel.astype(np.float64), CENTER, R, BOX, EVOL, a_obs, True, dvel.astype(np.float64))
    rp = apo.ap_rpos(Pp, los, True)[:, 0]
    Db = (ob.astype(np.float64) / np.divide(BOX, PAINT)) @ R.T      # D_bar = R (out_bar / cell_p)
    bp = bracket(rp, chi, aoc)
    assert np.minimum(np.abs(rp - chi[bp["lo"]]), np.abs(rp - chi[bp["lo"] + 1])).min() > 1e-7 * rp.max()      # float32 r' takes the same bracket
    sfid = bracket(bp["y"], df["a"], df["chi"])["slope"]
    S = scatter(len(chi), bp, -((Db * Pp).sum(-1) / rp * sfid) * bp["slope"], np.zeros(N, bool))
    assert int((S["cnt"] > 0).sum()) >= 4
    within_bound("one kind: full against the restatement", full, S["ref"], S["cnt"], S["m"] * 1e4)      # float32 inputs of the kernel: a sanity check of c_i, m
    within_bound("one kind: halves", h0 + h1, full, S["cnt"], S["m"])


def test_kind_boundaries_three_kinds(gpu):
    """mcpm_kaiser_sky_tables_vjp_f32 on the curved sky (chi, g, f): bitwise repeatable, and equal to the sum of the same call with
    out_bar zeroed on one and on the other half of the cells, each kind to c_i m_k 2^-29 with c_i, m_k from a float64 restatement of the
    per-cell contributions g_bar = w (b1E d + f q), f_bar = w g q, a_bar = g_bar g' + f_bar f'.
    The halves alone would not see a wrong kind boundary (a wrong exponent scales the full call and both halves by the same power of two):
    the comparison of the full call with the restatement does, at 1e4 times the bound (float32 meshes and distances; a wrong exponent is a
    factor 2 at least).  Keep both.  No look-up of this seed lies within 1e-7 of a node (asserted)."""
    import torch
    from montecosmo_amd import bricks, nbody
    shape, final, cell, b1E = (16, 16, 16), (10, 10, 10), 40., 1.0
    center, rotvec = (60., -40., 1400.), (0.1, 0.2, -0.1)      # tests/test_gpu_kaiser_sky.py
    rng = np.random.default_rng(101)
    cosmo = bricks.Planck18()
    box = np.multiply(final, cell)
    X = np.fft.rfftn(0.4 * rng.standard_normal(shape))
    X[0, 0, 0] = 0.
    lin = X.astype(np.complex64)
    ob = rng.standard_normal(shape).astype(np.float32)
    _, ctx = bricks.kaiser_sky(cosmo, lin, box_size=box, box_center=center, box_rot=rotvec, b1E=b1E, a_obs=None, curved_sky=True, return_ctx=True)
    geom, flags, tables, nchi, ngrow = ctx.args[:5]
    assert flags == 3
    plan = nbody.get_plan(shape)

    def bar(w):
        out = []
        for _ in range(2):
            tb = torch.empty(nchi + 2 * ngrow, dtype=torch.float64, device=gpu)
            plan.call("mcpm_kaiser_sky_tables_vjp_f32", ctx.meshes, geom, flags, tables, nchi, ngrow, b1E, torch.from_numpy(w).to(gpu), tb)
            out.append(tb)
        assert torch.equal(out[0], out[1])
        return out[0].cpu().numpy()

    half = np.arange(ob.size).reshape(shape) < ob.size // 2
    full, h0, h1 = bar(ob), bar(np.where(half, ob, np.float32(0.))), bar(np.where(half, np.float32(0.), ob))
    assert np.isfinite(full).all()
    # restatement
    cfg = dict(box_size=box, box_center=np.array(center), box_rotvec=np.array(rotvec), a_obs=None, curved_sky=True)
    d, gt = nbody._dist_cache(cosmo), nbody._growth_cache(cosmo)
    chi, aoc = d["chi"][::-1].copy(), d["a"][::-1].copy()
    r, l, _, _ = kf.geometry(cfg, None, shape, tables={"chi": chi, "a_chi": aoc, "a": gt["a"], "g": gt["g"], "f": gt["f"]})
    lin64 = lin.astype(np.complex128)
    dlt, q = kf._irfftn(lin64, shape).ravel(), kf.mu2_delta_tensor(lin64, l).ravel()
    ba = bracket(r.ravel(), chi, aoc)
    bg = bracket(ba["y"], gt["a"], gt["g"])
    bf = bracket(ba["y"], gt["a"], gt["f"])
    for x_, b_, xp_ in ((r.ravel(), ba, chi), (ba["y"], bg, gt["a"])):      # the kernel's float32 r takes the same brackets
        assert np.minimum(np.abs(x_ - xp_[b_["lo"]]), np.abs(x_ - xp_[b_["lo"] + 1])).min() > 1e-7 * np.abs(x_).max()
    w = ob.astype(np.float64).ravel()
    gb, fb = w * (b1E * dlt + bf["y"] * q), w * bg["y"] * q
    none = np.zeros(w.size, bool)
    S = {"chi": scatter(nchi, ba, -(gb * bg["slope"] + fb * bf["slope"]) * ba["slope"], none), "g": scatter(ngrow, bg, gb, none),
         "f": scatter(ngrow, bg, fb, none)}
    for k, sl in (("chi", slice(0, nchi)), ("g", slice(nchi, nchi + ngrow)), ("f", slice(nchi + ngrow, nchi + 2 * ngrow))):
        assert int((S[k]["cnt"] > 0).sum()) >= 2
        within_bound(f"three kinds {k}: full against the restatement", full[sl], S[k]["ref"], S[k]["cnt"], S[k]["m"] * 1e4)      # float32 meshes: a sanity check of c_i, m_k
        within_bound(f"three kinds {k}: halves", (h0 + h1)[sl], full[sl], S[k]["cnt"], S[k]["m"])
