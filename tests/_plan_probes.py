"""Probes of tests/test_gpu_plan_history.py: seeded inputs per geometry and one function per operation family, each `(plan, inputs) ->
dict of named numpy arrays` holding every output a caller can see.  A probe never writes to an input (in-place entry points get clones),
so one set of inputs serves every plan of a module.  The nbody / bricks wrappers find their plan in `nbody._PLANS`: `installed(plan, geo)`
puts the plan under test there, so that a probe runs on the plan it was given and on no other."""
import contextlib

import numpy as np

F32 = np.float32
K_STEPS = 3                                          # saved states of the lone step and of the carried chain
WSCALE = float(F32(0.37109375 * 1.0009765625))       # not a power of two (tests/test_gpu_adjoint_carry.py)
BIAS = dict(b1=1.1, b2=0.3, bs2=-0.2, b3=0.15, bds2=0.25, bs3=-0.1, bn2=2.0, bnpar=1.5)      # tests/test_gpu_bias.py
BOX, CENTER, ROTVEC, PAINT = (640., 640., 640.), (100., -50., 1500.), (0.2, -0.1, 0.3), (24, 20, 16)      # tests/test_gpu_ap.py
LIK_N, MCLMC_D = 4099, 65537


class Geo:
    def __init__(self, name, mesh, ptcl, seed):
        self.name, self.mesh, self.ptcl, self.seed = name, tuple(mesh), tuple(ptcl), seed
        self.N, self.M = int(np.prod(ptcl)), int(np.prod(mesh))


# G1: 64^3 is 4 tiles of 16 per axis (tiled_geometry_ok needs 3) and a power of two (mcpm_fftpm_supported): tiled density and
# three-component paints, hand-written FFT / fused Poisson passes, interleaved force meshes, fused steppers.
# G2: lattice != mesh and 24, 12 are no powers of two: generic fixed-point paint, rocFFT, lattice spacings 1.5, 1 and 0.75 cells, the
# lattice_scatter_fx NGP adjoint.
G1 = Geo("G1", (64, 64, 64), (64, 64, 64), 611)
G2 = Geo("G2", (24, 16, 12), (16, 16, 16), 612)
GEOS = (G1, G2)

_COSMO = []


def cosmo():
    if not _COSMO:
        from montecosmo_amd import bricks
        _COSMO.append(bricks.Planck18())
    return _COSMO[0]


def heavy(rng, *shape):
    """Heavy-tailed weights, max|w| / rms|w| ~ 1e3 (tests/test_gpu_parity.py::test_paint3_fixed_point_tiles)."""
    return (rng.standard_normal(shape) * np.exp(1.5 * rng.standard_normal(shape[:1] + (1,) * (len(shape) - 1)))).astype(F32)


class Inputs:
    """h: host float32 / complex64 arrays; d: the same on the device.  Displacements are clipped to |d| <= 3.9 cells: no particle of a probe
    takes a float-atomic path."""

    def __init__(self, geo, dev):
        import torch
        from montecosmo_amd import synth, nbody
        self.geo, self.dev = geo, dev
        N, M, mesh = geo.N, geo.M, geo.mesh
        self.NA = NA = 5003
        rng = np.random.default_rng(geo.seed)
        sn = lambda *s: rng.standard_normal(s).astype(F32)
        h = dict(disp=np.clip(sn(N, 3) * 1.5, -3.9, 3.9).astype(F32), w=heavy(rng, N), w3=heavy(rng, N, 3), mesh=sn(*mesh), mesh3=sn(3, *mesh),
                 ob=sn(N), ob3=sn(N, 3), mb=sn(*mesh), fbar=sn(N, 3), xb=sn(N, 3), vb=sn(N, 3),
                 pos_abs=(rng.uniform(-1., 2., (NA, 3)) * np.array(mesh)).astype(F32), w_abs=heavy(rng, NA), ob_abs=sn(NA), ob3_abs=sn(NA, 3),
                 fbar_abs=sn(NA, 3), spec=synth.init_mesh(mesh, seed=geo.seed, rms_disp=1.0),
                 vel=3.0 * sn(N, 3), dvel=0.5 * sn(N, 3), wbar=sn(N), png_ob=(sn(mesh[0], mesh[1], mesh[2] // 2 + 1)
                                                                              + 1j * sn(mesh[0], mesh[1], mesh[2] // 2 + 1)).astype(np.complex64))
        # the likelihood's cells (tests/test_gpu_reductions_ragged.py::test_lik_real_shash) and the sampler's state (tests/test_gpu_mclmc.py)
        count = rng.uniform(35., 95., LIK_N).astype(F32)
        mask = rng.uniform(size=LIK_N) < 0.8
        obs = np.rint(np.abs(count) + 8. * rng.standard_normal(LIK_N)).clip(0).astype(F32)
        selec = rng.uniform(50., 80., LIK_N).astype(F32)
        obs[~mask], selec[~mask] = np.nan, 0.
        h.update(lik_count=count, lik_obs=obs, lik_selec=selec, lik_mask=mask)
        u = rng.standard_normal(MCLMC_D)
        h.update(mc_u=(u / np.linalg.norm(u)).astype(F32), mc_q=sn(MCLMC_D), mc_g=sn(MCLMC_D) * 3, mc_s=rng.uniform(0.5, 2., MCLMC_D).astype(F32))
        # light-cone tables call (tests/test_gpu_table_sums.py)
        h.update(lc_r0=rng.uniform(800., 2600., 3001).astype(F32), lc_g=sn(3001), lc_g2=sn(3001), lc_d=sn(3001))
        self.h = h
        self.d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in h.items()}
        self.dg, self.alphas, self.betas, self.lpt_s = nbody._step_scalars(cosmo(), 0.1, 1.0, K_STEPS, "bullfrog")
        self._states()

    def _states(self):
        """K_STEPS forward steps on a plan of their own: the saved states (x'_i, v_i) and force meshes that the adjoint-step probes read."""
        import torch
        from montecosmo_amd import nbody
        g, K = self.geo, K_STEPS
        plan = nbody.Plan(g.mesh, g.ptcl)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.sx = [torch.empty((g.N, 3), **f32) for _ in range(K + 1)]
        self.sv = [torch.empty((g.N, 3), **f32) for _ in range(K + 1)]
        self.fm = [torch.empty((3 * g.M,), **f32) for _ in range(K)]
        s = self.lpt_s
        plan.call("mcpm_lpt_f32", self.d["spec"], 2, float(s[0]), float(s[1]), float(s[2]), 0, 0, self.sx[0], self.sv[0])
        plan.call("mcpm_drift_f32", self.sx[0], self.sv[0], g.N, float(self.dg / 2), self.sx[0])
        for i in range(K):
            plan.call("mcpm_bullfrog_step_f32", self.sx[i], self.sv[i], float(self.alphas[i]), float(self.betas[i]), self.tau(i), 2, self.fm[i],
                      self.sx[i + 1], self.sv[i + 1])
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in self.sx + self.sv + self.fm)

    def tau(self, i):
        return float(self.dg / 2 if i == K_STEPS - 1 else self.dg)

    def empty(self, *shape, dtype=None):
        import torch
        return torch.empty(shape, dtype=dtype or torch.float32, device=self.dev)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _keys(geo):
    import torch
    dev, st = torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream
    return {(geo.mesh, geo.ptcl, dev, st), (geo.mesh, geo.mesh, dev, st)}      # the second: wrappers of mesh-only operations (add_png)


@contextlib.contextmanager
def installed(plan, geo):
    """`plan` is what nbody.get_plan returns for the geometry's shapes while the block runs; the cache is empty afterwards."""
    from montecosmo_amd import nbody
    nbody.clear_plans()
    for k in _keys(geo):
        nbody._PLANS[k] = plan
    try:
        assert nbody.get_plan(geo.mesh, geo.ptcl) is plan and nbody.get_plan(geo.mesh) is plan
        yield plan
    finally:
        nbody.clear_plans()


def new_plan(geo):
    from montecosmo_amd import nbody
    nbody.clear_plans()
    return nbody.Plan(geo.mesh, geo.ptcl)


# ---- 1: paint ------------------------------------------------------------------------------------------------------------------------
def paint_cases(I):
    d = I.d
    return [("lat2", d["disp"], I.geo.N, 1, 2, d["w"]), ("abs1", d["pos_abs"], I.NA, 0, 1, d["w_abs"]), ("abs3", d["pos_abs"], I.NA, 0, 3, d["w_abs"])]


def probe_paint(plan, I):
    res = {}
    for tag, pos, n, mode, order, w in paint_cases(I):
        for wt, wtag in ((None, "unit"), (w, "w")):
            for acc in (0, 1):
                mesh = I.d["mesh"].clone() if acc else I.empty(*I.geo.mesh)
                plan.call("mcpm_paint_f32", pos, n, mode, wt, 1, 1.0 if wt is None else 0.0, order, mesh, acc)
                res[f"{tag}-{wtag}-acc{acc}"] = _np(mesh)
    return res


# ---- 2: three-component paint --------------------------------------------------------------------------------------------------------
def probe_paint3(plan, I):
    d, g, res = I.d, I.geo, {}
    for acc in (0, 1):
        out = d["mesh3"].clone() if acc else I.empty(3, *g.mesh)
        plan.call("mcpm_paint3_f32", d["disp"], g.N, 1, d["w3"], 2, out, acc)
        res[f"plain-acc{acc}"] = _np(out)
        out = d["mesh3"].clone() if acc else I.empty(3, *g.mesh)
        plan.call("mcpm_paint3_scaled_f32", d["disp"], g.N, 1, d["w3"], WSCALE, 2, out, acc)
        res[f"scaled-acc{acc}"] = _np(out)
    res["scaled-beta0"] = _np(paint3_beta0(plan, I, d["w3"]))
    return res


def paint3_beta0(plan, I, w3):
    """The weights w3 scaled by beta_0, the scale a finished carried chain last announced a weight maximum for."""
    out = I.empty(3, *I.geo.mesh)
    plan.call("mcpm_paint3_scaled_f32", I.d["disp"], I.geo.N, 1, w3, float(I.betas[0]), 2, out, 0)
    return out


# ---- 3: read, read_vjp, paint_vjp ------------------------------------------------------------------------------------------------------
def probe_read(plan, I):
    d, g, res = I.d, I.geo, {}
    for tag, pos, n, mode, order in (("lat2", d["disp"], g.N, 1, 2), ("abs3", d["pos_abs"], I.NA, 0, 3), ("abs1", d["pos_abs"], I.NA, 0, 1)):
        o1, o3 = I.empty(n), I.empty(n, 3)
        plan.call("mcpm_read_f32", pos, n, mode, d["mesh"], 1, order, o1)
        plan.call("mcpm_read_f32", pos, n, mode, d["mesh3"], 3, order, o3)
        res[f"read1-{tag}"], res[f"read3-{tag}"] = _np(o1), _np(o3)
    # read_vjp: positions (one and three components) and the mesh (a weighted paint)
    pb = I.empty(g.N, 3)
    plan.call("mcpm_read_vjp_pos_f32", d["disp"], g.N, 1, d["mesh3"], 3, 2, d["ob3"], pb)
    res["read_vjp-pos3-lat2"] = _np(pb)
    pb, mbar = I.empty(g.N, 3), I.empty(*g.mesh)
    plan.call("mcpm_read_vjp_pos_f32", d["disp"], g.N, 1, d["mesh"], 1, 2, d["ob"], pb)
    plan.call("mcpm_paint_f32", d["disp"], g.N, 1, d["ob"], 1, 0.0, 2, mbar, 0)
    res["read_vjp-pos1-lat2"], res["read_vjp-mesh-lat2"] = _np(pb), _np(mbar)
    pb, mbar = I.empty(I.NA, 3), I.empty(*g.mesh)
    plan.call("mcpm_read_vjp_pos_f32", d["pos_abs"], I.NA, 0, d["mesh"], 1, 3, d["ob_abs"], pb)
    plan.call("mcpm_paint_f32", d["pos_abs"], I.NA, 0, d["ob_abs"], 1, 0.0, 3, mbar, 0)
    res["read_vjp-pos1-abs3"], res["read_vjp-mesh-abs3"] = _np(pb), _np(mbar)
    # paint_vjp: weighted in lattice mode, unit weights in absolute mode
    pb, wb = I.empty(g.N, 3), I.empty(g.N)
    plan.call("mcpm_paint_vjp_f32", d["disp"], g.N, 1, d["w"], 1, 0.0, 2, d["mb"], pb, wb)
    res["paint_vjp-pos-lat2"], res["paint_vjp-w-lat2"] = _np(pb), _np(wb)
    pb, wb = I.empty(I.NA, 3), I.empty(I.NA)
    plan.call("mcpm_paint_vjp_f32", d["pos_abs"], I.NA, 0, None, 1, 1.0, 3, d["mb"], pb, wb)
    res["paint_vjp-pos-abs3"], res["paint_vjp-w-abs3"] = _np(pb), _np(wb)
    return res


# ---- 4: pm_forces and pm_forces_vjp ------------------------------------------------------------------------------------------------------
def probe_forces(plan, I):
    import torch
    d, g, res = I.d, I.geo, {}
    f = I.empty(g.N, 3)
    plan.call("mcpm_pm_forces_f32", d["disp"], g.N, 1, 2, 0, 0, 0, 0.0, f)
    res["painted-lat2"] = _np(f)
    f = I.empty(I.NA, 3)
    plan.call("mcpm_pm_forces_spec_f32", d["spec"], d["pos_abs"], I.NA, 0, 2, 0, 0, 0.0, f)
    res["spec-abs2"] = _np(f)
    pb = I.empty(g.N, 3)
    plan.call("mcpm_pm_forces_vjp_f32", None, d["disp"], g.N, 1, 2, d["fbar"], pb, None)
    res["vjp-painted-lat2"] = _np(pb)
    pb, sb = I.empty(I.NA, 3), torch.empty_like(d["spec"])
    plan.call("mcpm_pm_forces_vjp_f32", d["spec"], d["pos_abs"], I.NA, 0, 2, d["fbar_abs"], pb, sb)
    res["vjp-spec-pos-abs2"], res["vjp-spec-mesh-abs2"] = _np(pb), _np(sb)
    return res


# ---- 5, 6: lpt, nbody_bf through the wrappers ------------------------------------------------------------------------------------------
LPT_A, NBODY_A0 = 0.5, 0.1


def probe_lpt(plan, I):
    from montecosmo_amd import nbody
    d, g = I.d, I.geo
    lp0 = nbody.LatticePos.regular(g.mesh, g.ptcl)
    dpos, vel = nbody.lpt(cosmo(), d["spec"], lp0, a=LPT_A, lpt_order=2, read_order=1)
    mb, sb = nbody.lpt_vjp(cosmo(), d["spec"], lp0, LPT_A, d["xb"], d["vb"], lpt_order=2)
    return dict(dpos=_np(dpos), vel=_np(vel), init_mesh_bar=_np(mb), scalar_bars=np.array([sb["g"], sb["g2"], sb["dg2dg"]]))


def nbody_sweep(plan, I, n_steps):
    from montecosmo_amd import nbody
    d, g = I.d, I.geo
    lp0 = nbody.LatticePos.regular(g.mesh, g.ptcl)
    (lp, vel), ctx = nbody.nbody_bf(cosmo(), d["spec"], lp0, a0=NBODY_A0, a1=1., n_steps=n_steps, return_ctx=True, lattice_out=True)
    assert ctx.plan is plan
    mb, sb = nbody.nbody_bf_vjp(ctx, d["xb"], d["vb"])
    return dict(pos=_np(lp.disp), vel=_np(vel), init_mesh_bar=_np(mb), alpha_bar=sb["alpha"], beta_bar=sb["beta"],
                scalar_bars=np.array([sb["g"], sb["g2"], sb["dg2dg"], sb["dg"]]))


def probe_nbody3(plan, I):
    return nbody_sweep(plan, I, 3)


def probe_nbody1(plan, I):
    return nbody_sweep(plan, I, 1)


# ---- 7, 8: adjoint steps on the saved states -------------------------------------------------------------------------------------------
def probe_lone_step(plan, I):
    """One unhinted mcpm_bullfrog_step_vjp_f32 (in place) on the last saved state."""
    import torch
    i = K_STEPS - 1
    xb, vb = I.d["xb"].clone(), I.d["vb"].clone()
    sbar = torch.zeros(3, dtype=torch.float64, device=I.dev)
    plan.call("mcpm_bullfrog_step_vjp_f32", I.sx[i], I.sv[i], I.fm[i], float(I.alphas[i]), float(I.betas[i]), I.tau(i), 2, xb, vb,
              sbar[0:1], sbar[1:2], 0.5, sbar[2:3])
    s = _np(sbar)
    return dict(x_bar=_np(xb), v_bar=_np(vb), alpha_bar=s[0:1], beta_bar=s[1:2], dg_bar=s[2:3])


def chain_step(plan, I, i, src_x, src_v, xb, vb, sbar, hint):
    K = K_STEPS
    if hint:
        plan.call("mcpm_plan_hint_next_adjoint", float(I.betas[i - 1]), float(I.dg))
    plan.call("mcpm_bullfrog_step_vjp_from_f32", I.sx[i], I.sv[i], I.fm[i], float(I.alphas[i]), float(I.betas[i]), I.tau(i), 2, src_x, src_v,
              xb, vb, sbar[i:i + 1], sbar[K + i:K + i + 1], 0.5 if i == K - 1 else 1.0, sbar[2 * K:2 * K + 1])


def probe_chain3(plan, I):
    """The carried chain of K_STEPS steps, as bench.py issues it: the first step reads the loss cotangents where they are."""
    import torch
    K, g = K_STEPS, I.geo
    xb, vb = I.empty(g.N, 3), I.empty(g.N, 3)
    sbar = torch.zeros(2 * K + 1, dtype=torch.float64, device=I.dev)
    for i in reversed(range(K)):
        first = i == K - 1
        chain_step(plan, I, i, I.d["xb"] if first else xb, I.d["vb"] if first else vb, xb, vb, sbar, hint=i > 0)
    return dict(x_bar=_np(xb), v_bar=_np(vb), scalar_bars=_np(sbar))


# ---- 9: plan-resident reductions of the model side ---------------------------------------------------------------------------------------
def probe_lik(plan, I):
    import torch
    from montecosmo_amd import _lib
    d, n = I.d, LIK_N
    cb, qb, sums = I.empty(n), I.empty(n), I.empty(5, dtype=torch.float64)
    plan.call("mcpm_lik_real_f32", _lib.LIK_SHASH, n, d["lik_obs"], d["lik_count"], d["lik_selec"], 1.0, d["lik_mask"], float(F32(0.9)),
              float(F32(0.4)), float(F32(-0.08)), cb, qb, sums)
    return dict(count_bar=_np(cb), sqsel_bar=_np(qb), sums=_np(sums))


def mclmc_call(plan, I, u, q, g, s, dsize):
    import torch
    stats = torch.tensor([7., 7., 7., 0.25], dtype=torch.float64, device=I.dev)
    plan.call("mcpm_mclmc_kick_drift_f32", u, q, g, s, dsize, 0.37, 0.21, stats)
    return stats


def probe_mclmc(plan, I):
    d = I.d
    u, q = d["mc_u"].clone(), d["mc_q"].clone()
    stats = mclmc_call(plan, I, u, q, d["mc_g"], d["mc_s"], MCLMC_D)
    return dict(u=_np(u), q=_np(q), stats=_np(stats))


def lc_tables():
    from montecosmo_amd import nbody
    dc, gt = nbody._dist_cache(cosmo()), nbody._growth_cache(cosmo())
    tabs = np.concatenate([dc["chi"][::-1], dc["a"][::-1]] + [gt[k] for k in ("a", "g", "g2", "f", "f2")])
    return tabs, len(dc["chi"]), len(gt["a"])


def lc_call(plan, I, tabs, nchi, ng):
    import torch
    d = I.d
    out = I.empty(nchi + 4 * ng, dtype=torch.float64)
    plan.call("mcpm_lightcone_tables_vjp_f32", d["lc_r0"], 3001, torch.from_numpy(np.ascontiguousarray(tabs)).to(I.dev), nchi, ng, d["lc_g"],
              d["lc_g2"], d["lc_d"], out)
    return out


def probe_lc_tables(plan, I):
    return dict(table_bar=_np(lc_call(plan, I, *lc_tables())))


def probe_observe(plan, I):
    from montecosmo_amd import bricks, nbody
    d, g = I.d, I.geo
    lp = nbody.LatticePos(d["disp"], g.mesh, g.ptcl)
    out, ctx = bricks.observe_pos(cosmo(), lp, d["vel"], CENTER, ROTVEC, BOX, g.mesh, PAINT, a_obs=0.7, curved_sky=False, dvel=d["dvel"],
                                  return_ctx=True)
    assert ctx.plan is plan
    pb, vb, db, gf = bricks.observe_pos_vjp(ctx, d["ob3"])
    return dict(out=_np(out.disp), pos_bar=_np(pb), vel_bar=_np(vb), dvel_bar=_np(db), gf_bar=np.array([gf]))


def probe_observe_tables(plan, I):
    from montecosmo_amd import bricks, nbody
    d, g = I.d, I.geo
    lp = nbody.LatticePos(d["disp"], g.mesh, g.ptcl)
    out, ctx = bricks.observe_pos(cosmo(), lp, d["vel"], CENTER, ROTVEC, BOX, g.mesh, PAINT, a_obs=None, curved_sky=True, dvel=d["dvel"],
                                  return_ctx=True)
    assert ctx.plan is plan and ctx.flags & 2
    return dict(out=_np(out.disp), table_bar=_np(bricks.observe_pos_tables_vjp(ctx, d["ob3"])))


def probe_bias(plan, I):
    from montecosmo_amd import bricks, nbody
    d, g = I.d, I.geo
    lp = nbody.LatticePos(d["disp"], g.mesh, g.ptcl)
    (w, dvel, _), ctx = bricks.lagrangian_bias(cosmo(), lp, 0.7, BOX, d["spec"], BIAS, read_order=2, return_ctx=True)
    assert ctx.plan is plan
    mb, bias_bar, gbar = bricks.lagrangian_bias_vjp(ctx, d["wbar"], d["fbar"])
    return dict(weights=_np(w), dvel=_np(dvel), lin_mesh_bar=_np(mb), bias_bar=np.array([bias_bar[k] for k in bricks.BIAS_KEYS]),
                growth_bar=np.asarray(gbar, dtype=np.float64).reshape(-1))


def probe_png(plan, I):
    from montecosmo_amd import bricks
    d = I.d
    out, ctx = bricks.add_png(cosmo(), -300., d["spec"], BOX, return_ctx=True)
    assert ctx.plan is plan
    lb, fb, tb = bricks.add_png_vjp(ctx, d["png_ob"])
    return dict(out=_np(out), lin_mesh_bar=_np(lb), fNL_bar=np.array([fb]), trans_bar=tb)


COMMON = dict(paint=probe_paint, paint3=probe_paint3, read=probe_read, forces=probe_forces, lpt=probe_lpt, nbody3=probe_nbody3,
              nbody1=probe_nbody1, lone_step=probe_lone_step, chain3=probe_chain3, lik=probe_lik, mclmc=probe_mclmc, lc_tables=probe_lc_tables)
MODEL = dict(observe=probe_observe, observe_tables=probe_observe_tables, bias=probe_bias, png=probe_png)      # G2-sized, through the wrappers
PROBES = {"G1": dict(COMMON), "G2": dict(COMMON, **MODEL)}
# the sweeps, the adjoint steps and the plan-resident reductions: what runs after a battery of refused calls
ADJOINT = ("nbody3", "nbody1", "lone_step", "chain3", "lik", "mclmc", "lc_tables", "observe", "observe_tables", "bias", "png")


def names(geo):
    return list(PROBES[geo.name])


def run(plan, I, which):
    """The named probes, in the order given, on one plan."""
    out = {}
    with installed(plan, I.geo):
        for name in which:
            out[name] = PROBES[I.geo.name][name](plan, I)
    return out


def run_fresh(I, name):
    """One probe on a brand-new plan."""
    plan = new_plan(I.geo)
    return run(plan, I, [name])[name]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differences(want, got, tag=""):
    """['probe/output: largest |difference|', ...] of every output that is not bit for bit what `want` holds."""
    bad = []
    for name, outs in got.items():
        assert set(outs) == set(want[name]), (name, set(outs) ^ set(want[name]))
        for k, v in outs.items():
            if not same_bits(want[name][k], v):
                w = np.asarray(want[name][k])
                with np.errstate(all="ignore"):
                    dmax = float(np.nanmax(np.abs(np.asarray(v).astype(np.complex128) - w.astype(np.complex128)))) if w.shape == np.shape(v) else np.nan
                bad.append(f"{tag}{name}/{k}: max |diff| {dmax:.3e} of max |value| {float(np.nanmax(np.abs(w))):.3e}")
    return bad
