"""A call's result is a function of its arguments, not of what its mcpm_plan did before.

The plan carries state from call to call (integer accumulators kept zero by a flush kernel, weight maxima keyed by a pointer, redo and tile
lists, the scratch and the ticket of the deterministic sums, the regions of plan->reduce, the hint / carry / fb machine of the reverse sweep,
scratch meshes, settings), and nbody._PLANS keeps one plan per shape for the life of a process.  Here every probe of tests/_plan_probes.py
(each reads back every output a caller can see) is run once on a brand-new plan -- the FRESH value, anchored to the float64 oracle -- and then
again on ONE plan per geometry after histories that exercise that state: other probes in any order, calls that fail their argument checks,
non-finite and degenerate inputs, abandoned chains, settings changed and restored, larger reductions.  Every output must come back bit for bit.

Geometries: G1 = 64^3 (tiled paints: four tiles per axis where tiled_geometry_ok asks for three; powers of two, so mcpm_fftpm_supported: the
hand-written FFT, interleaved force meshes, fused steppers) and G2 = mesh (24, 16, 12) with lattice (16, 16, 16) (generic fixed-point paint,
rocFFT, non-integer lattice spacing, lattice_scatter_fx).

What the file caught when it was written: a hint (mcpm_plan_hint_next_adjoint) outlived the adjoint step it was meant for when that step
failed its argument checks, and was consumed by the next unchained step -- a lone mcpm_bullfrog_step_vjp_f32, or step 0 of a one-step
mcpm_nbody_bf_vjp_f32, whose init_mesh_bar was then off by 0.07 where its largest entry is 0.12, without an error (test_after_error_returns,
test_after_abandoned_chains).  Local mutants that these tests turn red: the flush of the generic paint no longer zeroing its accumulator
(every test but the control); mcpm_paint3_tiled no longer forgetting the array it had a weight maximum for (test_after_abandoned_chains);
the hint rule reverted (test_after_error_returns, test_after_abandoned_chains).  One mutant no test can see: mcpm_nbody_bf_vjp_f32 without
its `fb_valid = 0` at entry -- every step of the sweep clears that flag itself before anything reads it, so the statement is redundant.  Measured on an MI355X: 4.3 s for the fixture (inputs, saved
states, 28 fresh plans), 0.3 s or less for each test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _plan_probes as P  # noqa: E402
from oracle import pm_oracle as o, background as obg  # noqa: E402  (checker only)

F32 = np.float32


class Env:
    pass


@pytest.fixture(scope="module")
def env(gpu):
    """Inputs of both geometries and the fresh value of every probe: one new plan per probe, computed once and left unchanged."""
    from montecosmo_amd import nbody
    E = Env()
    E.inputs = {g.name: P.Inputs(g, gpu) for g in P.GEOS}
    E.fresh = {g.name: {name: P.run_fresh(E.inputs[g.name], name) for name in P.names(g)} for g in P.GEOS}
    yield E
    nbody.clear_plans()


def history(env, before=None, which=None, order=None):
    """On ONE new plan per geometry: `before(plan, inputs)`, then the probes `which` (default: all) in `order` (a permutation of their
    indices); -> the outputs that differ from the fresh ones."""
    bad = []
    for g in P.GEOS:
        I = env.inputs[g.name]
        plan = P.new_plan(g)
        keep = before(plan, I) if before else None      # (arrays that a pending carry refers to stay allocated until the end)
        todo = [n for n in P.names(g) if which is None or n in which]
        if order is not None:
            todo = [todo[i] for i in order(len(todo))]
        bad += P.differences(env.fresh[g.name], P.run(plan, I, todo), tag=g.name + ":")
        del keep
    return bad


# ---- the fresh values themselves -------------------------------------------------------------------------------------------------------
def test_control_two_fresh_plans_agree(env):
    """Every probe on a second, independent new plan: the project's determinism claim (integer sums, fixed-order folds), bit for bit -- the
    probes that run rocFFT on G2 included."""
    bad = []
    for g in P.GEOS:
        again = {name: P.run_fresh(env.inputs[g.name], name) for name in P.names(g)}
        bad += P.differences(env.fresh[g.name], again, tag=g.name + ":")
        for name, outs in env.fresh[g.name].items():      # (all zeros, or a NaN, would equal anything alike)
            bad += [f"{g.name}:{name}/{k}: not finite or all zero" for k, v in outs.items() if not (np.isfinite(v).all() and np.any(v != 0))]
    assert not bad, bad


def rel_l2(a, b):
    a, b = np.asarray(a), np.asarray(b)
    dt = np.complex128 if (np.iscomplexobj(a) or np.iscomplexobj(b)) else np.float64
    a, b = a.astype(dt), b.astype(dt)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_fresh_results_match_the_oracle(env):
    """G2, probes 1, 3, 4, 5 and 6 against oracle.pm_oracle in float64, at the tolerances tests/test_gpu_parity.py holds the same operation to
    (paint, read 2e-6: test_paint_read_absolute, test_generic_paint_is_order_independent; read_vjp, paint_vjp 1e-5: test_paint_read_vjp;
    pm_forces 1e-5: test_pm_forces_painted_and_pm_forces2; pm_forces_vjp 2e-5: test_pm_forces_vjp; lpt 1e-5: test_lpt; lpt_vjp 1e-5 and
    rtol 1e-4: test_lpt_vjp_standalone; nbody_bf 1e-5, its gradient 1e-4: test_nbody_bf_particle_lattice_differs_from_mesh; the scalar
    cotangents of the sweep: test_nbody_bf_vjp).  So "equal to fresh" cannot mean "consistently wrong"."""
    g, I, F = P.G2, env.inputs["G2"], env.fresh["G2"]
    h = {k: (v.astype(np.complex128) if np.iscomplexobj(v) else v.astype(np.float64)) for k, v in I.h.items() if v.dtype != bool}
    q = o.regular_pos(g.mesh, g.ptcl)
    qi = np.floor(q)      # non-integer lattice spacing: the kernels add the lattice point's fraction and the displacement in float32
    lat = qi + ((q - qi).astype(F32) + I.h["disp"]).astype(np.float64)
    errs = []

    def gate(tag, got, want, tol):
        e = rel_l2(got, want)
        print(f"ERR {tag} {e:.3e} gate {tol:.1e}")
        if not e < tol:
            errs.append((tag, e, tol))

    cases = {"lat2": (lat, h["w"], 2), "abs1": (h["pos_abs"], h["w_abs"], 1), "abs3": (h["pos_abs"], h["w_abs"], 3)}
    for tag, (pos, w, order) in cases.items():
        for wtag, wt in (("unit", 1.0), ("w", w)):
            ref = o.paint(pos, g.mesh, wt, order)
            gate(f"paint {tag}-{wtag}-acc0", F["paint"][f"{tag}-{wtag}-acc0"], ref, 2e-6)
            gate(f"paint {tag}-{wtag}-acc1", F["paint"][f"{tag}-{wtag}-acc1"], ref + h["mesh"], 2e-6)
    for tag, pos, order in (("lat2", lat, 2), ("abs3", h["pos_abs"], 3), ("abs1", h["pos_abs"], 1)):
        gate(f"read1 {tag}", F["read"][f"read1-{tag}"], o.read(pos, h["mesh"], order), 2e-6)
        gate(f"read3 {tag}", F["read"][f"read3-{tag}"], np.stack([o.read(pos, h["mesh3"][c], order) for c in range(3)], -1), 2e-6)
    gate("read_vjp pos3 lat2", F["read"]["read_vjp-pos3-lat2"], sum(o.read_vjp(lat, h["mesh3"][c], h["ob3"][:, c], 2)[0] for c in range(3)), 1e-5)
    pb, mb = o.read_vjp(lat, h["mesh"], h["ob"], 2)
    gate("read_vjp pos1 lat2", F["read"]["read_vjp-pos1-lat2"], pb, 1e-5)
    gate("read_vjp mesh lat2", F["read"]["read_vjp-mesh-lat2"], mb, 1e-5)
    pb, mb = o.read_vjp(h["pos_abs"], h["mesh"], h["ob_abs"], 3)
    gate("read_vjp pos1 abs3", F["read"]["read_vjp-pos1-abs3"], pb, 1e-5)
    gate("read_vjp mesh abs3", F["read"]["read_vjp-mesh-abs3"], mb, 1e-5)
    pb, wb = o.paint_vjp(lat, g.mesh, h["w"], h["mb"], 2)
    gate("paint_vjp pos lat2", F["read"]["paint_vjp-pos-lat2"], pb, 1e-5)
    gate("paint_vjp w lat2", F["read"]["paint_vjp-w-lat2"], wb, 1e-5)
    pb, wb = o.paint_vjp(h["pos_abs"], g.mesh, np.ones(I.NA), h["mb"], 3)
    gate("paint_vjp pos abs3", F["read"]["paint_vjp-pos-abs3"], pb, 1e-5)
    gate("paint_vjp w abs3", F["read"]["paint_vjp-w-abs3"], wb, 1e-5)
    gate("pm_forces painted", F["forces"]["painted-lat2"], o.pm_forces(lat, g.mesh, 2), 1e-5)
    gate("pm_forces spec", F["forces"]["spec-abs2"], o.pm_forces(h["pos_abs"], h["spec"], 2), 1e-5)
    gate("pm_forces_vjp painted", F["forces"]["vjp-painted-lat2"], o.pm_forces_vjp(lat, g.mesh, h["fbar"])[0], 2e-5)
    pb, mb = o.pm_forces_vjp(h["pos_abs"], h["spec"], h["fbar_abs"])
    gate("pm_forces_vjp spec pos", F["forces"]["vjp-spec-pos-abs2"], pb, 2e-5)
    gate("pm_forces_vjp spec mesh", F["forces"]["vjp-spec-mesh-abs2"], mb, 2e-5)
    cos_o = obg.Planck18()
    dpos, vel = o.lpt(cos_o, h["spec"], q, P.LPT_A, lpt_order=2, read_order=1)
    gate("lpt dpos", F["lpt"]["dpos"], dpos, 1e-5)
    gate("lpt vel", F["lpt"]["vel"], vel, 1e-5)
    mb, _, sb = o.lpt_vjp(cos_o, h["spec"], q, P.LPT_A, h["xb"], h["vb"], lpt_order=2, read_order=1)
    gate("lpt_vjp mesh", F["lpt"]["init_mesh_bar"], mb, 1e-5)
    for i, k in enumerate(("g", "g2", "dg2dg")):
        if not np.isclose(F["lpt"]["scalar_bars"][i], sb[k], rtol=1e-4, atol=1e-4 * abs(sb["g"])):
            errs.append(("lpt_vjp " + k, F["lpt"]["scalar_bars"][i], sb[k]))
    for n_steps in (3, 1):
        got = F[f"nbody{n_steps}"]
        p_o, v_o = o.nbody_bf(cos_o, h["spec"], q, P.NBODY_A0, 1., n_steps)
        gate(f"nbody{n_steps} pos", got["pos"], p_o[0] - q, 1e-5)
        gate(f"nbody{n_steps} vel", got["vel"], v_o[0], 1e-5)
        mb, sb = o.nbody_bf_vjp(cos_o, h["spec"], q, h["xb"], h["vb"], P.NBODY_A0, 1., n_steps)
        gate(f"nbody{n_steps} init_mesh_bar", got["init_mesh_bar"], mb, 1e-4)
        for k in ("alpha", "beta"):
            if not np.allclose(got[k + "_bar"], sb[k], rtol=2e-4, atol=1e-3 * np.abs(sb[k]).max()):
                errs.append((f"nbody{n_steps} {k}_bar", got[k + "_bar"], sb[k]))
        for i, k in enumerate(("g", "g2", "dg2dg")):
            if not np.isclose(got["scalar_bars"][i], sb[k], rtol=1e-3, atol=1e-3 * abs(sb["g"])):
                errs.append((f"nbody{n_steps} {k}_bar", got["scalar_bars"][i], sb[k]))
    assert not errs, errs


# ---- histories ---------------------------------------------------------------------------------------------------------------------------
def _orders():
    """Six seeded permutations of the probe list, and the list reversed."""
    perms = [lambda n, s=s: list(np.random.default_rng(9000 + s).permutation(n)) for s in range(6)]
    return perms + [lambda n: list(range(n))[::-1]]


@pytest.mark.parametrize("perm", range(7), ids=[f"seed{s}" for s in range(6)] + ["reversed"])
def test_any_order(env, perm):
    """The full probe list end to end on one plan per geometry, in a permuted order: every output equal to its fresh value."""
    bad = history(env, order=_orders()[perm])
    assert not bad, bad


def _raises(plan, name, *args):
    from montecosmo_amd._lib import McpmError
    with pytest.raises(McpmError):
        plan.call(name, *args)


def _errors(plan, I):
    """Calls that fail the host-side argument checks: each raises McpmError before any launch."""
    import torch
    d, g = I.d, I.geo
    mesh, mesh3, out = torch.full(g.mesh, 7., device=I.dev), torch.full((3,) + g.mesh, 7., device=I.dev), torch.full((g.N, 3), 7., device=I.dev)
    _raises(plan, "mcpm_paint_f32", None, g.N, 1, None, 1, 1.0, 2, mesh, 0)                          # null particles
    _raises(plan, "mcpm_paint_f32", d["disp"], g.N, 1, None, 1, 1.0, 2, None, 0)                     # null mesh
    _raises(plan, "mcpm_paint_f32", d["disp"], g.N, 1, None, 1, 1.0, 5, mesh, 0)                     # order 5
    _raises(plan, "mcpm_paint_f32", d["disp"][:-1], g.N - 1, 1, None, 1, 1.0, 2, mesh, 0)            # lattice mode, n != Np
    _raises(plan, "mcpm_paint_f32", d["disp"], g.N, 1, d["w"], 0, 0.0, 2, mesh, 0)                   # wstride 0
    _raises(plan, "mcpm_paint3_f32", d["disp"], g.N, 1, None, 2, mesh3, 0)                           # null weights
    _raises(plan, "mcpm_paint3_scaled_f32", d["disp"], g.N, 1, d["w3"], P.WSCALE, 5, mesh3, 0)
    _raises(plan, "mcpm_read_f32", d["disp"], g.N, 1, None, 3, 2, out)
    _raises(plan, "mcpm_pm_forces_vjp_f32", None, d["disp"], g.N, 1, 2, None, out, None)
    x, v, sb = torch.full((g.N, 3), 7., device=I.dev), torch.full((g.N, 3), 7., device=I.dev), np.full(4, 7.)
    mbar = torch.full_like(d["spec"], 7.)
    _raises(plan, "mcpm_nbody_bf_f32", d["spec"], 0, I.alphas, I.betas, float(I.dg), I.lpt_s, 2, 2, x, v, None)               # n_steps 0
    _raises(plan, "mcpm_nbody_bf_vjp_f32", d["spec"], 0, I.alphas, I.betas, float(I.dg), I.lpt_s, 2, 2, I.sx[0], d["xb"], d["vb"], mbar, sb)
    _raises(plan, "mcpm_lpt_vjp_f32", d["spec"], 3, I.lpt_s, d["xb"], d["vb"], mbar, sb[:3].copy())
    nchi, ng = 3000, 100      # 3400 entries: more than the tables region of plan->reduce holds (tests/test_gpu_table_sums.py)
    tabs = np.concatenate([np.linspace(0., 3000., nchi), np.linspace(0.2, 1., nchi)] + [np.linspace(0.1, 1., ng)] * 5)
    from montecosmo_amd._lib import McpmError
    with pytest.raises(McpmError, match="tables exceed the accumulators"):
        P.lc_call(plan, I, tabs, nchi, ng)
    u8, stats = torch.ones(8, device=I.dev), torch.zeros(4, dtype=torch.float64, device=I.dev)
    _raises(plan, "mcpm_mclmc_kick_drift_f32", u8, None, u8.clone(), None, 1, 0.1, 0.1, stats)       # d = 1
    # a hint, then the adjoint step it was meant for fails its checks (null force_meshes): the hint must not outlive that call
    i = P.K_STEPS - 1
    xb, vb = d["xb"].clone(), d["vb"].clone()
    plan.call("mcpm_plan_hint_next_adjoint", float(I.betas[i - 1]), float(I.dg))
    _raises(plan, "mcpm_bullfrog_step_vjp_from_f32", I.sx[i], I.sv[i], None, float(I.alphas[i]), float(I.betas[i]), I.tau(i), 2, xb, vb, xb, vb,
            None, None, 0.5, None)
    torch.cuda.synchronize()
    for t in (mesh, mesh3, out, x, v):      # nothing was launched
        assert bool((t == 7.).all())
    assert bool((mbar == 7.).all()) and np.all(sb == 7.) and float(stats.abs().sum()) == 0. and torch.equal(xb, d["xb"]) and torch.equal(vb, d["vb"])


def test_after_error_returns(env):
    """A battery of refused calls, the last of them a hinted adjoint step, then probes 6 (both n_steps), 7, 8 and 9.  The battery runs
    three times: before a one-step sweep, before a lone step (the two calls that a hint left pending would spoil: a three-step sweep sets
    the same hint itself and would hide it) and before the list."""
    seen = {}

    def before(plan, I):
        _errors(plan, I)
        seen[I.geo.name] = P.run(plan, I, ["nbody1"])
        _errors(plan, I)
        seen[I.geo.name].update(P.run(plan, I, ["lone_step"]))
        _errors(plan, I)

    bad = history(env, before=before, which=P.ADJOINT)
    for g in P.GEOS:
        bad += P.differences(env.fresh[g.name], seen[g.name], tag=g.name + ":right after the errors:")
    assert not bad, bad


def _paints(plan, I, disp, w, w3, n=None):
    """Generic paint (absolute mode), density paint and three-component paint in lattice mode (tiled on G1), the latter fixed point and f64."""
    g, d = I.geo, I.d
    mesh, mesh3 = I.empty(*g.mesh), I.empty(3, *g.mesh)
    if w is not None:
        plan.call("mcpm_paint_f32", d["pos_abs"][:g.N], min(I.NA, g.N), 0, w, 1, 0.0, 2, mesh, 0)
    plan.call("mcpm_paint_f32", disp, g.N, 1, w, 1, 1.0 if w is None else 0.0, 2, mesh, 0)
    if w3 is not None:
        plan.call("mcpm_paint3_f32", disp, g.N, 1, w3, 2, mesh3, 0)
        plan.call("mcpm_paint3_scaled_f32", disp, g.N, 1, w3, P.WSCALE, 2, mesh3, 1)
    return mesh, mesh3


def _non_finite(plan, I):
    import torch
    g, d = I.geo, I.d
    N = g.N
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(I.dev)
    for bad in (np.nan, np.inf):
        w, w3 = I.h["w"].copy(), I.h["w3"].copy()
        w[N // 3], w3[N // 5, 1] = bad, bad
        mesh, mesh3 = _paints(plan, I, d["disp"], t(w), t(w3))
        assert not bool(torch.isfinite(mesh).all()) and not bool(torch.isfinite(mesh3).all())      # the value reached the mesh
    mesh, mesh3 = _paints(plan, I, d["disp"], t(np.zeros(N)), t(np.zeros((N, 3))))
    assert not bool(mesh.any()) and not bool(mesh3.any())
    # tests/test_gpu_parity.py::test_paint_non_finite_displacement_is_visible
    # (64^3 only, the density paint only: there the tile kernels hand such a particle to the leftover kernel, which names no cell with it;
    # the generic paint of G2 takes positions in the documented range |pos| < 32767 and has no such net)
    if g is P.G1:
        disp = np.zeros((N, 3), F32)
        disp[777, 1], disp[4242, 0] = np.nan, 1e9
        mesh = I.empty(*g.mesh)
        plan.call("mcpm_paint_f32", t(disp), N, 1, None, 1, 1.0, 2, mesh, 0)
        assert plan.last_outliers() == 2 and bool(torch.isnan(mesh.reshape(-1)[0])) and bool(torch.isfinite(mesh.reshape(-1)[1:]).all())
    # two wild particles (tests/test_gpu_adjoint_carry.py::_paint3_case("wild"))
    disp = I.h["disp"].copy()
    disp[1234], disp[N // 2 + 77] = (20000.25, 0.5, -0.25), (0.75, -17000.5, 1.25)
    _paints(plan, I, t(disp), d["w"], d["w3"])
    if g is P.G1:
        assert plan.last_outliers() >= 2
    # the overflow proof flags every tile for the f64 repaint (tests/test_gpu_parity.py::test_paint3_fixed_point_tiles)
    dc, w15, mesh3 = t(-(np.indices(g.ptcl).reshape(3, -1).T % 4)), t(np.full((N, 3), 1.5)), I.empty(3, *g.mesh)
    plan.call("mcpm_paint3_f32", dc, N, 1, w15, 2, mesh3, 0)
    if g is P.G1:
        import ctypes as C
        redo = C.c_int64()
        plan.call("mcpm_plan_last_redo", C.byref(redo))
        assert redo.value == (64 // 16) ** 3
    _paints(plan, I, dc, None, w15)
    # empty input
    e3, one = I.empty(0, 3), I.empty(1)
    mesh, mesh3 = torch.full(g.mesh, 7., device=I.dev), torch.full((3,) + g.mesh, 7., device=I.dev)
    plan.call("mcpm_paint_f32", e3, 0, 0, d["w"], 1, 0.0, 2, mesh, 0)
    plan.call("mcpm_paint3_f32", e3, 0, 0, d["w3"], 2, mesh3, 0)
    plan.call("mcpm_read_f32", e3, 0, 0, d["mesh"], 1, 2, one)
    assert not bool(mesh.any()) and not bool(mesh3.any())


def test_after_non_finite_and_degenerate_inputs(env):
    """NaN, inf and all-zero weights through the generic paint, the tiled density paint and the tiled paint3; a non-finite displacement; two
    wild particles; the input whose overflow proof sends every tile to the f64 repaint; an empty input.  Then the full probe list."""
    bad = history(env, before=_non_finite)
    assert not bad, bad


def _abandoned(plan, I):
    import torch
    from montecosmo_amd import nbody
    K, g, d = P.K_STEPS, I.geo, I.d
    keep = []
    # (a) a hinted driver call whose chain is not continued; its cotangent arrays stay allocated, the next sweep uses others
    ax, av = I.empty(g.N, 3), I.empty(g.N, 3)
    sbar = torch.zeros(2 * K + 1, dtype=torch.float64, device=I.dev)
    P.chain_step(plan, I, K - 1, d["xb"], d["vb"], ax, av, sbar, hint=True)
    keep += [ax, av, sbar]
    got = P.run(plan, I, ["chain3"])
    # (b) a hinted particle step of the composing API whose mcpm_plan_chained_fb is never fetched
    bx, bv = d["xb"].clone(), d["vb"].clone()
    i = K - 1
    plan.call("mcpm_plan_hint_next_adjoint", float(I.betas[i - 1]), float(I.dg))
    plan.call("mcpm_step_adjoint_particles_il_f32" if g is P.G1 else "mcpm_step_adjoint_particles_f32", I.sx[i], I.sv[i], I.fm[i], d["mesh"],
              float(I.alphas[i]), float(I.betas[i]), I.tau(i), 2, bx, bv, sbar[i:i + 1], sbar[K + i:K + i + 1], 0.5, sbar[2 * K:])
    keep += [bx, bv]
    got.update(P.run(plan, I, ["lone_step"]))
    # (c) a hint with no adjoint call after it at all, followed directly by a one-step sweep; and by the LPT adjoint, then a lone step
    plan.call("mcpm_plan_hint_next_adjoint", float(I.betas[0]), float(I.dg))
    got.update(P.run(plan, I, ["nbody1"]))
    plan.call("mcpm_plan_hint_next_adjoint", float(I.betas[0]), float(I.dg))
    got.update(P.run(plan, I, ["lpt"]))
    got.update(P.run(plan, I, ["lone_step"]))
    # (d) a chain that ran to its end, and then its vel_bar array with other contents as the weights of a three-component paint, at the very
    # scale for which the chain's last hinted call left a weight maximum behind: that maximum is not this array's any more
    cx, cv = I.empty(g.N, 3), I.empty(g.N, 3)
    for i in reversed(range(K)):
        first = i == K - 1
        P.chain_step(plan, I, i, d["xb"] if first else cx, d["vb"] if first else cv, cx, cv, sbar, hint=i > 0)
    cv.copy_(d["w3"])
    reuse = {"paint3": {"scaled-beta0": P._np(P.paint3_beta0(plan, I, cv))}}
    keep += [cx, cv, got, reuse]
    return keep


def test_after_abandoned_chains(env):
    """A carried chain that stops after its first call, a materialised force cotangent that nobody fetches, a hint that no adjoint step follows,
    a finished chain's array painted with other contents: the probe run right after each, and then the full list, equal the fresh values."""
    seen = {}

    def before(plan, I):
        keep = _abandoned(plan, I)
        seen[I.geo.name] = keep[-2:]
        return keep

    bad = history(env, before=before)
    for g in P.GEOS:
        got, reuse = seen[g.name]
        bad += P.differences(env.fresh[g.name], got, tag=g.name + ":right after:")
        if not P.same_bits(env.fresh[g.name]["paint3"]["scaled-beta0"], reuse["paint3"]["scaled-beta0"]):
            bad.append(g.name + ": paint3 of a finished chain's vel_bar array differs from the paint of the same weights elsewhere")
    assert not bad, bad


def _settings(plan, I):
    import ctypes as C
    import torch
    from montecosmo_amd._lib import lib
    g, d = I.geo, I.d
    mesh, mesh3 = I.empty(*g.mesh), I.empty(3, *g.mesh)
    paint = lambda: plan.call("mcpm_paint_f32", d["disp"], g.N, 1, d["w"], 1, 0.0, 2, mesh, 0)
    paint3 = lambda: plan.call("mcpm_paint3_f32", d["disp"], g.N, 1, d["w3"], 2, mesh3, 0)
    x1, v1, fm = I.empty(g.N, 3), I.empty(g.N, 3), I.empty(3 * g.M)
    step = lambda: plan.call("mcpm_bullfrog_step_f32", I.sx[0], I.sv[0], float(I.alphas[0]), float(I.betas[0]), I.tau(0), 2, fm, x1, v1)
    patch = 1 if (g.ptcl[0] % 2 == 0 and g.ptcl[1] % 2 == 0 and g.ptcl[2] % 64 == 0) else 0      # the default (include/mcpm.h)
    try:
        for h in (1, 2, 3, 4, 6):
            plan.call("mcpm_plan_set_halo", h)
            paint()
            paint3()
        plan.call("mcpm_plan_set_halo", 0)
        plan.call("mcpm_plan_set_centre", 0)
        paint()
        paint3()
        plan.call("mcpm_plan_set_centre", 1)
        plan.call("mcpm_plan_set_paint3_fixed", 0)
        paint3()
        plan.call("mcpm_plan_set_paint3_fixed", 1)
        if patch:
            plan.call("mcpm_plan_set_lattice_patch", 0)
            step()
        plan.call("mcpm_plan_set_lattice_patch", patch)
        slots = torch.zeros(64 * 32, dtype=torch.int32, device=I.dev)
        plan.call("mcpm_plan_track_dmax", slots)
        step()
        plan.call("mcpm_plan_track_dmax", None)
        torch.cuda.synchronize()
        assert int(slots.max()) > 0
        plan.call("mcpm_plan_profile", 1)
        step()
        ms, by, calls = (C.c_double * 16)(), (C.c_double * 16)(), (C.c_int64 * 16)()
        assert lib.mcpm_plan_profile_read(plan.h, 16, ms, by, calls) > 0 and sum(calls) > 0      # (returns the number of stages)
        plan.call("mcpm_plan_profile", 0)
        plan.call("mcpm_plan_set_particle_pitch", 3 * g.N + 1088)
        shifted = P.run(plan, I, ["nbody1"])
        plan.call("mcpm_plan_set_particle_pitch", 0)
    finally:      # a failing assertion leaves no setting behind (the plan is this test's own, but so that the rule is kept)
        plan.call("mcpm_plan_set_halo", 0)
        plan.call("mcpm_plan_set_centre", 1)
        plan.call("mcpm_plan_set_paint3_fixed", 1)
        plan.call("mcpm_plan_set_lattice_patch", patch)
        plan.call("mcpm_plan_track_dmax", None)
        plan.call("mcpm_plan_profile", 0)
        plan.call("mcpm_plan_set_particle_pitch", 0)
    return [slots, shifted]


def test_after_settings_round_trips(env):
    """Every setting moved and put back, with work under it: halo, centre, the paint3 accumulator, the lattice patch, dmax tracking,
    profiling, the particle pitch (a one-step sweep under a shifted pitch gives the fresh bits too).  Then the full probe list."""
    seen = {}

    def before(plan, I):
        keep = _settings(plan, I)
        seen[I.geo.name] = keep[-1]
        return keep

    bad = history(env, before=before)
    for g in P.GEOS:
        bad += P.differences(env.fresh[g.name], seen[g.name], tag=g.name + ":shifted pitch:")
    assert not bad, bad


def _reductions(plan, I):
    import torch
    with P.installed(plan, I.geo):
        P.nbody_sweep(plan, I, 12)      # the sweep's rows of plan->reduce: 28 doubles, then 8
        P.nbody_sweep(plan, I, 2)
    dbig = 2 ** 22 + 3                  # many workgroups before few: the scratch of the deterministic sums is reallocated
    rng = np.random.default_rng(77)
    u, q, gr = (torch.from_numpy(rng.standard_normal(dbig).astype(F32)).to(I.dev) for _ in range(3))
    stats = P.mclmc_call(plan, I, u, q, gr, None, dbig)
    assert bool(torch.isfinite(stats).all())
    nchi, ng = 2664, 100                # nchi + 4 ng + 8 = 3072: the whole tables region, then the probes' small tables
    tabs = np.concatenate([np.linspace(0., 3000., nchi), np.linspace(0.2, 1., nchi)] + [np.linspace(0.1, 1., ng)] * 5)
    full = P.lc_call(plan, I, tabs, nchi, ng)
    assert bool(torch.isfinite(full).all()) and bool(full.any())


def test_after_larger_and_smaller_reductions(env):
    """Sweeps of 12 and then 2 steps, a deterministic sum over 2^22 + 3 elements, a table sum that fills its region of plan->reduce: then
    the full probe list, whose sums are all smaller."""
    bad = history(env, before=_reductions)
    assert not bad, bad
