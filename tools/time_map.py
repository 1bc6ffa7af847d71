"""Timings of the MAP / Laplace passes on one MI355X, and the sweep behind `lapprox.FD_STEP` (profiles/map_laplace.txt is this tool's output).
usage: python tools/time_map.py [--out FILE] [--skip-model] [--skip-sweep]
1. The Adam step (mcpm_adam_step_f32: 16 B read, 12 B written per element) at d = 64^3 and 220^3: medians of 5 by device events, as a
   fraction of a streaming copy of the same 28 B per element, next to the backend='torch' sequence on the same vectors.
2. One `optimize` epoch and one Hutchinson probe (two gradients) against the bare `logdensity_and_grad` call of the config-5 model
   (tests/test_gpu_config5.py: final 146^3, initial 220^3, 10-step N-body): what the new passes add to the gradient.
3. fd_step in 10^(-3 .. -0.5) on the 16^3 model of tests/test_gpu_samplers.py, at the end of 50 Adam epochs from `kaiser_post`: `hess_diag_exact`
   on 16 fixed indices (the scalars, then field entries spread evenly), the change between neighbouring steps, and the middle of the plateau."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from montecosmo_amd import lapprox, logdensity, model, samplers, bricks, utils, nbody  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default=None)
ap.add_argument("--skip-model", action="store_true")
ap.add_argument("--skip-sweep", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_map.py measures on the GPU: none found")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=1, n=5):
    """Median over n of the device-event time of `reps` calls, in ms per call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ts)


say(f"measured on: {torch.cuda.get_device_name(0)}; medians of 5, device events")
say()
say("1. Adam step, 28 B per element")
plan = nbody.get_plan((8, 8, 8))
for n in (64, 220):
    d = n ** 3
    gen = torch.Generator(device="cuda").manual_seed(0)
    q, g = (torch.randn(d, device="cuda", generator=gen) for _ in range(2))
    m, v = torch.zeros_like(q), torch.zeros_like(q)
    src = torch.randn((7 * d + 1) // 2, device="cuda", generator=gen)      # 14 B per element read, 14 B written
    dst = torch.empty_like(src)
    reps = 200 if n == 64 else 20
    t_hip = timed(lambda: plan.call("mcpm_adam_step_f32", q, m, v, g, d, 0.1, 0.9, 0.999, 1e-8, 10., 1000.), reps)
    t_copy = timed(lambda: dst.copy_(src), reps)
    t_torch = timed(lambda: samplers._adam_torch(q, m, v, g, 0.1, 0.9, 0.999, 1e-8, 10., 1000.), max(reps // 10, 2))
    say(f"   d = {n}^3 = {d}: hip {1e3 * t_hip:9.1f} us ({28e-9 * d / (1e-3 * t_hip):7.0f} GB/s), copy of the same bytes {1e3 * t_copy:9.1f} us "
        f"-> copy / hip = {t_copy / t_hip:.2f}; backend='torch' {1e3 * t_torch:9.1f} us = {t_torch / t_hip:.1f} x hip")
    del q, g, m, v, src, dst

if not a.skip_model:
    say()
    say("2. config-5 model (final 146^3, initial 220^3, nbody): what the passes add to one gradient")
    ks = np.logspace(-3, 1, 128)
    kpow = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))
    fwd = model.FieldLevelForward(final_shape=(146,) * 3, cell_length=10., box_center=(0., 0., 2500.), evolution="nbody", nbody_n_steps=10,
                                  a_obs=0.7, lin_kpow=kpow)
    lat = {"Omega_m": dict(loc=0.3111, scale=0.1, loc_fid=0.3111, scale_fid=1e-2), "sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2),
           "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2), "b2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=3e-2),
           "bs2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=1e-1), "bn2": dict(loc=0., scale=1e3, loc_fid=0., scale_fid=1.)}
    fixed = dict(b3=0., bds2=0., bs3=0., bnpar=0., ngbars=1e-3, s_e=1.0, s_ed=0., s_e2=0.)
    gen = torch.Generator(device="cuda").manual_seed(0)
    ld0 = logdensity.FieldLevelLogDensity(fwd, torch.zeros(fwd.final_shape), lat, fixed, precond="kaiser")
    truth = {k + "_": 0.0 for k in lat}
    truth["white_mesh_"] = torch.randn(fwd.init_shape, device="cuda", generator=gen) * ld0.scale
    base = ld0.base_params(truth)
    gxy = fwd.evolve(ld0.make_cosmo(base), {k: base[k] for k in bricks.BIAS_KEYS}, utils.rg2cgh(truth["white_mesh_"]) * ld0.transfer)
    rc = fixed["ngbars"] * fwd.cell_length ** 3
    obs = rc * nbody.irfftn(utils.chreshape(nbody.rfftn(gxy), utils.r2chshape(fwd.final_shape)))
    obs = obs + rc ** .5 * torch.randn(fwd.final_shape, device="cuda", generator=gen)
    flat = samplers.FlatLogDensity(logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="kaiser"))
    q0 = flat.pack(dict(truth, white_mesh_=0.7 * truth["white_mesh_"]))
    t_grad = timed(lambda: flat(q0))
    t_epoch = timed(lambda: samplers.optimize(flat, q0, n_epochs=3)) / 3      # (with the two clones of the start, shared by three epochs)
    t_probe = timed(lambda: lapprox.hess_diag_hutchinson(flat, q0, n_probes=2, fd_step=0.03, start=flat.ns)) / 2
    say(f"   dimension {q0.numel()}: logdensity_and_grad {t_grad:8.2f} ms; one optimize epoch {t_epoch:8.2f} ms = gradient + {100 * (t_epoch / t_grad - 1):.2f} %; "
        f"one Hutchinson probe {t_probe:8.2f} ms = two gradients + {100 * (t_probe / (2 * t_grad) - 1):.2f} %")
    del flat, q0, obs, gxy, truth, ld0
    nbody.clear_plans()
    torch.cuda.empty_cache()

if not a.skip_sweep:
    say()
    say("3. fd_step sweep: hess_diag_exact on 16 fixed indices of the 16^3 LPT model, after 50 Adam epochs from kaiser_post")
    sys.path.insert(0, os.path.join(".", "tests"))
    from test_gpu_samplers import _mock_posterior  # noqa: E402
    _, ld, flat, _, _ = _mock_posterior(16)
    q, pots = samplers.optimize(flat, flat.pack(ld.kaiser_post(1, scale_field=7 / 8)), n_epochs=50)
    d, ns = q.numel(), flat.ns
    idx = list(range(ns)) + [ns + int(j) for j in np.linspace(0, d - ns - 1, 16 - ns).astype(int)]
    say(f"   dimension {d}, potential {pots[0]:.1f} -> {pots[-1]:.1f}; indices {idx}")
    steps = [10.0 ** e for e in np.arange(-3.0, -0.49, 0.25)]
    H = np.array([lapprox.hess_diag_exact(flat, q, indices=idx, fd_step=s).cpu().numpy() for s in steps])
    change = [float(np.median(np.abs(H[k + 1] - H[k]) / np.maximum(np.abs(H[k + 1]), 1e-3))) for k in range(len(steps) - 1)]
    for k, s in enumerate(steps):
        say(f"   fd_step {s:9.5f}: H_kk = " + " ".join(f"{h:9.4f}" for h in H[k]) + (f"   median change to the next {change[k]:.2e}" if k < len(change) else ""))
    lo = min(change)
    best, run = (0, 0), None      # the longest run of neighbouring pairs whose change stays within 3 x the least: the plateau
    for k, c in enumerate(change + [math.inf]):
        if c <= 3 * lo:
            run = k if run is None else run
        elif run is not None:
            best, run = max(best, (k - run, run)), None
    n_pairs, first = best
    chosen = math.sqrt(steps[first] * steps[first + n_pairs])
    say(f"   plateau: fd_step {steps[first]:.5f} .. {steps[first + n_pairs]:.5f} (change <= 3 x {lo:.2e}); its middle: {chosen:.4f}")

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
