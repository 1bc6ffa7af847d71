"""The three phases of the reference's production pipeline (montecosmo/script.py:32-191: field_warmup -> full_warmup -> full_run) on one MI355X,
on the synthetic problem of tools/run_nuts_field.py: chains start from `kaiser_post(n_chains)`; the field alone is warmed up on
`ld.condition(fiducial scalars)`; every latent is warmed up together (--tune-mass: diagonal preconditioning); the chains' configs are collapsed
to one (`samplers.collapse_configs`); then `n_runs` runs of `n_samples` kept states at `--thinning`, each saved with `save_run` (PATH_c{chain}_{run}.npz
and PATH_c{chain}_last_state.pt).  Chains run one after another.  --resume continues every chain from its saved state (no warm-up; the shared
config is read from PATH_config.pt).  Prints one JSON summary line.
--tune-mass wants three chains or more: a variance estimated from one short warm-up has outliers, under which the unadjusted chain leaves its
step size's stability range; the element-wise MEDIAN over the chains removes them (with two chains it is the mean and does not).  At final 32^3
with 256 + 768 warm-up transitions, one chain on its own estimate ended at an energy error of 1e25 per dimension, four chains at 1.2e-4."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from montecosmo_amd import model, logdensity, samplers, bricks, utils, nbody  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--final-n", type=int, default=64)
ap.add_argument("--evolution", default="lpt", choices=["kaiser", "lpt", "nbody"])
ap.add_argument("--sampler", default="mclmc", choices=["mclmc", "mams"])
ap.add_argument("--n-chains", type=int, default=4)
ap.add_argument("--field-warmup", type=int, default=256, help="transitions of the field-only warm-up")
ap.add_argument("--warmup", type=int, default=512, help="transitions of the full warm-up")
ap.add_argument("--tune-mass", action="store_true", help="estimate a diagonal inverse mass in the full warm-up")
ap.add_argument("--inverse-mass", default=None, metavar="FILE", help="start the full warm-up from the diagonal inverse mass of this .npz "
                "(array 'inverse_mass' over the whole flat vector: tools/run_map_laplace.py writes one)")
ap.add_argument("--n-runs", type=int, default=2)
ap.add_argument("--n-samples", type=int, default=16, help="kept states per run")
ap.add_argument("--thinning", type=int, default=64)
ap.add_argument("--eval-per-ess", type=float, default=1e3)
ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
ap.add_argument("--path", default="mclmc_field", help="prefix of the saved runs")
ap.add_argument("--resume", action="store_true")
ap.add_argument("--start-run", type=int, default=1, help="number of the first run written")
ap.add_argument("--out", default=None, help="also write the summary here")
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()

nf = a.final_n
ks = np.logspace(-3, 1, 128)
kpow = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))
fwd = model.FieldLevelForward(final_shape=(nf,) * 3, cell_length=10., box_center=(0., 0., 2500.), evolution=a.evolution,
                              nbody_n_steps=10, a_obs=0.7, lin_kpow=kpow)
print("shapes: final", fwd.final_shape, "init", fwd.init_shape, "evol", fwd.evol_shape, "paint", fwd.paint_shape, flush=True)
lat = {"Omega_m": dict(loc=0.3111, scale=0.1, loc_fid=0.3111, scale_fid=1e-2),
       "sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2),
       "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2), "b2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=3e-2),
       "bs2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=1e-1), "bn2": dict(loc=0., scale=1e3, loc_fid=0., scale_fid=1.)}
fixed = dict(b3=0., bds2=0., bs3=0., bnpar=0., ngbars=1e-3, s_e=1.0, s_ed=0., s_e2=0., s_k2e=0., s_kmu2e=0.)
torch.manual_seed(0)
truth = {k + "_": 0.0 for k in lat}
ld0 = logdensity.FieldLevelLogDensity(fwd, torch.zeros(fwd.final_shape), lat, fixed, precond="kaiser")
prior_std = 1.0 if ld0.scale is None else ld0.scale
truth["white_mesh_"] = torch.randn(fwd.init_shape, device="cuda") * prior_std
base = ld0.base_params(truth)
white = utils.rg2cgh(truth["white_mesh_"]) * ld0.transfer
gxy = fwd.evolve(ld0.make_cosmo(base), {k: base[k] for k in bricks.BIAS_KEYS}, white)
rc = fixed["ngbars"] * fwd.cell_length ** 3
cm = rc * nbody.irfftn(utils.chreshape(nbody.rfftn(gxy), utils.r2chshape(fwd.final_shape)))
obs = cm + rc ** .5 * torch.randn(fwd.final_shape, device="cuda")
ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond="kaiser")
joint = samplers.FlatLogDensity(ld)
ns = joint.ns
warmup, run = (samplers.mclmc_warmup, samplers.mclmc_run) if a.sampler == "mclmc" else (samplers.mams_warmup, samplers.mams_run)
keep = lambda q: q[:ns].tolist() + [float(q[ns:].std())]
t_all = time.perf_counter()
phases = {}
cfg_path = f"{a.path}_config.pt"

if a.resume and os.path.exists(cfg_path):
    shared = torch.load(cfg_path, weights_only=False)
    if shared["inverse_mass"] is not None:
        shared["inverse_mass"] = shared["inverse_mass"].cuda()
    states = [samplers.load_state(f"{a.path}_c{c}", torch.device("cuda")) for c in range(a.n_chains)]
else:
    # phase 0: every chain from the Kaiser posterior of the initial field, scalars at their fiducial values
    start = ld.kaiser_post(a.seed, base=True, scale_field=7 / 8, n_chains=a.n_chains)
    scalars = {k: np.asarray(v)[0] for k, v in start.items() if k != "white_mesh"}
    # phase 1: field-only warm-up on the conditioned log density (script.py:46-49)
    t0 = time.perf_counter()
    field_ld = ld.condition(scalars)
    field = samplers.FlatLogDensity(field_ld)
    fields = []
    for c in range(a.n_chains):
        q0 = field.pack(ld.sample_params({"white_mesh": start["white_mesh"][c]}))
        st, cf = warmup(field, q0, a.field_warmup, seed=a.seed + 100 * c, backend=a.backend)
        fields.append(field.unpack(st["q"])["white_mesh_"].clone())
        print(f"chain {c} field warm-up: step size {cf['step_size']:.4f} L {cf['L']:.2f} [{time.perf_counter() - t0:.0f} s]", flush=True)
    torch.cuda.synchronize()
    phases["field_warmup_s"] = round(time.perf_counter() - t0, 2)
    # phase 2: full warm-up from the warmed field and the fiducial scalars
    t0 = time.perf_counter()
    states, configs = [], []
    config0 = None
    if a.inverse_mass:
        config0 = {"inverse_mass": torch.from_numpy(np.load(a.inverse_mass)["inverse_mass"]).float().cuda()}
    for c in range(a.n_chains):
        q1 = joint.pack(dict(ld.sample_params(scalars), white_mesh_=fields[c]))
        st, cf = warmup(joint, q1, a.warmup, config=config0, diagonal_preconditioning=a.tune_mass, seed=a.seed + 100 * c + 1, backend=a.backend)
        states.append(st)
        configs.append(cf)
        print(f"chain {c} full warm-up: step size {cf['step_size']:.4f} L {cf['L']:.2f} [{time.perf_counter() - t0:.0f} s]", flush=True)
    torch.cuda.synchronize()
    phases["full_warmup_s"] = round(time.perf_counter() - t0, 2)
    # one shared config (script.py:141-144)
    shared = samplers.collapse_configs(configs, eval_per_ess=a.eval_per_ess)
    if a.sampler == "mams":      # L / step_size is the mean number of steps of a trajectory: the rule above (written for MCLMC's decoherence
        shared["L"] = float(np.median([cf["L"] for cf in configs]))      # length) would make it 200; keep the warm-ups' own trajectory length
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in shared.items()}, cfg_path)
print(f"shared config: step size {shared['step_size']:.4f} L {shared['L']:.2f} inverse mass "
      f"{'none' if shared['inverse_mass'] is None else [round(float(x), 4) for x in shared['inverse_mass'][:ns]]} (scalars)", flush=True)

# phase 3: the runs
t0 = time.perf_counter()
n_eval0 = joint.n_eval
draws, infos, backend = [], [], None
for c in range(a.n_chains):
    st = states[c]
    for i_run in range(a.start_run, a.start_run + a.n_runs):
        res = run(joint, st, shared, a.n_samples, thinning=a.thinning, keep=keep, backend=a.backend)
        samplers.save_run(res, i_run, f"{a.path}_c{c}", extra_fields=("n_evals", "energy_change", "mse_per_dim", "acceptance_rate", "step_size", "logdensity"))
        st, backend = res["last_state"], res["backend"]
        draws += res["samples"]
        infos += res["infos"]
        print(f"chain {c} run {i_run}: lp {res['infos'][-1]['logdensity']:.1f} [{time.perf_counter() - t0:.0f} s]", flush=True)
torch.cuda.synchronize()
run_s = time.perf_counter() - t0
n_eval_run = joint.n_eval - n_eval0
phases["run_s"] = round(run_s, 2)
draws = np.array(draws)
summary = {"sampler": a.sampler, "backend": backend, "final_shape": fwd.final_shape, "init_shape": fwd.init_shape, "evolution": a.evolution,
           "dimension": int(ns + np.prod(fwd.init_shape)), "n_chains": a.n_chains, "field_warmup": a.field_warmup, "warmup": a.warmup,
           "tune_mass": a.tune_mass, "n_runs": a.n_runs, "n_samples": a.n_samples, "thinning": a.thinning, "resumed": bool(a.resume),
           "step_size": shared["step_size"], "L": shared["L"], **phases, "wall_s": round(time.perf_counter() - t_all, 1),
           "gradient_evals_run": n_eval_run, "ms_per_gradient_run": round(1e3 * run_s / max(n_eval_run, 1), 3),
           "mse_per_dim": float(np.nanmean([i["mse_per_dim"] for i in infos])) if a.sampler == "mclmc" else None,
           "acceptance_rate": float(np.mean([i["acceptance_rate"] for i in infos])) if a.sampler == "mams" else None,
           "logdensity_truth": ld(truth), "logdensity_end": infos[-1]["logdensity"],
           "posterior_mean_sample_space": dict(zip(joint.scalars + ["white_std"], draws.mean(0).round(4).tolist()))}
print(json.dumps(summary), flush=True)
if a.out:
    open(a.out, "w").write(json.dumps(summary, indent=1))
