"""MAP, then Laplace, on one MI355X (the flow of the reference's notebooks tests/nbodying.ipynb and tests/pnging.ipynb: MAP, then Fisher), on
the synthetic problem of tools/run_nuts_field.py: `kaiser_post` start -> `samplers.optimize` -> `lapprox.cov_x_from_pot_x_y` for the scalars
and the field's Hutchinson diagonal.
usage: python tools/run_map_laplace.py [final_n=146] [n_epochs=100] [n_probes=64] [lr0=0.1] [evolution=nbody] [out.json] [precond=fourier] [--lik=quad_gauss|...] [--fd-step=F] [--seed=42]
Writes the JSON (pots, the MAP scalars in base space, their Laplace standard deviations, the number of gradient evaluations) and, next to it,
out.npz with `inverse_mass` = 1 / diag of the Hessian over the whole flat vector (scalars from the diagonal of the Schur complement's inverse,
the field from its Hutchinson diagonal), non-positive entries replaced and all clamped to the range of the positive ones: what
`samplers.mclmc_warmup(config={'inverse_mass': ...})` takes, and `tools/run_mclmc_field.py --inverse-mass out.npz` reads."""
import json, sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from montecosmo_amd import model, logdensity, samplers, lapprox, bricks, utils, nbody

opt = lambda name, default: ([a.split("=", 1)[1] for a in sys.argv if a.startswith(f"--{name}=")] or [default])[-1]
lik_type = opt("lik", "quad_gauss")
if lik_type not in logdensity.FieldLevelLogDensity.LIK_STOCH:
    raise SystemExit(f"--lik must be one of {sorted(logdensity.FieldLevelLogDensity.LIK_STOCH)}")
fd_step = float(opt("fd-step", lapprox.FD_STEP))
seed = int(opt("seed", 42))
sys.argv = [a for a in sys.argv if not a.startswith("--")]

nf = int(sys.argv[1]) if len(sys.argv) > 1 else 146
n_epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 100
n_probes = int(sys.argv[3]) if len(sys.argv) > 3 else 64
lr0 = float(sys.argv[4]) if len(sys.argv) > 4 else 0.1
evolution = sys.argv[5] if len(sys.argv) > 5 else "nbody"
out_path = sys.argv[6] if len(sys.argv) > 6 else "map_laplace.json"
precond = sys.argv[7] if len(sys.argv) > 7 else "fourier"

ks = np.logspace(-3, 1, 128)
kpow = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))
fwd = model.FieldLevelForward(final_shape=(nf,) * 3, cell_length=10., box_center=(0., 0., 2500.), evolution=evolution,
                              nbody_n_steps=10, a_obs=0.7, lin_kpow=kpow)
print("shapes: final", fwd.final_shape, "init", fwd.init_shape, "evol", fwd.evol_shape, "paint", fwd.paint_shape, flush=True)
lat = {"Omega_m": dict(loc=0.3111, scale=0.1, loc_fid=0.3111, scale_fid=1e-2),
       "sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2),
       "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2), "b2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=3e-2),
       "bs2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=1e-1), "bn2": dict(loc=0., scale=1e3, loc_fid=0., scale_fid=1.)}
fixed = dict(b3=0., bds2=0., bs3=0., bnpar=0., ngbars=1e-3, s_e=1.0, s_ed=0., s_e2=0., s_k2e=0., s_kmu2e=0.)
torch.manual_seed(0)
truth = {k + "_": 0.0 for k in lat}
truth["white_mesh_"] = torch.randn(fwd.init_shape, device="cuda")
ld0 = logdensity.FieldLevelLogDensity(fwd, torch.zeros(fwd.final_shape), lat, fixed, precond=precond, lik_type=lik_type)
prior_std = 1.0 if ld0.scale is None else ld0.scale
truth["white_mesh_"] = truth["white_mesh_"] * prior_std
base = ld0.base_params(truth)
white = utils.rg2cgh(truth["white_mesh_"]) * ld0.transfer
gxy = fwd.evolve(ld0.make_cosmo(base), {k: base[k] for k in bricks.BIAS_KEYS}, white)
rc = fixed["ngbars"] * fwd.cell_length ** 3
cm = rc * nbody.irfftn(utils.chreshape(nbody.rfftn(gxy), utils.r2chshape(fwd.final_shape)))
obs = cm + rc ** .5 * torch.randn(fwd.final_shape, device="cuda")
ld = logdensity.FieldLevelLogDensity(fwd, obs, lat, fixed, precond=precond, lik_type=lik_type)
flat = samplers.FlatLogDensity(ld)
ns = flat.ns
q0 = flat.pack(ld.kaiser_post(1, scale_field=7 / 8))
print(f"dimension {q0.numel()}, log density at the truth {ld(truth):.1f}", flush=True)

t0 = time.perf_counter()
cb = lambda i, info: print(f"epoch {i:4d} potential {info['potential']:.1f} lr {info['lr']:.4f} [{time.perf_counter() - t0:.0f} s]", flush=True) \
    if i % 10 == 0 or i == n_epochs - 1 else None
q, pots = samplers.optimize(flat, q0, lr0=lr0, n_epochs=n_epochs, callback=cb)
torch.cuda.synchronize()
t_map = time.perf_counter() - t0
n_map = flat.n_eval

t0 = time.perf_counter()
cov, schur = lapprox.cov_x_from_pot_x_y(flat, q, ns, method="hutchinson", chunk_size=n_probes, seed=seed, fd_step=fd_step)
diag = lapprox.hess_diag_hutchinson(flat, q, n_probes=n_probes, seed=seed, fd_step=fd_step, start=ns)      # (the probes cov_x just ran: kept simple)
torch.cuda.synchronize()
t_lap = time.perf_counter() - t0

# standard deviations in base space: d base / d sample by a central difference of `base_params` along each scalar
sample = flat.unpack(q)
map_base = ld.base_params(sample)
names = [n[:-1] for n in flat.scalars]
std_sample = np.sqrt(np.where(np.diag(cov) > 0, np.diag(cov), np.nan))
std_base = {}
for i, n in enumerate(names):
    if flat.sizes[i] != 1:
        continue
    k = int(sum(flat.sizes[:i]))
    hi, lo = dict(sample), dict(sample)
    hi[n + "_"], lo[n + "_"] = sample[n + "_"] + 1e-3, sample[n + "_"] - 1e-3
    std_base[n] = float(abs(float(ld.base_params(hi)[n]) - float(ld.base_params(lo)[n])) / 2e-3 * std_sample[k])

# the starting metric: 1 / H_kk, the scalars from their marginal variance; entries that are not positive take the median of the others
var = torch.cat([torch.tensor(np.diag(cov).copy(), dtype=torch.float64, device=q.device), 1.0 / diag[ns:]])
good = torch.isfinite(var) & (var > 0)
inverse_mass = torch.where(good, var, var[good].median()).clamp(float(var[good].min()), float(var[good].max())).float()
summary = {"final_shape": fwd.final_shape, "init_shape": fwd.init_shape, "evolution": evolution, "precond": precond, "lik_type": lik_type,
           "dimension": int(q.numel()), "n_epochs": len(pots), "lr0": lr0, "n_probes": n_probes, "fd_step": fd_step, "seed": seed,
           "pots": pots, "potential_truth": -ld(truth), "map_s": round(t_map, 2), "laplace_s": round(t_lap, 2),
           "gradient_evals": flat.n_eval, "gradient_evals_map": n_map,
           "map_base": {n: np.asarray(map_base[n], dtype=np.float64).tolist() for n in names},
           "truth_base": {n: np.asarray(base[n], dtype=np.float64).tolist() for n in names},
           "laplace_std_sample": dict(zip(flat.scalars, std_sample.tolist())), "laplace_std_base": std_base,
           "schur_diagonal": np.diag(schur).tolist(), "field_hess_diag": {"min": float(diag[ns:].min()), "median": float(diag[ns:].median()),
                                                                          "max": float(diag[ns:].max()), "non_positive": int((~good[ns:]).sum())}}
print(json.dumps({k: v for k, v in summary.items() if k != "pots"}), flush=True)
open(out_path, "w").write(json.dumps(summary, indent=1))
np.savez(out_path.rsplit(".", 1)[0] + ".npz", inverse_mass=inverse_mass.cpu().numpy(), q_map=q.cpu().numpy())
