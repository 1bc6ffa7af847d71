"""The call a field-level NUTS chain of BASELINE config 5 times -- log density + gradient of the field-level model at a 256^3 evolution
mesh (final 146^3, 'kaiser' preconditioning, 10-step BullFrog; the problem of tests/test_gpu_config5.py and tools/profile_png_ab.py) --
with Alcock-Paczynski off (ap_auto None), automatic (True: fiducial Planck18, Omega_m sampled) and parametrised (False: alpha_iso, alpha_ap
sampled).  The three models live in one process and their timed blocks are interleaved, round after round.
The sampled point sits off the fiducial cosmology (Omega_m_ = 10 sample units = +0.1, alpha_iso_ = 2 = +0.02), so Alcock-Paczynski also
moves the particles by many cells before the paint; `Omega_m_` = 0 and `alpha_iso_` = 0 time the stage with (almost) no such movement.
usage: python tools/profile_ap_ab.py [evolution=nbody] [reps=10] [rounds=3] [Omega_m_=10] [alpha_iso_=2]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from montecosmo_amd import model, logdensity, bricks, utils, nbody

evolution = sys.argv[1] if len(sys.argv) > 1 else "nbody"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
om_ = float(sys.argv[4]) if len(sys.argv) > 4 else 10.0
iso_ = float(sys.argv[5]) if len(sys.argv) > 5 else 2.0
LAT = {"Omega_m": dict(loc=0.3111, scale=0.1, loc_fid=0.3111, scale_fid=1e-2), "sigma8": dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2),
       "b1": dict(loc=1., scale=1e2, loc_fid=1., scale_fid=1e-2), "b2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=3e-2),
       "bs2": dict(loc=0., scale=1e2, loc_fid=0., scale_fid=1e-1), "bn2": dict(loc=0., scale=1e3, loc_fid=0., scale_fid=1.)}
AP_LAT = {k: dict(loc=1., scale=0.1, loc_fid=1., scale_fid=1e-2, low=0., high=np.inf) for k in bricks.AP_KEYS}      # model.py:189-204
FIXED = dict(b3=0., bds2=0., bs3=0., bnpar=0., ngbars=1e-3, s_e=1.0, s_ed=0., s_e2=0.)
ks = np.logspace(-3, 1, 128)
kpow = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))


def forward(ap_auto):
    return model.FieldLevelForward(final_shape=(146,) * 3, cell_length=10., box_center=(0., 0., 2500.), evolution=evolution, nbody_n_steps=10,
                                   a_obs=0.7 if evolution == "nbody" else None, lin_kpow=kpow, ap_auto=ap_auto, cosmo_fid=bricks.Planck18())


gen = torch.Generator(device="cuda").manual_seed(0)
fwd0 = forward(None)
ld0 = logdensity.FieldLevelLogDensity(fwd0, torch.zeros(fwd0.final_shape), LAT, FIXED, precond="kaiser")
truth = {k + "_": 0.0 for k in LAT}
truth["white_mesh_"] = torch.randn(fwd0.init_shape, device="cuda", generator=gen) * ld0.scale
base = ld0.base_params(truth)
gxy = fwd0.evolve(ld0.make_cosmo(base), {k: base[k] for k in bricks.BIAS_KEYS}, utils.rg2cgh(truth["white_mesh_"]) * ld0.transfer)
rc = FIXED["ngbars"] * fwd0.cell_length ** 3
cm = rc * nbody.irfftn(utils.chreshape(nbody.rfftn(gxy), utils.r2chshape(fwd0.final_shape)))
obs = cm + rc ** .5 * torch.randn(fwd0.final_shape, device="cuda", generator=gen)
point = dict(truth, **{"b1_": 30.0, "sigma8_": -8.0, "Omega_m_": om_, "b2_": 5.0, "white_mesh_": 0.7 * truth["white_mesh_"]})
runs = []
for ap_auto in (None, True, False):
    lat = dict(LAT, **AP_LAT) if ap_auto is False else LAT
    pt = dict(point, alpha_iso_=iso_, alpha_ap_=-0.75 * iso_) if ap_auto is False else point
    ld = logdensity.FieldLevelLogDensity(forward(ap_auto), obs, lat, FIXED, precond="kaiser")
    for _ in range(3):
        ld.logdensity_and_grad(pt)
    runs.append((ap_auto, ld, pt, []))
for _ in range(rounds):
    for ap_auto, ld, pt, ms in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            lp, g = ld.logdensity_and_grad(pt)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / reps)
        print(f"{evolution} ap_auto={ap_auto}: {ms[-1]:.2f} ms per log density + gradient ({reps} calls), lp {lp:.2f}", flush=True)
m0 = float(np.mean(runs[0][3]))
for ap_auto, _, _, ms in runs:
    m = float(np.mean(ms))
    print(f"# ap_auto={ap_auto}: mean {m:.2f} ms over {rounds} rounds ({m - m0:+.2f} ms, {100 * (m / m0 - 1):+.1f} %)", flush=True)
