"""Times bias_type 'eulerian' against 'lagrangian' on one GPU: one evolve + evolve_vjp (evolution 'nbody', png_type None and 'bias') at
final 64^3 and 146^3 (evolution mesh 256^3), medians of 5 with the two models alternating; then the streaming passes of
mcpm_eulerian_bias_f32 / mcpm_eulerian_bias_vjp_f32 alone at 256^3 (the plan's stage profile brackets exactly them: moments + weights;
VJP pass 1 + pass 2), with their counted bytes per cell and the fraction of the 6.3 TB/s streaming-copy figure of the README.
usage: python tools/time_eulerian.py [--out FILE] [--sizes 64,146]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecosmo_amd import model, bricks, nbody, _lib  # noqa: E402

COPY_TBS = 6.3
ST_LPT = 8      # stage index of the lattice kernels (mcpm_stage_name)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def evolve_times(nf, png_type, n=5, warm=2):
    ks = np.logspace(-3, 1, 128)
    kw = dict(final_shape=(nf,) * 3, cell_length=10., box_center=(0., 0., 2500.), evolution="nbody", nbody_n_steps=10, a_obs=0.7,
              lin_kpow=(ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6)), png_type=png_type)
    fwds = {bt: model.FieldLevelForward(bias_type=bt, **kw) for bt in ("lagrangian", "eulerian")}
    f0 = fwds["eulerian"]
    cosmo = bricks.Planck18()
    bias = dict(b1=0.8, b2=0.2, bs2=-0.15, b3=0.1, bds2=0.1, bs3=-0.05, bn2=5.0, bnpar=2.0)
    pkw = {} if png_type is None else {"png": dict(fNL=100., fNL_bp=3.0, fNL_bpd=-2.0)}
    g = torch.Generator(device="cuda").manual_seed(0)
    white = torch.fft.rfftn(torch.randn(f0.init_shape, device="cuda", generator=g)) * float((f0.init_shape[0] ** 3 / np.prod(f0.box_size)) ** .5)
    gb = torch.randn(f0.paint_shape, device="cuda", generator=g)
    t = {bt: [] for bt in fwds}
    for it in range(warm + n):
        for bt, fwd in fwds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gxy, ctx = fwd.evolve(cosmo, bias, white, return_ctx=True, **pkw)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            grads = fwd.evolve_vjp(ctx, gb)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= warm:
                t[bt].append((t1 - t0, t2 - t1))
            del ctx, grads
    shapes = f"final {nf}^3 (init {f0.init_shape[0]}, evol {f0.evol_shape[0]}, paint {f0.paint_shape[0]})"
    med = {bt: np.median(np.array(v), axis=0) * 1e3 for bt, v in t.items()}
    for bt in fwds:
        say(f"{shapes}  png_type {str(png_type):5s} {bt:10s}  evolve {med[bt][0]:8.1f} ms  evolve_vjp {med[bt][1]:8.1f} ms  sum {med[bt].sum():8.1f} ms")
    say(f"{shapes}  png_type {str(png_type):5s} eulerian / lagrangian = {med['eulerian'].sum() / med['lagrangian'].sum():.3f}")
    nbody.clear_plans()
    torch.cuda.empty_cache()


def stage_ms(plan, fn, n=20, warm=5):
    for _ in range(warm):
        fn()
    ms, by, calls = np.zeros(16), np.zeros(16), (C.c_int64 * 16)()
    plan.call("mcpm_plan_profile", 1)
    for _ in range(n):
        fn()
    _lib.lib.mcpm_plan_profile_read(plan.h, 16, ms.ctypes.data_as(C.POINTER(C.c_double)), by.ctypes.data_as(C.POINTER(C.c_double)), calls)
    plan.call("mcpm_plan_profile", 0)
    return ms[ST_LPT] / calls[ST_LPT] * 1e3, by[ST_LPT] / calls[ST_LPT]      # us, bytes per call


def kernel_times(n=256):
    shape, box = (n,) * 3, (10. * n,) * 3
    g = torch.Generator(device="cuda").manual_seed(1)
    X = torch.fft.rfftn(0.4 * torch.randn(shape, device="cuda", generator=g))
    P = torch.fft.rfftn(2e-5 * torch.randn(shape, device="cuda", generator=g))
    wb = torch.randn(shape, device="cuda", generator=g)
    bias, png = dict(b1=0.8, b2=0.2, bs2=-0.15, bn2=5.0), dict(fNL_bp=2.0e4, fNL_bpd=1.0e4)
    plan, M = nbody.get_plan(shape), float(n) ** 3
    for png_type, phi in ((None, None), ("bias", P)):
        tag = "with phi" if phi is not None else "no phi  "
        fwd = lambda: bricks.eulerian_bias(X, phi, box, bias, png, png_type=png_type, return_ctx=True)
        us, by = stage_ms(plan, fwd)
        say(f"{n}^3 {tag} moments + weights : {us:7.1f} us  {by / M:5.1f} B/cell counted  {by / us * 1e-6:5.2f} TB/s = {by / us * 1e-6 / COPY_TBS:4.2f} of {COPY_TBS} TB/s")
        _, ctx = fwd()
        us, by = stage_ms(plan, lambda: bricks.eulerian_bias_vjp(ctx, wb))
        say(f"{n}^3 {tag} VJP passes 1 + 2  : {us:7.1f} us  {by / M:5.1f} B/cell counted  {by / us * 1e-6:5.2f} TB/s = {by / us * 1e-6 / COPY_TBS:4.2f} of {COPY_TBS} TB/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,146")
    ap.add_argument("--kernel-n", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    say(f"Eulerian against Lagrangian bias on one {torch.cuda.get_device_name(0)}: evolve + evolve_vjp, evolution 'nbody' (10 steps), host clock around a")
    say("device synchronise, 2 warm-up and 5 timed rounds with the two models alternating, medians.  No gate.")
    for nf in [int(s) for s in a.sizes.split(",") if s]:
        for png_type in (None, "bias"):
            evolve_times(nf, png_type)
    say()
    say("Streaming passes of mcpm_eulerian_bias_f32 / _vjp_f32 alone (HIP events around the passes, 5 warm-up and 20 timed calls, mean).")
    say("Counted bytes: moments 1 (2) floats in + weights 7 (8) in, 1 out = 36 (44) B/cell; VJP pass 1 8 (9) in, pass 2 7 (8) in + 7 (8) out = 88 (100) B/cell.")
    kernel_times(a.kernel_n)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
