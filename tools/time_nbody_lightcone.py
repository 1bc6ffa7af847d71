"""Times the N-body light cone on one GPU, device events, medians of 5.
1. The select pass (mcpm_nbody_lightcone_f32) alone, and the light-cone share of the reverse sweep -- the g_bar pass, the K + 1 injection
   passes and the K - 1 maximum passes the injected carries cost -- as the difference between mcpm_nbody_bf_lc_vjp_f32 and
   mcpm_nbody_bf_vjp_f32 on the same checkpoints and cotangents; bytes from shapes, as a fraction of the README's 6.3 TB/s streaming copy.
2. One evolve + evolve_vjp of FieldLevelForward(evolution='nbody') on the light cone (a_obs=None) at final 64^3 and 146^3 (evolution 256^3),
   10 steps, against the same model at fixed a_obs and against 'lpt' on the light cone.
usage: python tools/time_nbody_lightcone.py [--out FILE] [--sizes 64,146] [--kernel-n 256]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from montecosmo_amd import model, bricks, nbody, synth  # noqa: E402

COPY_TBS = 6.3
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def event_ms(fn, n=5, warm=2):
    """Median over n calls of the device time of fn (HIP events on the current stream)."""
    out = []
    for it in range(warm + n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warm:
            out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def kernel_times(n, K=10):
    shape = (n,) * 3
    spec = synth.init_mesh(n, seed=0, rms_disp=1.5)
    pos = nbody.LatticePos.regular(shape)
    cosmo = bricks.Planck18()
    N = n ** 3
    g = torch.Generator(device="cuda").manual_seed(0)
    # shells: a_p grows along x, so that neighbours share an interval except at the K - 1 boundaries, as on a survey's light cone
    a_p = (0.25 + 0.7 * torch.arange(n, device="cuda", dtype=torch.float32) / n)[:, None, None].expand(n, n, n).reshape(-1).contiguous()
    (lp, vel), ctx = nbody.nbody_bf(cosmo, spec, pos, a0=0.2, a1=a_p, a_end=0.9, n_steps=K, return_ctx=True, lattice_out=True)
    plan = ctx.plan
    d, v = torch.empty_like(lp.disp), torch.empty_like(vel)
    sel = lambda: plan.call("mcpm_nbody_lightcone_f32", ctx.ckpt, K, float(ctx.dg), float(ctx.lpt_s[0]), ctx.final[0], ctx.final[1], ctx.g_p, d, v)
    ms = event_ms(sel)
    by = 76.0 * N
    say(f"{n}^3 K={K} select pass              : {ms * 1e3:8.1f} us  76 B/particle  {by / ms * 1e-9:5.2f} TB/s = {by / ms * 1e-9 / COPY_TBS:4.2f} of {COPY_TBS} TB/s")
    xb, vb = torch.randn((N, 3), device="cuda", generator=g), torch.randn((N, 3), device="cuda", generator=g)
    plain = nbody.NbodyCtx(**{k: getattr(ctx, k) for k in ("plan", "init_mesh", "n_steps", "dg", "alphas", "betas", "lpt_s", "lpt_order", "paint_order",
                                                          "ckpt", "cosmo", "a0", "a1", "integrator", "pitch")})
    t_lc = event_ms(lambda: nbody.nbody_bf_vjp(ctx, xb, vb))
    t_pl = event_ms(lambda: nbody.nbody_bf_vjp(plain, xb, vb))
    by = (4.0 * K + 150.0 + 12.0 * (K - 1)) * N
    say(f"{n}^3 K={K} reverse sweep            : light cone {t_lc:8.2f} ms  plain {t_pl:8.2f} ms  ratio {t_lc / t_pl:.3f}")
    say(f"{n}^3 K={K} g_bar + injection passes : {(t_lc - t_pl) * 1e3:8.1f} us  {by / N:.0f} B/particle counted (4 K + 150, and 12 (K - 1) for the maxima of the "
        f"injected carries)  {by / max(t_lc - t_pl, 1e-9) * 1e-9:5.2f} TB/s = {by / max(t_lc - t_pl, 1e-9) * 1e-9 / COPY_TBS:4.2f} of {COPY_TBS} TB/s")
    del ctx, plain
    nbody.clear_plans()
    torch.cuda.empty_cache()


def evolve_times(nf):
    ks = np.logspace(-3, 1, 128)
    kw = dict(final_shape=(nf,) * 3, cell_length=10., box_center=(0., 0., 2500.), nbody_n_steps=10, nbody_a_start=0.1,
              lin_kpow=(ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6)))
    fwds = {"nbody light cone": model.FieldLevelForward(evolution="nbody", a_obs=None, **kw),
            "nbody fixed a_obs": model.FieldLevelForward(evolution="nbody", a_obs=0.45, **kw),
            "lpt light cone": model.FieldLevelForward(evolution="lpt", a_obs=None, **kw)}
    f0 = fwds["nbody light cone"]
    cosmo = bricks.Planck18()
    bias = dict(b1=0.8, b2=0.2, bs2=-0.15, b3=0.1, bds2=0.1, bs3=-0.05, bn2=5.0, bnpar=2.0)
    g = torch.Generator(device="cuda").manual_seed(0)
    white = torch.fft.rfftn(torch.randn(f0.init_shape, device="cuda", generator=g)) * float((f0.init_shape[0] ** 3 / np.prod(f0.box_size)) ** .5)
    gb = torch.randn(f0.paint_shape, device="cuda", generator=g)
    med = {}
    for name, fwd in fwds.items():
        def both():
            gxy, ctx = fwd.evolve(cosmo, bias, white, return_ctx=True)
            fwd.evolve_vjp(ctx, gb)
        med[name] = event_ms(both)
    shapes = f"final {nf}^3 (evol {f0.evol_shape[0]}^3, particles {f0.ptcl_shape[0]}^3)"
    for name in fwds:
        say(f"{shapes}  {name:18s} evolve + evolve_vjp {med[name]:8.1f} ms")
    say(f"{shapes}  light cone / fixed a_obs = {med['nbody light cone'] / med['nbody fixed a_obs']:.3f}   light cone nbody / lpt = "
        f"{med['nbody light cone'] / med['lpt light cone']:.2f}")
    nbody.clear_plans()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,146")
    ap.add_argument("--kernel-n", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    say(f"N-body light cone on one {torch.cuda.get_device_name(0)}: HIP events, 2 warm-up and 5 timed calls, medians.  No gate.")
    kernel_times(a.kernel_n)
    say()
    for nf in [int(s) for s in a.sizes.split(",") if s]:
        evolve_times(nf)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
