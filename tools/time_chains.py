"""Times of the chain diagnostics (montecosmo_amd/chains.py on csrc/chains.hip) on one MI355X, written to
profiles/chain_diagnostics.txt: (C, N, D) = (4, 1000, 64^3) float32 draws generated on the device from a seed, medians of 5 runs after a
warm-up, from device events.
  the moments pass (mcpm_chain_moments_f32) alone: its rate on C N D 4 bytes against the 6.3 TB/s streaming copy (it reads them twice);
  the tau pass (mcpm_chain_tau_f32) alone for iid draws and for AR(1) draws with phi = 0.9, with the sweeps of the slowest wave (16 lags
    per sweep) and the mean and maximum number of lags summed;
  the whole calls multi_ess and split_gelman_rubin on resident draws (host clock around a synchronise: they end in a copy back);
  the host backend at (4, 1000, 32^3), ONE run, with the number of threads it may use (numpy's FFT runs on one).
usage: python tools/time_chains.py [output file]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from montecosmo_amd import chains

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chain_diagnostics.txt")
if not torch.cuda.is_available():
    raise SystemExit("tools/time_chains.py measures on a GPU; there is none here")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
COPY_RATE = 6.3e12
C_, N, D, D_HOST, REPS, LAGS_PER_SWEEP = 4, 1000, 64 ** 3, 32 ** 3, 5, 16


def event_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def host_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def ar1(phi, d, seed):
    """Stationary AR(1) draws (C, N, d) float32 on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.empty((C_, N, d), dtype=torch.float32, device=dev)
    x[:, 0] = torch.randn((C_, d), device=dev, generator=g)
    s = (1. - phi * phi) ** .5
    for t in range(1, N):
        x[:, t] = phi * x[:, t - 1] + s * torch.randn((C_, d), device=dev, generator=g)
    return x


lines = [f"# tools/time_chains.py on {torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName}): "
         f"(C, N, D) = ({C_}, {N}, {D}) float32, medians of {REPS} (min .. max)",
         f"# share = C N D 4 bytes / time / {COPY_RATE / 1e12} TB/s"]


def report(name, ms, extra=""):
    med, lo, hi = ms
    line = f"{name:<46s} {med:10.3f} ms ({lo:.3f} .. {hi:.3f})  {extra}"
    print(line, flush=True)
    lines.append(line)


nbytes = C_ * N * D * 4
for label, phi in (("iid", 0.), ("AR(1) phi = 0.9", .9)):
    x = ar1(phi, D, 1)
    r = chains._Resident(x)
    if phi == 0.:
        ms = event_ms(lambda: chains._dev_moments(r))
        report("moments pass (device events)", ms, f"{nbytes / 1e9:.2f} GB  share {nbytes / (ms[0] * 1e-3) / COPY_RATE:.3f}")
    mean, m2 = chains._dev_moments(r)
    tau, lags = chains._dev_tau(r, mean, m2, True)
    lags = lags.cpu().numpy()
    waves = np.pad(lags, (0, -len(lags) % 64), mode="edge").reshape(-1, 64).max(axis=1)      # a wave goes on while a lane is unfinished
    sweeps = -(-waves // LAGS_PER_SWEEP)
    ms = event_ms(lambda: chains._dev_tau(r, mean, m2, True))
    report(f"tau pass, {label} (device events)", ms, f"sweeps: slowest wave {sweeps.max()}, mean wave {sweeps.mean():.1f};  lags summed: mean "
           f"{lags.mean():.1f}, max {lags.max()};  {nbytes * 2 * sweeps.mean() / (ms[0] * 1e-3) / 1e12:.2f} TB/s of loads issued")
    report(f"multi_ess whole call, {label} (host clock)", host_ms(lambda: chains.multi_ess(x)))
    if phi == 0.:
        report("split_gelman_rubin whole call (host clock)", host_ms(lambda: chains.split_gelman_rubin(x)))
    del x, r, mean, m2, tau

xh = ar1(.9, D_HOST, 2).cpu().numpy()
t = time.perf_counter()
chains.multi_ess(xh, backend="host")
host_s = time.perf_counter() - t
t = time.perf_counter()
chains.multi_ess(xh, backend="hip")
up_s = time.perf_counter() - t
threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
line = (f"host backend multi_ess at ({C_}, {N}, {D_HOST}), AR(1) phi = 0.9, one run: {host_s * 1e3:.0f} ms ({threads} CPUs allowed, torch threads "
        f"{torch.get_num_threads()}; numpy's FFT uses one);  the same host array through the upload and the kernels: {up_s * 1e3:.0f} ms")
print(line, flush=True)
lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
