"""Times of the real-space binned diagnostics (montecosmo_amd/metrics.py on csrc/binned.hip) on one MI355X, written to
profiles/binned_diagnostics.txt: n = 256^3 cells, batch 1 and 16, medians of 5 runs after a warm-up, a host clock around work that ends
in a device synchronise.
  mse_radius, default shells (float64 radii): the binning pass alone (mcpm_binned_sums_f32 on prepared device arrays) and the whole call;
  mse_value, 50 quantile edges: the sort that finds the edges, the binning pass alone, and the whole call.
Each line: milliseconds; the bytes the algorithm needs (the binning values and mesh0 once, mesh1 once per batch row) over the time, as a
fraction of the 6.3 TB/s streaming-copy rate; and the same result from numpy on the host, device-to-host copy included, one sample at a
time as the reference does it (ONE run: it takes seconds).
usage: python tools/time_binned.py [output file]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from montecosmo_amd import metrics, _lib

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "binned_diagnostics.txt")
if not torch.cuda.is_available():
    raise SystemExit("tools/time_binned.py measures on a GPU; there is none here")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
COPY_RATE = 6.3e12
N, CELL, REPS = 256, 4., 5
n = N ** 3


def median_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def pass_only(values, t0, t1, edges, batch):
    """One mcpm_binned_sums_f32 call on prepared device arrays (it uploads the edges and synchronises once; no copy back)."""
    ws = C.c_int64()
    _lib.call("mcpm_binned_workspace", n, len(edges), batch, C.byref(ws))
    work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
    res = torch.empty((2 + batch, len(edges) - 1), dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    v, a, b = values.reshape(-1), t0.reshape(1, n), t1.reshape(batch, n)
    return lambda: _lib.call("mcpm_binned_sums_f32", stream, n, v, int(v.dtype == torch.float64), a, 0, b, n, CELL ** 3, None, batch, edges,
                             len(edges), work, ws.value, res)


def host_numpy(values, t0, t1, edges_of):
    """The reference's route: copy to the host, then per sample np.digitize and three np.bincount; returns seconds."""
    t = time.perf_counter()
    v, a, b = values.cpu().numpy().reshape(-1), t0.cpu().numpy().reshape(-1), t1.cpu().numpy().reshape(-1, n)
    for row in b:
        se = (a - row) ** 2 * CELL ** 3
        edges = edges_of(v)
        dig = np.digitize(v, edges)
        cnt = np.bincount(dig, minlength=len(edges) + 1)[1:-1]
        np.bincount(dig, weights=v, minlength=len(edges) + 1)[1:-1] / cnt
        np.bincount(dig, weights=se, minlength=len(edges) + 1)[1:-1] / cnt
    return time.perf_counter() - t


lines = [f"# tools/time_binned.py on {torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName}): n = {N}^3 cells, medians of {REPS} (min .. max), host clock + synchronise",
         f"# share = algorithmic bytes / time / {COPY_RATE / 1e12} TB/s; host = numpy on the host per sample, copy included, one run"]


def report(name, batch, nbytes, fn, host_s=None):
    med, lo, hi = median_ms(fn)
    line = f"{name:<44s} batch {batch:>2d}  {med:9.3f} ms ({lo:.3f} .. {hi:.3f})"
    if nbytes:
        line += f"  {nbytes / 1e9:6.2f} GB  share {nbytes / (med * 1e-3) / COPY_RATE:6.3f}"
    if host_s is not None:
        line += f"  host {host_s * 1e3:10.1f} ms"
    print(line, flush=True)
    lines.append(line)


g = torch.Generator(device=dev).manual_seed(0)
ix = (torch.arange(N, device=dev, dtype=torch.float64) - N / 2) * CELL


def radii(axis):
    """float64 radii of a box whose centre is 2000 away along `axis`.  Along z, the fastest axis, the 64 cells of a round fall into 64
    shells (the serving loop's worst case); along x they share one to three."""
    c = [ix + (2000. if i == axis else 0.) for i in range(3)]
    return torch.sqrt(c[0][:, None, None] ** 2 + c[1][None, :, None] ** 2 + c[2][None, None, :] ** 2)


mesh0 = torch.randn((N, N, N), device=dev, generator=g)
for batch in (1, 16):
    mesh1 = mesh0 + 0.3 * torch.randn((batch, N, N, N), device=dev, generator=g)
    # by radius
    nbytes = n * (8 + 4 + 4 * batch)
    rmesh = radii(0)
    redges = metrics._vedges(rmesh, None, 1, CELL)[0]
    report(f"mse_radius pass, centre along x ({len(redges)} edges)", batch, nbytes, pass_only(rmesh, mesh0, mesh1, redges, batch))
    rmesh = radii(2)
    redges = metrics._vedges(rmesh, None, 1, CELL)[0]
    host = host_numpy(rmesh, mesh0, mesh1, lambda v: redges)
    report(f"mse_radius pass, centre along z ({len(redges)} edges)", batch, nbytes, pass_only(rmesh, mesh0, mesh1, redges, batch))
    report("mse_radius whole call, centre along z", batch, nbytes, lambda: metrics.mse_radius(mesh0, mesh1, rmesh, CELL), host)
    # by value
    q = np.linspace(0., 1., 50, endpoint=False) + .01
    vedges = metrics._vedges(mesh0, 50, None)[0]
    assert np.array_equal(vedges, np.quantile(mesh0.cpu().numpy().astype(np.float64), q))
    nbytes = n * (4 + 4 * batch)
    host = host_numpy(mesh0, mesh0, mesh1, lambda v: np.quantile(v, q))
    if batch == 1:
        report("mse_value edges: sort + 50 quantiles", batch, 0, lambda: metrics._vedges(mesh0, 50, None))
    report("mse_value pass (50 quantile edges)", batch, nbytes, pass_only(mesh0, mesh0, mesh1, vedges, batch))
    report("mse_value whole call", batch, nbytes, lambda: metrics.mse_value(mesh0, mesh1, CELL, 50), host)
    del mesh1
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
