"""Times of the credible intervals and quantiles of chains (montecosmo_amd/bdec.py on csrc/bdec.hip) on one MI355X, written to
profiles/credible_intervals.txt: (C, N, D) = (4, 1000, 64^3) float32 draws generated on the device from a seed, medians of 5 runs after a
warm-up, from device events.
  the sort kernel (mcpm_bdec_sort_f32) in one call for credint(type='small') at p = 0.95, and in one call for the six ranks of quantile at
    three p; its rate on the C N D 4 bytes it reads once;
  the whole calls bdec.sci_noweights and bdec.quantile on resident draws (host clock around a synchronise: they end in a copy back);
  the same results formed on the same device by torch.sort over a pooled, transposed copy, in chunks of dimensions that keep the copy,
    the sorted values and the int64 indices (16 bytes per draw) within CHUNK_SORT_BYTES, and checked to be bitwise the kernel's;
  a streaming copy of the bytes read (torch's copy of the draws: it reads and writes them).
usage: python tools/time_bdec.py [output file]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from montecosmo_amd import bdec, chains

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "credible_intervals.txt")
if not torch.cuda.is_available():
    raise SystemExit("tools/time_bdec.py measures on a GPU; there is none here")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
C_, N, D, REPS = 4, 1000, 64 ** 3, 5
M = C_ * N
P_CI, PS = .95, np.array([.05, .5, .95])
CHUNK_SORT_BYTES = 1 << 30


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


lines = [f"# tools/time_bdec.py on {torch.cuda.get_device_name(dev)} ({torch.cuda.get_device_properties(dev).gcnArchName}): "
         f"(C, N, D) = ({C_}, {N}, {D}) float32, iid normal draws, medians of {REPS} (min .. max)"]


def report(name, ms, extra=""):
    med, lo, hi = ms
    line = f"{name:<58s} {med:10.3f} ms ({lo:.3f} .. {hi:.3f})  {extra}"
    print(line, flush=True)
    lines.append(line)
    return med


g = torch.Generator(device=dev).manual_seed(1)
x = torch.randn((C_, N, D), dtype=torch.float32, device=dev, generator=g)
nbytes = x.numel() * 4
r = chains._Resident(x)
L = bdec._sci_length(P_CI, M)
i_hi = bdec._ranks(PS, M)
ranks = sorted({int(v) for v in np.concatenate([i_hi - 1, i_hi])})

# a streaming copy of the draws
y = torch.empty_like(x)
ms = event_ms(lambda: y.copy_(x))
copy_ms = report("streaming copy of the draws (reads and writes them)", ms, f"{nbytes / 1e9:.2f} GB each way  {2 * nbytes / (ms[0] * 1e-3) / 1e12:.2f} TB/s")
del y

# the kernel alone
fused_ci = report("sort kernel: credint small, p = 0.95 (device events)", event_ms(lambda: bdec._dev_lds(r, [], L, None, False)),
                  f"L = {L}")
fused_q = report(f"sort kernel: the {len(ranks)} ranks of quantile at {len(PS)} p (device events)", event_ms(lambda: bdec._dev_lds(r, ranks, None, None, False)))
lines.append(f"#   the kernel reads {nbytes / 1e9:.2f} GB once: {nbytes / (fused_ci * 1e-3) / 1e12:.2f} TB/s in the credint call, "
             f"{fused_ci / copy_ms:.1f} streaming copies")
report("bdec.sci_noweights whole call (host clock)", host_ms(lambda: bdec.sci_noweights(x, P_CI, axis=(0, 1), backend="hip")))
report("bdec.quantile whole call, three p (host clock)", host_ms(lambda: bdec.quantile(x, PS, axis=(0, 1), backend="hip")))


# the same by torch.sort over a pooled, transposed copy, in chunks that fit
per = max(1, CHUNK_SORT_BYTES // (16 * M))
idx = torch.as_tensor(ranks, device=dev)


def sorted_chunks():
    for lo in range(0, D, per):
        yield lo, torch.sort(x[:, :, lo:lo + per].reshape(M, -1).t().contiguous(), dim=1).values


def torch_ci():
    out = torch.empty((2, D), dtype=torch.float32, device=dev)
    for lo, s in sorted_chunks():
        i = torch.argmin(s[:, L:].double() - s[:, :M - L].double(), dim=1)
        out[0, lo:lo + per] = s.gather(1, i[:, None])[:, 0]
        out[1, lo:lo + per] = s.gather(1, (i + L)[:, None])[:, 0]
    return out


def torch_q():
    out = torch.empty((len(ranks), D), dtype=torch.float32, device=dev)
    for lo, s in sorted_chunks():
        out[:, lo:lo + per] = s[:, idx].t()
    return out


sort_ci = report(f"torch.sort sequence: credint small ({per} dimensions per chunk)", event_ms(torch_ci))
sort_q = report("torch.sort sequence: the ranks of quantile", event_ms(torch_q))
same_ci = torch.equal(torch_ci(), bdec._dev_lds(r, [], L, None, False)["sci"])
same_q = torch.equal(torch_q(), bdec._dev_lds(r, ranks, None, None, False)["rank"])
lines.append(f"# torch.sort sequence / sort kernel: credint {sort_ci / fused_ci:.2f}, quantile {sort_q / fused_q:.2f}  "
             f"(results bitwise equal: credint {same_ci}, quantile {same_q}; iid normal draws hold no NaN and no zero)")
torch.cuda.reset_peak_memory_stats(dev)
base = torch.cuda.max_memory_allocated(dev)
bdec.sci_noweights(x, P_CI, axis=(0, 1), backend="hip")
peak_fused = torch.cuda.max_memory_allocated(dev) - base
torch.cuda.reset_peak_memory_stats(dev)
torch_ci()
peak_sort = torch.cuda.max_memory_allocated(dev) - base
lines.append(f"# device memory allocated beside the draws: sort kernel call {peak_fused / 1e6:.1f} MB, torch.sort sequence {peak_sort / 1e6:.1f} MB")
print("\n".join(lines[-2:]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
