"""Device time of the binned spectra (montecosmo_amd/metrics.py), HIP events after warm-up:
  1. powtranscoh of two real 512^3 meshes (two R2C + one binning pass + host work), and the R2C and binning pieces alone;
  2. powtranscoh from two 512^3 half-spectra;
  3. powtranscoh of a 256^3 mesh against a batch of 8.
The binning rate counts algorithmic bytes: 8 * B * nx * ny * (nz/2+1) per spectrum read.
usage: python tools/time_spectrum.py [reps=10]   (profile: rocprofv3 --kernel-trace --stats -- python tools/time_spectrum.py 3)"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from montecosmo_amd import metrics, nbody
from montecosmo_amd._lib import lib, check

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
HBM = 8e12


def timed(fn, n=reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def binning_only(s0, s1, box, batch=1, stride1=0):
    """One mcpm_spectrum_bins_c64 launch sequence on prepared spectra (no host tables, no copies back)."""
    shape = nbody.ch2rshape(s0.shape[-3:])
    edges = metrics._kedges(shape, box)
    ktab = metrics._ktable(shape, np.asarray(box, dtype=np.float64))
    ws = C.c_int64()
    check(lib.mcpm_spectrum_workspace(*shape, len(edges), 1, 1, batch, C.byref(ws)), None, "workspace")
    work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
    out = torch.empty(batch * 6 * (len(edges) - 1), dtype=torch.float64, device=dev)
    los = np.zeros(3)
    ells = (C.c_int * 1)(0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f64 = metrics._f64p

    def run():
        check(lib.mcpm_spectrum_bins_c64(stream, *shape, nbody._ptr(s0), 0, nbody._ptr(s1), stride1, batch, f64(ktab), None, None,
                                         f64(edges), len(edges), f64(los), ells, 1, nbody._ptr(work), ws.value, nbody._ptr(out)),
              None, "bins")
    return run


rec = {}
n, box = 512, (1000., 1000., 1000.)
g = torch.Generator(device=dev).manual_seed(0)
m0 = torch.randn((n, n, n), device=dev, generator=g)
m1 = torch.randn((n, n, n), device=dev, generator=g)
s0, s1 = nbody.rfftn(m0), nbody.rfftn(m1)
plan = nbody.get_plan((n, n, n))
spec_tmp = torch.empty_like(s0)
rec["r2c_512_ms"] = timed(lambda: plan.call("mcpm_fft_r2c", nbody._ptr(m0), nbody._ptr(spec_tmp), 1))
rec["binning_512_two_spectra_ms"] = timed(binning_only(s0, s1, box))
bytes_ = 2 * 8 * n * n * (n // 2 + 1)
rec["binning_512_GBps"] = bytes_ / rec["binning_512_two_spectra_ms"] / 1e6
rec["binning_512_hbm_share"] = bytes_ / (rec["binning_512_two_spectra_ms"] * 1e-3) / HBM
rec["powtranscoh_512_real_ms"] = timed(lambda: metrics.powtranscoh(m0, m1, box))
rec["powtranscoh_512_spectra_ms"] = timed(lambda: metrics.powtranscoh(s0, s1, box))
del m0, m1, s0, s1, spec_tmp
torch.cuda.empty_cache()

n, box, B = 256, (1000., 1000., 1000.), 8
t0 = torch.randn((n, n, n), device=dev, generator=g)
tb = torch.randn((B, n, n, n), device=dev, generator=g)
rec["powtranscoh_256_batch8_ms"] = timed(lambda: metrics.powtranscoh(t0, tb, box))
sb = torch.stack([nbody.rfftn(tb[i]) for i in range(B)])
st = nbody.rfftn(t0)
rec["binning_256_batch8_ms"] = timed(binning_only(st, sb, box, batch=B, stride1=n * n * (n // 2 + 1)))
print(json.dumps({k: round(v, 4) for k, v in rec.items()}), flush=True)
