"""Device time of the binned bispectrum (montecosmo_amd/metrics.py `bispectrum`, csrc/bispectrum.hip) on one MI355X: a 256^3 mesh with
the default edges and triangles, a single mesh and a batch of 8, medians of 5 after one warm-up, HIP events.
  - the pieces of one row: the shell split, the C2R of its n_bins spectra, the triple sums, and the whole call (host work, the triangle
    counts from the cache, the spectrum pass for kmean and the copies back included);
  - a plain torch restatement on the same device: one masked irfftn per bin and one product-sum per triangle;
  - the LDS read rate of the sums pass, 3 * M * T * 8 bytes (float64 in LDS) over its time, against 256 B/clk/CU (ds_read_b64) on 256 CUs
    at 2.4 GHz.
usage: python tools/time_bispectrum.py [out=profiles/bispectrum.txt] [n=256]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from montecosmo_amd import metrics, nbody, _lib

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bispectrum.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
CUS, CLK, LDS_RATE = 256, 2.4e9, 256.


def median_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


shape, box = (n, n, n), np.array([1000., 1000., 1000.])
edges = metrics._bispec_edges(shape, box)
tri = metrics._bispec_triangles(edges)
n_bins, T, M, mh = len(edges) - 1, len(tri), n ** 3, n * n * (n // 2 + 1)
g = torch.Generator(device=dev).manual_seed(0)
gauss = torch.randn((8,) + shape, device=dev, generator=g)
meshes = gauss + 0.5 * (gauss * gauss - 1)
del gauss
lines = [f"binned bispectrum, {n}^3, box 1000, default edges ({n_bins} bins) and triangles (T = {T}); medians of 5, ms"]

# the pieces of one row
ktab = metrics._ktable(shape, box)
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
plan = nbody.get_plan(shape)
spec = metrics._to_spec(meshes[:1], True, shape, dev)
shells = torch.empty((1, n_bins, n, n, n // 2 + 1), dtype=torch.complex64, device=dev)
fields = torch.empty((1, n_bins) + shape, dtype=torch.float32, device=dev)
tri_dev = torch.from_numpy(np.sort(tri, axis=1).astype(np.int32)).to(dev)
ws = C.c_int64()
_lib.call("mcpm_bispectrum_workspace", n, n, n, n_bins, T, 1, C.byref(ws))
work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
res = torch.empty((1, T), dtype=torch.float64, device=dev)


def split():
    _lib.call("mcpm_bispectrum_split_c64", stream, n, n, n, spec, mh, 1, ktab, None, edges, len(edges), shells)


def c2r():
    plan.call("mcpm_fft_c2r", shells[0], fields[0], n_bins)


def sums():
    _lib.call("mcpm_bispectrum_sums_f32", stream, fields, M, n_bins, 1, tri_dev, T, work, ws.value, res)


t_split = median_ms(split)
t_c2r = median_ms(lambda: (split(), c2r()))      # (the C2R may overwrite its input: every repeat transforms a fresh split)
t_sums = median_ms(sums)
lds_bytes = 3. * M * T * 8
rate = lds_bytes / (t_sums * 1e-3)
lines += [f"  shell split (writes {n_bins * mh * 8 / 1e9:.2f} GB)            {t_split:9.3f}",
          f"  C2R of {n_bins} spectra (split + C2R minus split)   {t_c2r - t_split:9.3f}",
          f"  triple sums                                {t_sums:9.3f}",
          f"    LDS reads 3 M T 8 B = {lds_bytes:.3e} B: {rate / 1e12:.1f} TB/s = {rate / (CUS * CLK):.1f} B/clk/CU at 2.4 GHz on 256 CUs, "
          f"{100 * rate / (CUS * CLK * LDS_RATE):.0f} % of the {LDS_RATE:.0f} B/clk/CU of ds_read_b64"]
del shells, fields, work
torch.cuda.empty_cache()

kw = dict(box_size=box, kedges=list(edges), triangles=tri)
metrics.bispectrum(meshes[0], **kw)      # fills the triangle-count cache
t_one = median_ms(lambda: metrics.bispectrum(meshes[0], **kw))
t_eight = median_ms(lambda: metrics.bispectrum(meshes, **kw))
metrics._NTRI_CACHE.clear()
t_cold = median_ms(lambda: (metrics._NTRI_CACHE.clear(), metrics.bispectrum(meshes[0], **kw)), reps=3)
lines += [f"  metrics.bispectrum, one mesh               {t_one:9.3f}",
          f"  metrics.bispectrum, one mesh, counts not cached {t_cold:9.3f}",
          f"  metrics.bispectrum, batch of 8             {t_eight:9.3f}   ({t_eight / 8:.3f} per mesh)"]

# plain torch on the same device: masked irfftn per bin, one product-sum per triangle
kx, ky, kz = nbody.rfftk(shape, box)
dig = torch.from_numpy(np.digitize(np.sqrt((kx ** 2 + ky ** 2) + kz ** 2), edges) - 1).to(dev)
zero = torch.zeros((), dtype=torch.complex64, device=dev)


def torch_fields(m):
    d = torch.fft.rfftn(m)
    return torch.stack([torch.fft.irfftn(torch.where(dig == b, d, zero), s=shape) * M for b in range(n_bins)])


def torch_sums(F):
    return torch.stack([(F[i] * F[j] * F[l]).sum(dtype=torch.float64) for i, j, l in tri.tolist()])


def torch_whole(m):
    return torch_sums(torch_fields(m)).cpu()


F = torch_fields(meshes[0])
t_tf = median_ms(lambda: torch_fields(meshes[0]))
t_ts = median_ms(lambda: torch_sums(F))
del F
t_tw = median_ms(lambda: torch_whole(meshes[0]))
t_tw8 = median_ms(lambda: [torch_whole(meshes[i]) for i in range(8)], reps=3)
lines += ["plain torch restatement (float32 fields, float64 sums), same device",
          f"  rfftn + {n_bins} masked irfftn                    {t_tf:9.3f}",
          f"  {T} product-sums                          {t_ts:9.3f}",
          f"  whole, one mesh                            {t_tw:9.3f}",
          f"  whole, 8 meshes one after another          {t_tw8:9.3f}   ({t_tw8 / 8:.3f} per mesh)"]
got = metrics._triple_sums(meshes[:1], True, shape, ktab, None, edges, np.sort(tri, axis=1))[0]
want = torch_whole(meshes[0]).numpy()
lines.append(f"  largest |S - S_torch| / max |S_torch| between the two: {np.max(np.abs(got - want)) / np.max(np.abs(want)):.2e}")
text = "\n".join(lines) + "\n"
print(text, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
