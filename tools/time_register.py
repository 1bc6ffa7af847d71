"""Times the catalogue passes and the whole cut-sky register_catalog on synthetic randoms (default 2^24):

    python tools/time_register.py [--n 16777216] [--out profiles/register_catalog.txt]

torch.cuda.Event medians over 5 runs (after one warm-up) of each coordinate kernel, the footprint and the masked sum, with the
bytes each moves per object against the 6.3 TB/s a streaming copy reaches on this part, then the host numpy float64
conversion of the same arrays (numpy's sin, cos and interp run on one thread, so on one thread and split over a pool of at most
16) and register_catalog end to end."""
import argparse
import concurrent.futures
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COPY_TBS = 6.3


def median_ms(fn, runs=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from montecosmo_amd import bricks, nbody, register, tables
    n = a.n
    rng = np.random.default_rng(0)
    rnd = {'RA': rng.uniform(100, 140, n), 'DEC': np.rad2deg(np.arcsin(rng.uniform(np.sin(np.deg2rad(10)), np.sin(np.deg2rad(40)), n))),
           'Z': rng.uniform(0.4, 0.7, n), 'WEIGHT': rng.uniform(0.5, 1.5, n)}
    cosmo = bricks.Planck18()
    lines = [f"register_catalog passes, {n} synthetic randoms, {torch.cuda.get_device_name(0)}; medians of 5 runs; "
             f"streaming copy = {COPY_TBS} TB/s"]

    lo, hi, _ = bricks.sky_extent(cosmo, rnd)
    size, center = hi - lo, (lo + hi) / 2
    shape, cell = bricks.get_mesh_shape(size, 256 ** 3, 0.2)
    box = np.multiply(shape, cell)
    dev = nbody._device()
    ra, dec, z, w = (torch.from_numpy(rnd[k]).to(dev) for k in ('RA', 'DEC', 'Z', 'WEIGHT'))
    dist = tables.on_device(cosmo, tables.DISTANCE, dev)
    tab, nt = dist.t, dist.n["a_dist"]
    geom = bricks._cell_geom(center, np.zeros(3), box, shape)
    plan = nbody.get_plan(shape)
    out7 = torch.empty(7, dtype=torch.float64, device=dev)
    pos, pos2 = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
    ratio = np.array([0.5, 0.5, 0.5])
    p64 = torch.from_numpy(rng.uniform(0, 1000, (n, 3))).to(dev)
    v64 = torch.from_numpy(rng.standard_normal((n, 3))).to(dev)
    gbox = bricks._cell_geom((500., 500., 500.), np.zeros(3), (1000.,) * 3, shape)
    los = np.array([0., 0., 1.])
    w32 = w.float()
    mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    mesh = torch.rand(shape, dtype=torch.float32, device=dev)
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    M = int(np.prod(shape))
    cases = [
        ("sky2cart_minmax_f64", 32 * n, lambda: plan.call("mcpm_sky2cart_minmax_f64", ra, dec, z, n, tab, tab[nt:], nt, w, out7, out7[6:])),
        ("sky2cell_f32", 36 * n, lambda: plan.call("mcpm_sky2cell_f32", ra, dec, z, n, tab, tab[nt:], nt, geom, None, pos, None)),
        ("sky2cell_f32 (two outputs)", 48 * n, lambda: plan.call("mcpm_sky2cell_f32", ra, dec, z, n, tab, tab[nt:], nt, geom, ratio, pos, pos2)),
        ("box2cell_f32 (f64 pos + vel)", 60 * n, lambda: plan.call("mcpm_box2cell_f32", p64, v64, 1, n, gbox, los, 0.01, pos2)),
        ("footprint_u8 (order 2, bytes: lower bound)", 16 * n + M, lambda: plan.call("mcpm_footprint_u8", pos, n, w32, 2, mask, 0)),
        ("masked_sum_f64", 5 * M, lambda: plan.call("mcpm_masked_sum_f64", mesh, mask, M, out2)),
    ]
    plan.call("mcpm_sky2cell_f32", ra, dec, z, n, tab, tab[nt:], nt, geom, None, pos, None)      # the footprint's positions
    for name, nbytes, fn in cases:
        ms = median_ms(fn)
        tbs = nbytes / (ms * 1e-3) / 1e12
        lines.append(f"  {name:42s} {ms:9.4f} ms  {tbs:6.3f} TB/s = {100 * tbs / COPY_TBS:5.1f} % of a streaming copy (mesh {shape})")

    lines.append("  (footprint bytes: positions, weights and the clearing of the mask; the up to 8 scattered byte stores per object are not counted)")

    def host(lo, hi):
        cart = bricks.radecz2cart(cosmo, {k: rnd[k][lo:hi] for k in ('RA', 'DEC', 'Z')})
        return bricks.phys2cell_pos(cart, center, np.zeros(3), box, shape).astype(np.float32)
    t0 = time.perf_counter()
    cells = host(0, n)
    t_one = time.perf_counter() - t0
    workers = min(16, len(os.sched_getaffinity(0)))
    cuts = np.linspace(0, n, workers + 1).astype(int)
    with concurrent.futures.ThreadPoolExecutor(workers) as pool:
        t0 = time.perf_counter()
        parts = list(pool.map(host, cuts[:-1], cuts[1:]))
        t_pool = time.perf_counter() - t0
    assert sum(len(p) for p in parts) == len(cells)
    lines.append(f"  host numpy float64 radecz2cart + phys2cell_pos of the same arrays: {1e3 * t_one:.1f} ms on one thread, "
                 f"{1e3 * t_pool:.1f} ms split over {workers} threads")

    def whole():
        return register.register_catalog(64 ** 3, cosmo, {k: v[:n // 8] for k, v in rnd.items()}, rnd, padding=0.2)
    reg = whole()
    ms = median_ms(whole)
    lines.append(f"  register_catalog cut sky, {n} randoms + {n // 8} data, cell_budget 64^3 -> final {reg['count_mesh'].shape}: "
                 f"median {ms:.1f} ms (host checks, uploads and downloads included)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
