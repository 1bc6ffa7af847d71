"""Times the integrator work of one MCLMC transition (three velocity updates, two drifts, the partial refresh, the energy read-back) through
the 'torch' and the 'hip' back end of `samplers.make_integrator`, with and without `inverse_mass`.
usage: python tools/time_mclmc.py [out=profiles/mclmc_integrator.txt] [d ...]      (default d: 96^3 + 3 and 219^3 + 3, the init meshes of
final 64^3 and 146^3 plus three scalars)
The log density is a device Gaussian stub that ends in a host read, as `FlatLogDensity` does.  A window times N whole transitions with a host
clock that ends in a device synchronise, then N times two stub calls alone; the difference over N is the integrator's time per transition.
The four variants alternate inside every repeat; the figure is the median of 5 repeats, with the spread beside it."""
import math
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from montecosmo_amd import samplers  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/mclmc_integrator.txt"
dims = [int(a) for a in sys.argv[2:]] or [96 ** 3 + 3, 219 ** 3 + 3]
REPEATS = 5
# time of one log density + gradient at the model whose init mesh gives this d, for the share printed below
GRADIENT_MS = {96 ** 3 + 3: (3.0, "final 64^3, evolution='lpt'; `tools/run_mclmc_field.py --final-n 64 --n-chains 3 --thinning 32`, timed, spent 3.018 ms per "
                             "gradient of its run phase through 'hip' and 3.185 through 'torch', integrator included"),
               219 ** 3 + 3: (26.9, "final 146^3, evolution='nbody' on a 256^3 mesh: README, BASELINE config 5")}
if not torch.cuda.is_available():
    raise SystemExit("time_mclmc.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


lines = [f"MCLMC integrator work per transition, {torch.cuda.get_device_name(0)}; median of {REPEATS} windows (min .. max), microseconds",
         "transition = 3 x B + 2 x A + partial refresh + energy read-back; the Gaussian stub's two calls are timed alone and subtracted",
         ""]
verdict = {}
for d in dims:
    gen = torch.Generator(device=dev).manual_seed(d)
    sd = torch.exp(torch.rand(d, device=dev, generator=gen) - 0.5)
    inv_var = (1.0 / (sd * sd)).float()
    q0 = (sd * torch.randn(d, device=dev, generator=gen)).float()
    inverse_mass = (sd * sd).float()

    def stub(q):
        g = -(q * inv_var)
        return float(0.5 * torch.dot(q, g)), g

    n = 200 if d < 4_000_000 else 60
    eps, L = 0.3 * math.sqrt(d) / 30.0, math.sqrt(d)
    variants = [(b, p) for p in (False, True) for b in ("torch", "hip")]
    chains = {}
    for b, p in variants:
        integ = samplers.make_integrator(q0, inverse_mass if p else None, b)
        rng = samplers._Rng(1)
        lp, g = stub(q0)
        st = {"q": q0.clone(), "u": samplers._unit_normal(q0, rng), "lp": lp, "g": g}
        chains[(b, p)] = (integ, st, rng)

    def transition(key):
        integ, st, rng = chains[key]
        dE = samplers._mclmc_transition(integ, stub, st, eps, L, rng)
        assert math.isfinite(dE)

    def stubs_only():
        stub(q0)
        stub(q0)

    for key in variants:      # warm up every shape and code path the windows use
        for _ in range(5):
            transition(key)
    stubs_only()
    times = {key: [] for key in variants}
    stub_t = []
    for _ in range(REPEATS):
        s = window(stubs_only, n)
        stub_t.append(s)
        for key in variants:
            times[key].append(window(lambda: transition(key), n) - s)
    lines.append(f"d = {d}  ({n} transitions per window; two stub calls alone: {1e6 * statistics.median(stub_t):.0f} us)")
    med = {}
    for b, p in variants:
        t = [1e6 * x for x in times[(b, p)]]
        med[(b, p)] = statistics.median(t)
        lines.append(f"  backend={b:5s} inverse_mass={'yes' if p else 'no ':3s}  {med[(b, p)]:9.1f}  ({min(t):.1f} .. {max(t):.1f})")
    for p in (False, True):
        r = med[("torch", p)] / med[("hip", p)]
        verdict[(d, p)] = r
        lines.append(f"  torch / hip, inverse_mass={'yes' if p else 'no'}: {r:.2f}x")
    if d in GRADIENT_MS:
        ms, src = GRADIENT_MS[d]
        lines.append(f"  share of a gradient ({ms} ms: {src}), an ESTIMATE from two separate measurements (half a transition's integrator time over one gradient):")
        for b, p in variants:
            lines.append(f"    backend={b:5s} inverse_mass={'yes' if p else 'no ':3s}  {100 * 0.5e-3 * med[(b, p)] / ms:5.2f} %")
    lines.append("")
ok = all(r >= 1.0 for r in verdict.values())
lines.append("condition (the HIP path is not slower than the torch path at every size): " + ("MET, backend='auto' resolves to 'hip'" if ok else
             "NOT MET: backend='auto' must resolve to 'torch'"))
text = "\n".join(lines) + "\n"
print(text)
open(out_path, "w").write(text)
