"""Prints, for every feature mix of tests/_model_cases.py, a SHA-256 of the HIP log density and of each gradient array's bytes: two trees
that compute the same bits print the same lines.  The mixes with png_type and ap_auto=True run once more without `lin_kpow`, on the
Eisenstein & Hu power of the sampled cosmology.
usage: python tools/dump_model_cases.py        (from the repository root)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _model_cases as C      # noqa: E402
from montecosmo_amd import bricks, logdensity, model      # noqa: E402


def sha(x):
    x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:16] + f" {x.dtype}{list(x.shape)}"


for c, kpow in [(c, True) for c in C.CASES] + [(c, False) for c in C.CASES if c["png_type"] and c["ap_auto"] is True]:
    b = C.build(c)
    fid = bricks.Planck18(Omega_c=C.OM_FID - 0.0490) if c["ap_auto"] else None
    fwd = model.FieldLevelForward(cosmo_fid=fid, **(C.forward_kwargs(c) if kpow else dict(C.forward_kwargs(c), lin_kpow=None)))
    ld = logdensity.FieldLevelLogDensity(fwd, b["obs"], b["lat"], b["fixed"], precond=c["precond"], lik_type=c["lik_type"], **b["extra"])
    s32 = {k: (v if (np.ndim(v) == 0 or k == "ngbars_") else v.astype(np.float32)) for k, v in b["sample"].items()}
    lp, grad = ld.logdensity_and_grad(s32, temp_lik=c["temp"])
    print(C.case_id(c) + ("" if kpow else " (Eisenstein & Hu)"))
    print(f"  lp {sha(np.float64(lp))} {lp!r}")
    for k in sorted(grad):
        print(f"  {k} {sha(grad[k])}", flush=True)
