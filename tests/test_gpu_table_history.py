"""The table store (montecosmo_amd/tables.py) keeps nothing a result could depend on: a log density and its gradient at one cosmology are
bitwise the same before and after the store has been filled past its bound with other cosmologies' tables, so that every table of the first
has been evicted and is built and uploaded again.  Shapes and set-up are those of tests/_model_cases.py."""
import numpy as np
import pytest

import _model_cases as C

pytestmark = pytest.mark.gpu

LIGHTCONE = next(c for c in C.CASES if c["evo"] == "lpt_lc" and c["ap_auto"] is True and c["png_type"] is not None)
FIXED_A = next(c for c in C.CASES if c["evo"] == "lpt" and c["ap_auto"] is True and c["png_type"] is not None)


# without lin_kpow the power table is the Eisenstein & Hu one of the current cosmology: it moves with Omega_m, and cosmo_vjp's pair asks for two more
@pytest.mark.parametrize("c,eisenstein_hu", [(LIGHTCONE, True), (LIGHTCONE, False), (FIXED_A, True), (FIXED_A, False)],
                         ids=lambda v: C.case_id(v) if isinstance(v, dict) else ("eh" if v else "kpow"))
def test_results_do_not_depend_on_the_stores_history(gpu, monkeypatch, c, eisenstein_hu):
    import torch
    from montecosmo_amd import bricks, logdensity, model, tables
    b = C.build(c)
    kw = dict(C.forward_kwargs(c), cosmo_fid=bricks.Planck18(Omega_c=C.OM_FID - 0.0490))
    if eisenstein_hu:
        kw["lin_kpow"] = None
    fwd = model.FieldLevelForward(**kw)
    ld = logdensity.FieldLevelLogDensity(fwd, b["obs"], b["lat"], b["fixed"], precond=c["precond"], lik_type=c["lik_type"], **b["extra"])
    s32 = {k: (v if (np.ndim(v) == 0 or k == "ngbars_") else v.astype(np.float32)) for k, v in b["sample"].items()}
    lp, grad = ld.logdensity_and_grad(s32, temp_lik=c["temp"])
    for i in range(1, tables.BOUND + 2):      # more distinct Omega_m than the store holds entries
        lp_i, _ = ld.logdensity_and_grad(dict(s32, Omega_m_=s32["Omega_m_"] + 0.05 * i), temp_lik=c["temp"])
        assert np.isfinite(lp_i) and lp_i != lp
    assert len(tables._STORE) == tables.BOUND
    uploads, upload = [], tables.upload
    monkeypatch.setattr(tables, "upload", lambda array, device: uploads.append(len(array)) or upload(array, device))
    lp2, grad2 = ld.logdensity_and_grad(s32, temp_lik=c["temp"])
    assert uploads      # the first call's tables had been evicted: they were built again
    assert lp2 == lp and set(grad2) == set(grad)
    for k in grad:
        assert torch.equal(grad[k], grad2[k]) if torch.is_tensor(grad[k]) else np.array_equal(grad[k], grad2[k]), k
