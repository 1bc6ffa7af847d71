"""FieldLevelLogDensity on the HIP path against the composed float64 reference tests/_model_f64.py over the feature mixes of
tests/_model_cases.py: a table in which every valid pair of (evolution / time, bias_type, png_type, ap_auto, lik_type, survey, precond,
sampled s_ep, temp_lik) occurs.  Each feature's own test holds it alone, or beside one neighbour; here the branches of `evolve`,
`evolve_vjp` and `cosmo_vjp` run together, where a cotangent overwritten instead of accumulated, a context field the second feature
clobbers or a table Jacobian dropped would bias a posterior and show nowhere else.  The gates are those of
tests/test_gpu_model.py::test_log_density_and_gradient; the steps of the central differences are the table's, each held to its own half
by tests/test_model_f64_host.py."""
import numpy as np
import pytest

import _model_cases as C

pytestmark = pytest.mark.gpu


def _same(a, b):
    import torch
    return torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b)


@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_log_density_and_gradient_of_a_feature_mix(gpu, c):
    from montecosmo_amd import bricks, logdensity, model, nbody
    b = C.build(c)
    fid = bricks.Planck18(Omega_c=C.OM_FID - 0.0490) if c["ap_auto"] else None
    fwd = model.FieldLevelForward(cosmo_fid=fid, **C.forward_kwargs(c))
    ld = logdensity.FieldLevelLogDensity(fwd, b["obs"], b["lat"], b["fixed"], precond=c["precond"], lik_type=c["lik_type"], **b["extra"])
    sample, temp = b["sample"], c["temp"]
    s32 = {k: (v if (np.ndim(v) == 0 or k == "ngbars_") else v.astype(np.float32)) for k, v in sample.items()}
    lp, grad = ld.logdensity_and_grad(s32, temp_lik=temp)
    lp2, grad2 = ld.logdensity_and_grad(s32, temp_lik=temp)
    assert lp == lp2 and set(grad) == set(grad2) == set(ld.names()) and all(_same(grad[k], grad2[k]) for k in grad)
    lp_o = b["ref"](sample)
    print(f"\n{C.case_id(c)}: lp {lp:.6f} float64 {lp_o:.6f} |lp - lp_o| {abs(lp - lp_o):.3e} of the gate {2e-4 * abs(lp_o) + 0.05:.3e}")
    assert np.isfinite(lp_o) and abs(lp - lp_o) < 2e-4 * abs(lp_o) + 0.05, (lp, lp_o)
    worst = ("", 0.)
    for name, idx in C.scalar_names(b):
        fd = C.central_difference(b, name, idx, b["h"][name])
        g = grad[name + "_"] if idx is None else grad[name + "_"][idx]
        ratio = abs(fd - g) / (1e-2 * abs(fd) + 1e-3)
        worst = max(worst, (f"{name}{'' if idx is None else idx}", ratio), key=lambda t: t[1])
        print(f"  {name}{'' if idx is None else idx}: fd {fd:.6f} got {g:.6f} ({ratio:.3f} of the gate)")
        assert abs(fd - g) < 1e-2 * abs(fd) + 1e-3, (name, idx, fd, g)
    fd = C.central_difference(b, "white_mesh", None, b["h"]["white_mesh"])
    gw, d = grad["white_mesh_"].double().cpu().numpy(), b["direction"]
    an = float((gw * d).sum())
    typical = np.linalg.norm(gw) * np.linalg.norm(d) / np.sqrt(d.size)      # |<g, d>| for a random direction
    ratio = abs(fd - an) / (5e-3 * max(abs(fd), typical))
    worst = max(worst, ("white_mesh", ratio), key=lambda t: t[1])
    print(f"  white_mesh_: fd {fd:.6f} got {an:.6f} typical {typical:.4f} ({ratio:.3f} of the gate)")
    print(f"  worst gradient: {worst[0]} at {worst[1]:.3f} of its gate")
    assert abs(fd - an) < 5e-3 * max(abs(fd), typical), ("white_mesh_", fd, an, typical)
    if temp != 1.:
        # the stages: prior and forward model do not see the temperature; the likelihood alone carries it
        lik = ld._lik_quad_gauss if c["lik_type"] == "quad_gauss" else ld._lik_hip
        prior, base, _, _ = ld._prior(s32)
        w = nbody._f32(s32["white_mesh_"], fwd.init_shape)
        prior += ld._white_prior(w)
        f = ld._forward(base, w, need_ctx=True, need_phi=True)
        f1 = ld._forward(base, w, need_ctx=True, need_phi=True)
        assert f.temp == 1. and _same(f.cm, f1.cm) and _same(f.gxy, f1.gxy) and (f.phi is None or _same(f.phi, f1.phi))
        cold = lik(base, f1, False)[0]
        f.temp = temp
        hot = lik(base, f, False)[0]
        assert prior + cold == ld.logdensity_and_grad(s32, need_grad=False, temp_lik=1.)[0]
        assert prior + hot == lp and hot != cold
