"""The stages of the log density (montecosmo_amd/logdensity.py): the one prior function against the functions it calls (host only), the two
FFT adjoint helpers of nbody.py against the sequences they replaced and against the adjoint identity, and the one forward preamble that
`mean_counts` and `logdensity_and_grad` share.

Tolerance of the adjoint identities: tests/test_gpu_spectral.py (test_fft_batches_abi) holds mcpm_fft_r2c / mcpm_fft_c2r, which are all
`rfftn` / `irfftn` and their adjoints run, to a relative L2 error of 2e-6.  An inner product <a, b> whose factor a carries a relative L2 error
eps is off by at most eps |a| |b| (Cauchy-Schwarz); each side of <A x, s> = <x, A^T s> has one transformed factor, so the two sides, summed in
float64 from the float32 outputs, agree within 2e-6 (|A x| |s| + |x| |A^T s|)."""
import math

import numpy as np
import pytest

FFT_REL_L2 = 2e-6      # tests/test_gpu_spectral.py::test_fft_batches_abi

NORMAL = dict(loc=1., scale=10., loc_fid=0.8, scale_fid=1e-2, low=-math.inf, high=math.inf)
TRUNC = dict(loc=0.8102, scale=0.1, loc_fid=0.8102, scale_fid=1e-2, low=0., high=math.inf)
UNIF = dict(low=-1., high=1.5, loc_fid=0.25, scale_fid=2.5 / 12 ** .5)
XS = (-13., -2., 0., 0.7, 13.)


def _old(kind, x, c):
    from montecosmo_amd import logdensity as ld
    if kind == "unif":
        return ld.detrunc_unif_log_prob_and_grad(x, c)
    if kind == "trunc":
        return ld.detrunc_truncnorm_log_prob_and_grad(x, c)
    mu, sd = (c["loc"] - c["loc_fid"]) / c["scale_fid"], c["scale"] / c["scale_fid"]      # the closed normal form
    return -0.5 * ld.LOG2PI - math.log(sd) - 0.5 * ((x - mu) / sd) ** 2, -(x - mu) / sd ** 2, x * c["scale_fid"] + c["loc_fid"], c["scale_fid"]


def _host_density(latents, fixed, ngb_lat=None):
    """A log-density object as far as its prior stage reads it (no device, no forward model)."""
    from montecosmo_amd import logdensity
    ld = logdensity.FieldLevelLogDensity.__new__(logdensity.FieldLevelLogDensity)
    ld.latents, ld.fixed, ld.ngb_lat = latents, fixed, ngb_lat
    ld.n_rbins = 0 if ngb_lat is None else len(ngb_lat["loc_fid"])
    return ld


@pytest.mark.parametrize("kind,c", [("normal", NORMAL), ("trunc", TRUNC), ("unif", UNIF)])
def test_prior_function_returns_what_the_per_kind_functions_return(kind, c):
    from montecosmo_amd import logdensity
    ld = _host_density({"p": c}, {"q": 3.})
    for x in XS:
        got, want = logdensity.latent_log_prob_and_grad(x, c), _old(kind, x, c)
        assert len(got) == 4 and all(g == w for g, w in zip(got, want)), (kind, x, got, want)
        base = ld.base_params({"p_": x})
        assert base["p"] == got[2] and base["q"] == 3.


def test_per_shell_ngbars_prior_is_three_scalar_priors():
    from montecosmo_amd import logdensity
    ngb = {"loc": np.array([1e-3, 1.4e-3, 0.9e-3]), "scale": np.array([1e-2, 2e-2, 1e-2]), "loc_fid": np.array([1e-3, 1.4e-3, 1e-3]),
           "scale_fid": np.array([1e-5, 2e-5, 1e-5]), "low": np.array([0., 0., -math.inf]), "high": np.full(3, math.inf)}
    ld = _host_density({}, {"q": 3.}, ngb)
    xs = np.array([-2., 0.7, 13.])
    lp, base, grad, dbase = ld._prior({"ngbars_": xs})
    each = [logdensity.latent_log_prob_and_grad(float(xs[i]), {k: float(v[i]) for k, v in ngb.items()}) for i in range(3)]
    assert lp == (0.0 + each[0][0]) + each[1][0] + each[2][0]
    for i in range(3):
        assert (grad["ngbars_"][i], base["ngbars"][i], dbase["ngbars"][i]) == each[i][1:]
    assert np.array_equal(ld.base_params({"ngbars_": xs})["ngbars"], base["ngbars"])


def _pair(a, b):
    """The real-pair inner product of two complex arrays, in float64."""
    a, b = a.cpu().numpy().astype(np.complex128), b.cpu().numpy().astype(np.complex128)
    return float((a.real * b.real + a.imag * b.imag).sum())


def _norm(a):
    return float(np.linalg.norm(a.cpu().numpy().astype(np.complex128 if a.is_complex() else np.float64)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 6, 8), (6, 8, 10)])      # unequal even sides: every face, edge and corner plane of the half spectrum
def test_fft_adjoint_helpers(gpu, shape):
    import torch
    from montecosmo_amd import nbody
    from montecosmo_amd.utils import r2chshape
    gen = torch.Generator(device="cuda").manual_seed(5)
    cshape, M = r2chshape(shape), float(np.prod(shape))
    x, y = (torch.randn(shape, device="cuda", generator=gen) for _ in range(2))
    s, S = (torch.complex(torch.randn(cshape, device="cuda", generator=gen), torch.randn(cshape, device="cuda", generator=gen)) for _ in range(2))
    # rfftn_vjp: clone, halve the modes the C2R counts twice, unnormalised C2R into a fresh mesh
    kb = s.clone()
    kb[..., 1:shape[-1] // 2] *= 0.5
    want = torch.empty(shape, dtype=torch.float32, device="cuda")
    nbody.get_plan(shape).call("mcpm_fft_c2r", nbody._ptr(kb), nbody._ptr(want), 1)
    s_in = s.clone()
    got = nbody.rfftn_vjp(s)
    assert torch.equal(got, want) and torch.equal(s, s_in)      # (the argument is left as it was)
    assert torch.equal(nbody.rfftn_vjp(s.clone(), overwrite=True), want)
    X = nbody.rfftn(x)
    lhs, rhs = _pair(X, s), float((x.double() * got.double()).sum())
    print(f"\n{shape} rfftn: <rfftn x, s> {lhs:.9e}  <x, rfftn_vjp s> {rhs:.9e}  bound {FFT_REL_L2 * (_norm(X) * _norm(s) + _norm(x) * _norm(got)):.3e}")
    assert abs(lhs - rhs) <= FFT_REL_L2 * (_norm(X) * _norm(s) + _norm(x) * _norm(got))
    # irfftn_vjp: rfftn / M, then double the modes that stand for themselves and their mirror image
    want = nbody.rfftn(y) / M
    want[..., 1:shape[-1] // 2] *= 2.0
    got = nbody.irfftn_vjp(y)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(want))
    Y = nbody.irfftn(S)
    lhs, rhs = float((Y.double() * y.double()).sum()), _pair(S, got)
    print(f"{shape} irfftn: <irfftn S, y> {lhs:.9e}  <S, irfftn_vjp y> {rhs:.9e}  bound {FFT_REL_L2 * (_norm(Y) * _norm(y) + _norm(S) * _norm(got)):.3e}")
    assert abs(lhs - rhs) <= FFT_REL_L2 * (_norm(Y) * _norm(y) + _norm(S) * _norm(got))


@pytest.mark.gpu
@pytest.mark.parametrize("survey", [True, False])
def test_mean_counts_is_the_count_mesh_of_the_log_density(gpu, survey):
    """Both go through `_forward`: mean_counts(sample)[0] is bitwise the cm the likelihood of logdensity_and_grad is evaluated on."""
    import torch
    from test_gpu_likelihood import _model
    m = _model("lpt", "quad_gauss", survey, False, stoch_fixed=dict(s_ed=0.3, s_e2=0.))
    ld, s = m["mk"](m["obs"]), m["dev_sample"](m["sample"])
    seen = {}
    lik = ld._lik_quad_gauss
    ld._lik_quad_gauss = lambda base, f, need_grad: seen.update(cm=f.cm.clone(), selec=f.selec) or lik(base, f, need_grad)
    lp, _ = ld.logdensity_and_grad(s)
    cm, selec = ld.mean_counts(s)
    assert np.isfinite(lp) and tuple(cm.shape) == (8, 8, 8) and bool(cm.abs().sum() > 0)
    assert torch.equal(cm, seen["cm"])
    assert torch.equal(selec, seen["selec"]) if survey else selec == seen["selec"]
    assert torch.equal(cm, ld._forward(ld.base_params(s), s["white_mesh_"], need_ctx=True).cm)
