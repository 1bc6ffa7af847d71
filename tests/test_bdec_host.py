"""montecosmo_amd/bdec.py on the host backend (no GPU): against the independent float64 restatement tests/_bdec_f64.py, against known answers,
the shapes of every output, the declaration of the new entry point, the backend rules and the Chains methods.

The host backend and the restatement evaluate the same float64 formulas from the same sorted values, so the unweighted results are compared
exactly; the weighted and ord = 2 results, whose sums the two write in different ways (np.cumsum against a running sum), at 1e-12."""
import os

import numpy as np
import pytest
import torch

import _bdec_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bd():
    from montecosmo_amd import bdec
    return bdec


def _draws(seed, shape, dtype=np.float64):
    return np.random.default_rng(seed).standard_normal(shape).astype(dtype)


P_CASES = [.3, [.05, .5, .95], [[0., .25, 1.], [.5, .75, .999]]]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("p", P_CASES)
def test_quantile_and_qbci_against_restatement(bd, dtype, p):
    x = _draws(1, (3, 41, 2, 5), dtype)
    pooled = x.reshape(3 * 41, 10).astype(np.float64)
    q = bd.quantile(x, p, axis=(0, 1), backend="host")
    assert q.dtype == np.float64 and q.shape == np.shape(p) + (2, 5)
    np.testing.assert_array_equal(q.reshape(np.shape(p) + (10,)), ref.quantile(pooled, p))
    for kind in ("low", "med", "high"):
        ci = bd.qbci(x, p, axis=(0, 1), type=kind, backend="host")
        assert ci.shape == np.shape(p) + (2, 5, 2)
        np.testing.assert_array_equal(ci.reshape(np.shape(p) + (10, 2)), ref.qbci(pooled, p, kind))
        np.testing.assert_array_equal(bd.credint(x, p, axis=(0, 1), type=kind, backend="host"), ci)
    # one axis, and an axis that is not the first
    np.testing.assert_array_equal(bd.quantile(x[0], p, backend="host").reshape(np.shape(p) + (10,)), ref.quantile(pooled[:41], p))
    y = np.moveaxis(x[0], 0, -1)      # (2, 5, 41)
    np.testing.assert_array_equal(bd.quantile(y, p, axis=-1, backend="host"), bd.quantile(x[0], p, backend="host"))
    # 'auto' without a float32 GPU case to take is the host
    if dtype == np.float64:
        np.testing.assert_array_equal(bd.quantile(x, p, axis=(0, 1)), q)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,p", [(1, .95), (2, .95), (3, .5), (40, .95), (41, .5), (64, 0.), (64, 1.), (10, .25)])
def test_sci_noweights_against_restatement(bd, dtype, n, p):
    x = _draws(2, (n, 3, 4), dtype)
    ci, idx = bd.sci_noweights(x, p, backend="host", return_index=True)
    low, high, i = ref.sci_noweights(x.reshape(n, 12).astype(np.float64), p)
    assert ci.shape == (3, 4, 2) and ci.dtype == np.float64 and idx.shape == (3, 4) and idx.dtype == np.int32
    np.testing.assert_array_equal(ci[..., 0].reshape(-1), low)
    np.testing.assert_array_equal(ci[..., 1].reshape(-1), high)
    np.testing.assert_array_equal(idx.reshape(-1), i)
    np.testing.assert_array_equal(bd.credint(x, p, backend="host"), ci)
    with pytest.raises(TypeError):
        bd.sci_noweights(x, [.5, .9], backend="host")


def test_total_order_and_nan_rows(bd):
    x = np.array([[0., -0., 1.], [-0., np.inf, np.nan], [0., -np.inf, 2.], [-0., 3., -np.nan], [5., np.inf, 0.]], dtype=np.float32)
    s = bd.sort_draws(x, backend="host")
    want = ref.sort_total(x.astype(np.float64))
    np.testing.assert_array_equal(s, want)
    np.testing.assert_array_equal(np.signbit(s), np.signbit(want))
    assert list(np.signbit(s[:, 0])) == [True, True, False, False, False]      # -0 -0 +0 +0 5
    assert np.isnan(s[3:, 2]).all() and not np.signbit(s[3:, 2]).any() and s[0, 1] == -np.inf
    ci, idx = bd.sci_noweights(x, .5, backend="host", return_index=True)
    assert np.isnan(ci[2]).all() and idx[2] == -1 and not np.isnan(ci[:2]).any()
    low, high, i = ref.sci_noweights(x.astype(np.float64), .5)
    np.testing.assert_array_equal(ci[:, 0], low)
    np.testing.assert_array_equal(ci[:, 1], high)
    np.testing.assert_array_equal(idx, i)
    np.testing.assert_array_equal(bd.quantile(x, [.2, .5, 1.], backend="host"), ref.quantile(x.astype(np.float64), [.2, .5, 1.]))
    below, equal = bd.rank_counts(x, np.array([0., np.inf, 1.5]), backend="host")
    np.testing.assert_array_equal(below, [0, 3, 2])
    np.testing.assert_array_equal(equal, [4, 2, 0])
    b, e = ref.counts(x, [0., np.inf, 1.5])
    np.testing.assert_array_equal(below, b)
    np.testing.assert_array_equal(equal, e)


def test_known_answers(bd):
    n = 11
    x = np.arange(n, dtype=np.float64)
    p = np.array([0., .1, .25, .5, .77, 1.])
    # cdf_k = (k + 1) / n is linear in x = k: between the clipped ranks q = n p - 1, and x_(0) below cdf_0
    closed = np.clip(n * p - 1., 0., n - 1.)
    np.testing.assert_allclose(bd.quantile(x, p, backend="host"), closed, rtol=0, atol=1e-13)
    y = _draws(3, (57, 6))
    np.testing.assert_array_equal(bd.quantile(y, [0., 1.], backend="host"), np.stack([y.min(axis=0), y.max(axis=0)]))
    lo = bd.credint(y, .9, type="low", backend="host")
    hi = bd.credint(y, .9, type="high", backend="host")
    np.testing.assert_array_equal(lo[:, 0], y.min(axis=0))
    np.testing.assert_array_equal(hi[:, 1], y.max(axis=0))
    np.testing.assert_array_equal(lo[:, 1], bd.quantile(y, .9, backend="host"))
    np.testing.assert_allclose(hi[:, 0], bd.quantile(y, .1, backend="host"), rtol=0, atol=1e-13)      # 1 - .9 is .1 to 2^-55 only; times n = 57, times a spacing below 4
    # one tight cluster of 80 and 20 far outliers: the smallest 80 % interval is the cluster
    rng = np.random.default_rng(4)
    cluster = 3. + 1e-3 * rng.standard_normal(80)
    far = np.concatenate([-50. - 10. * rng.random(10), 60. + 10. * rng.random(10)])
    z = rng.permutation(np.concatenate([cluster, far]))
    ci = bd.sci_noweights(z, .79, backend="host")
    assert ci.shape == (2,) and cluster.min() <= ci[0] and ci[1] <= cluster.max()
    np.testing.assert_array_equal(bd.sci_noweights(z, .79, backend="host"), bd.credint(z, .79, backend="host"))


def test_weights_and_ord2(bd):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((9, 4))
    w = rng.integers(1, 4, 9)
    # integer weights = repeated samples, at the knots of the cdf (p = cumsum(w) / sum(w) of each column's order): there both cdfs pass
    # through the same points.  Between two knots they differ by construction: the weighted cdf rises linearly over the whole step
    # w_i / W up to x_(i), the repeated sample's over its first 1 / W and then stays at x_(i).
    rep = np.repeat(x, w, axis=0)
    for c in range(4):
        knots = np.cumsum(w[np.argsort(x[:, c])]) / w.sum()
        weighted, repeated = bd.quantile(x[:, c], knots, weights=w, backend="host"), bd.quantile(rep[:, c], knots, backend="host")
        np.testing.assert_allclose(weighted, repeated, rtol=1e-14, atol=0)      # (a few roundings of the interpolation each)
        np.testing.assert_allclose(weighted, np.sort(x[:, c]), rtol=1e-14, atol=0)
    p = np.array([.1, .5, .8])
    got = bd.quantile(x, p, weights=w, backend="host")
    np.testing.assert_allclose(got, ref.quantile_weighted(x, w[:, None], p), rtol=1e-12, atol=1e-14)
    np.testing.assert_array_equal(bd.quantile(x, p, weights=w), got)      # 'auto' with weights is the host
    wf = rng.random((9, 4)) + .1
    for order in (1, 2):
        got = bd.quantile(x, p, weights=wf, ord=order, backend="host")
        assert got.shape == (3, 4)
        np.testing.assert_allclose(got, ref.quantile_weighted(x, wf, p, order), rtol=1e-12, atol=1e-14)
        ci = bd.sci(x, [.5, .8], weights=wf, ord=order)
        assert ci.shape == (2, 4, 2)
        np.testing.assert_allclose(ci, ref.sci_weighted(x, wf, [.5, .8], order), rtol=1e-12, atol=1e-14)
        np.testing.assert_array_equal(bd.credint(x, .8, weights=wf, ord=order), ci[1])
        np.testing.assert_array_equal(bd.qbci(x, .8, weights=wf, ord=order, backend="host"),
                                      np.stack([bd.quantile(x, 1. - (1. - .8) / 2. - .8, weights=wf, ord=order, backend="host"),
                                                bd.quantile(x, (1. - .8) / 2. + .8, weights=wf, ord=order, backend="host")], axis=-1))
    assert np.all(np.diff(bd.sci(x[:, 0], .6)) > 0) and bd.sci(x[:, 0], .6).shape == (2,)
    # a uniform density on a uniform grid: the quantile of ord = 2 is the linear ramp
    grid = np.linspace(-2., 6., 33)
    np.testing.assert_allclose(bd.quantile(grid, [0., .2, .5, .9, 1.], weights=np.ones(33), ord=2, backend="host"),
                               -2. + 8. * np.array([0., .2, .5, .9, 1.]), rtol=0, atol=1e-13)
    with pytest.raises(NotImplementedError):
        bd.quantile(x, p, ord=3, backend="host")


@pytest.mark.parametrize("n", [1, 3, 7, 101])
def test_argmedian(bd, n):
    a = _draws(6, (4, n, 3))
    i = bd.argmedian(a, axis=1)
    assert i.shape == (4, 3)
    np.testing.assert_array_equal(np.take_along_axis(a, i[:, None], 1)[:, 0], np.median(a, axis=1))
    v = a[0, :, 0]
    assert v[bd.argmedian(v)] == np.median(v)
    assert a[0].reshape(-1)[bd.argmedian(a[0], axis=None)] == np.median(a[0])      # 3 n values: an odd count


def test_shapes_of_every_output(bd):
    x = _draws(7, (2, 9, 3))
    assert bd.quantile(x, .5, backend="host").shape == (9, 3)
    assert bd.quantile(x, .5, axis=1, backend="host").shape == (2, 3)
    assert bd.quantile(x, [[.1, .2]], axis=(0, 1), backend="host").shape == (1, 2, 3)
    assert bd.quantile(x, .5, axis=(0, 1, 2), backend="host").shape == ()
    assert bd.quantile(3., .5, backend="host").shape == () and bd.quantile(3., .5, backend="host") == 3.
    assert bd.qbci(x, [.5, .9], axis=(0, 1), backend="host").shape == (2, 3, 2)
    assert bd.sci_noweights(x, .9, axis=(0, 1), backend="host").shape == (3, 2)
    assert bd.sci(x, [.5, .9], axis=1).shape == (2, 2, 3, 2)
    assert bd.credint(x, backend="host").shape == (9, 3, 2)
    assert bd.sort_draws(x, axis=(0, 1), backend="host").shape == (18, 3)
    b, e = bd.rank_counts(x, np.zeros(3), axis=(0, 1), backend="host")
    assert b.shape == e.shape == (3,) and b.dtype == e.dtype == np.int32
    t = torch.from_numpy(x)
    np.testing.assert_array_equal(bd.quantile(t, .5, axis=(0, 1), backend="host"), bd.quantile(x, .5, axis=(0, 1), backend="host"))
    with pytest.raises(ValueError):
        bd.quantile(x, .5, axis=(0, 0), backend="host")
    with pytest.raises(ValueError):
        bd.quantile(x, .5, axis=3, backend="host")


def test_new_symbol_is_declared_and_exported():
    from montecosmo_amd import _lib, bdec
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    assert "int mcpm_bdec_sort_f32(" in header
    assert "mcpm_bdec_sort_f32" in _lib.SIGNATURES and hasattr(_lib.lib, "mcpm_bdec_sort_f32")
    assert len(_lib.SIGNATURES["mcpm_bdec_sort_f32"][1]) == 18
    assert _lib.ABI_VERSION == "mcpm 0.12 (gfx950)" and '#define MCPM_ABI_VERSION "mcpm 0.12 (gfx950)"' in header
    assert f"#define MCPM_BDEC_MAX_M {bdec.LDS_MAX_M}\n" in header and f"#define MCPM_BDEC_MAX_RANKS {bdec.MAX_RANKS}\n" in header
    makefile = open(os.path.join(ROOT, "montecosmo_amd", "csrc", "Makefile")).read()
    assert " bdec.hip " in makefile


def test_backend_rules(bd):
    x32, x64 = _draws(8, (2, 8, 3), np.float32), _draws(8, (2, 8, 3))
    w = np.ones(2)
    for fn in (bd.quantile, bd.qbci, bd.credint):
        with pytest.raises(TypeError):
            fn(x32, .5, weights=w, backend="hip")
        with pytest.raises(TypeError):
            fn(x32, .5, ord=2, backend="hip")
        with pytest.raises(TypeError):
            fn(x64, .5, backend="hip")      # float64 draws
        with pytest.raises(ValueError):
            fn(x32, .5, backend="cpu")
    with pytest.raises(TypeError):
        bd.sci(x32, .5, backend="hip")
    with pytest.raises(TypeError):
        bd.sci_noweights(x64, .5, backend="hip")
    with pytest.raises(TypeError):
        bd.rank_counts(x64, np.zeros((8, 3)), backend="hip")
    if not torch.cuda.is_available():      # float32 draws without a GPU: 'auto' is the host
        np.testing.assert_array_equal(bd.quantile(x32, .5, axis=(0, 1)), bd.quantile(x32, .5, axis=(0, 1), backend="host"))


def test_chains_methods_on_host_data():
    from montecosmo_amd import chains
    rng = np.random.default_rng(9)
    data = {"a": rng.standard_normal((3, 30)), "f": rng.standard_normal((3, 30, 2, 4)) + 5., "n_evals": rng.integers(1, 9, (3, 30))}
    ch = chains.Chains(data, backend="host")
    before = {k: np.array(v) for k, v in data.items()}
    p = [.05, .5]
    q, ci, med = ch.quantile(p), ch.credint(), ch.credint(.8, type="med")
    assert q["a"].shape == (2,) and q["f"].shape == (2, 2, 4) and ci["a"].shape == (2,) and ci["f"].shape == (2, 4, 2)
    assert q["n_evals"] == data["n_evals"].sum() and ci["n_evals"] == data["n_evals"].sum()
    np.testing.assert_array_equal(q["f"].reshape(2, 8), ref.quantile(data["f"].reshape(90, 8), p))
    low, high, _ = ref.sci_noweights(data["f"].reshape(90, 8), .95)
    np.testing.assert_array_equal(ci["f"].reshape(8, 2), np.stack([low, high], axis=-1))
    np.testing.assert_array_equal(med["a"], ref.qbci(data["a"].reshape(90, 1), .8, "med")[0])
    np.testing.assert_array_equal(chains.quantile(data["f"], p, backend="host"), q["f"])
    np.testing.assert_array_equal(chains.credint(data["f"], backend="host"), ci["f"])
    truth = {"a": rng.standard_normal(()), "f": rng.standard_normal((2, 4)) + 5.}
    cov = ch.coverage(truth)
    assert set(cov) == {"a", "f"}
    assert cov["f"] == ref.coverage(data["f"].reshape(90, 8), truth["f"], .95) and cov["a"] == ref.coverage(data["a"].reshape(90, 1), truth["a"], .95)
    assert ch.coverage({"f": truth["f"]}, p=.5, type="med")["f"] == float(np.mean((ref.qbci(data["f"].reshape(90, 8), .5, "med")[:, 0] <= truth["f"].reshape(-1))
                                                                               & (truth["f"].reshape(-1) <= ref.qbci(data["f"].reshape(90, 8), .5, "med")[:, 1])))
    with pytest.raises(ValueError):
        ch.coverage({"f": np.zeros(3)})
    for k, v in before.items():      # nothing was changed in place
        np.testing.assert_array_equal(data[k], v)
