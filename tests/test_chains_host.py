"""Chain diagnostics without a GPU (montecosmo_amd/chains.py, host backend): known answers that pin the reading of the formulas
(tests/_chains_f64.py says where they come from), AR(1) chains whose effective sample size is known in closed form, the host backend
against the restatement, the two new symbols, and the Chains transforms on small arrays."""
import os

import numpy as np
import pytest
import torch

import _chains_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X2 = np.array([[1, 3, 2, 5, 4, 6], [2, 2, 4, 3, 7, 5]], dtype=np.float64)
X1 = np.array([[1, 3, 2, 5, 4, 6, 8]], dtype=np.float64)


@pytest.fixture(scope="module")
def ch():
    from montecosmo_amd import chains
    return chains


def _both(ch):
    return [("restatement", ref.tau_and_lags, ref.effective_sample_size, ref.gelman_rubin, ref.split_gelman_rubin),
            ("host", lambda x: ch.autocorr_time(x, backend="host", return_lags=True), lambda x: ch.effective_sample_size(x, backend="host"),
             lambda x: ch.gelman_rubin(x, backend="host"), lambda x: ch.split_gelman_rubin(x, backend="host"))]


def test_known_answers_two_chains(ch):
    for name, tau, ess, gr, sgr in _both(ch):
        np.testing.assert_allclose(tau(X2)[0], 0.9525525525525529, rtol=1e-12, err_msg=name)
        assert int(tau(X2)[1]) == 4, name
        np.testing.assert_allclose(ess(X2), 12.597730138713741, rtol=1e-12, err_msg=name)
        np.testing.assert_allclose(gr(X2), 0.9212078230296404, rtol=1e-12, err_msg=name)
        np.testing.assert_allclose(sgr(X2), 2 ** .5, rtol=1e-12, err_msg=name)


def test_known_answers_one_chain_odd_draws(ch):
    for name, tau, ess, gr, sgr in _both(ch):
        np.testing.assert_allclose(ess(X1), 3.776373973468098, rtol=1e-12, err_msg=name)
        np.testing.assert_allclose(gr(X1), 1., rtol=1e-12, err_msg=name)
        np.testing.assert_allclose(sgr(X1), 1.96638416050035, rtol=1e-12, err_msg=name)


def test_restatement_direct_and_fft_autocovariances_agree():
    rng = np.random.default_rng(3)
    for shape, phi in [((2, 4, 7), 0.), ((3, 5, 8), .3), ((4, 257, 9), .7), ((4, 200, 6), .98)]:
        x = ref.ar1(rng, phi, shape)
        for bias in (True, False):
            a, la = ref.tau_and_lags(x, bias, "direct")
            b, lb = ref.tau_and_lags(x, bias, "fft")
            np.testing.assert_allclose(a, b, rtol=0, atol=1.2e-13 * max(1., np.abs(a).max()))
            np.testing.assert_array_equal(la, lb)


@pytest.mark.parametrize("phi", [0., .5, .9])
def test_ar1_effective_sample_size_and_rhat(ch, phi):
    c, n, d = 4, 1000, 512
    x = ref.ar1(np.random.default_rng(int(10 * phi) + 11), phi, (c, n, d))
    expect = c * n * (1 - phi) / (1 + phi)
    for name, mess, mgr in [("restatement", ref.multi_ess, ref.multi_gr),
                            ("host", lambda a: ch.multi_ess(a, backend="host"), lambda a: ch.multi_gr(a, backend="host"))]:
        ratio, gr = float(mess(x)) / expect, float(mgr(x))
        print(name, "phi", phi, "multi_ess / expected", ratio, "multi_gr", gr)
        assert .9 <= ratio <= 1.1, name
        assert .99 <= gr <= 1.03, name


@pytest.mark.parametrize("shape,phi", [((1, 4, 1), 0.), ((2, 4, 63), 0.), ((3, 5, 64), .2), ((4, 257, 65), .7), ((4, 200, 130), .98),
                                       ((3, 201, 5, 7), .5), ((2, 50), .5)])
@pytest.mark.parametrize("bias", [True, False])
def test_host_backend_matches_restatement(ch, shape, phi, bias):
    x = ref.ar1(np.random.default_rng(sum(shape)), phi, shape)
    tau_r, lags_r, pairs = ref.tau_and_lags(x, bias, return_pairs=True)
    tau, lags = ch.autocorr_time(x, bias=bias, backend="host", return_lags=True)
    assert tau.dtype == np.float64 and tau.shape == tuple(shape[2:]) and lags.shape == tuple(shape[2:])
    np.testing.assert_allclose(tau, tau_r, rtol=1e-12, atol=1e-12)
    sure = np.all(np.abs(pairs) > 1e-11, axis=0)      # a pair sum at rounding level may fall on either side of zero
    assert sure.mean() > .99
    np.testing.assert_array_equal(lags[sure], lags_r[sure])
    ess = ch.effective_sample_size(x, bias=bias, backend="host")
    np.testing.assert_allclose(ess, shape[0] * shape[1] / tau, rtol=1e-15)
    np.testing.assert_allclose(ch.gelman_rubin(x, backend="host"), ref.gelman_rubin(x), rtol=1e-12)
    if shape[1] >= 4:
        np.testing.assert_allclose(ch.split_gelman_rubin(x, backend="host"), ref.split_gelman_rubin(x), rtol=1e-12)
    mean, std = ch.chain_moments(x, backend="host")
    np.testing.assert_allclose(mean, x.mean(axis=1), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(std, x.std(axis=1), rtol=1e-13)
    np.testing.assert_allclose(ch.multi_ess(x, backend="host"), ref.multi_ess(x), rtol=1e-11)
    np.testing.assert_allclose(ch.multi_gr(x, backend="host"), ref.multi_gr(x), rtol=1e-12)


def test_torch_input_constant_dimension_and_reductions(ch):
    x = ref.ar1(np.random.default_rng(5), .4, (3, 40, 4, 5))
    x[:, :, 1, 2] = 3.
    with np.errstate(all="ignore"):
        want = ref.effective_sample_size(x)
    got = ch.effective_sample_size(torch.from_numpy(x), backend="auto")      # float64: the host path, GPU or not
    assert np.isnan(got[1, 2]) and np.isnan(want[1, 2])
    np.testing.assert_allclose(got, want, rtol=1e-12)
    y = np.delete(x.reshape(3, 40, 20), 7, axis=2).reshape(3, 40, 19)
    np.testing.assert_allclose(ch.multi_ess(y, axis=0, backend="host"), ref.multi_ess(y, axis=0), rtol=1e-11)
    a = np.random.default_rng(0).uniform(1, 2, (4, 5))
    np.testing.assert_allclose(ch.harmean(a, 1), 1 / np.mean(1 / a, 1), rtol=1e-15)
    np.testing.assert_allclose(ch.geomean(a), np.exp(np.mean(np.log(a))), rtol=1e-15)
    from montecosmo_amd import metrics
    assert metrics.multi_ess is ch.multi_ess and metrics.multi_gr is ch.multi_gr
    assert metrics.harmean is ch.harmean and metrics.geomean is ch.geomean
    assert {"multi_ess", "multi_gr", "harmean", "geomean"} <= set(metrics.__all__)


def test_argument_checks_come_before_any_device_call(ch, monkeypatch):
    from montecosmo_amd import _lib

    def no_call(name, *a, **k):
        raise AssertionError(f"device call {name}")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(ch.nbody, "_device", lambda: (_ for _ in ()).throw(AssertionError("device asked for")))
    x64 = np.zeros((2, 8, 3))
    for fn in (ch.effective_sample_size, ch.gelman_rubin, ch.split_gelman_rubin, ch.chain_moments, ch.multi_ess, ch.multi_gr):
        with pytest.raises((ValueError, TypeError)):
            fn(x64, backend="hip")
        with pytest.raises((ValueError, TypeError)):
            fn(torch.zeros(2, 8, 3, dtype=torch.float64), backend="hip")
        with pytest.raises(ValueError):
            fn(np.zeros(5, dtype=np.float32), backend="hip")
        with pytest.raises(ValueError):
            fn(np.zeros((2, 8), dtype=np.float32), backend="cpu")
    for fn in (ch.effective_sample_size, ch.gelman_rubin, ch.multi_ess):
        with pytest.raises(ValueError):
            fn(np.zeros((2, 1, 3), dtype=np.float32), backend="hip")
    with pytest.raises(ValueError):
        ch.split_gelman_rubin(np.zeros((2, 3, 3), dtype=np.float32), backend="hip")


def test_new_symbols_are_declared_and_exported():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    for name in ("mcpm_chain_moments_f32", "mcpm_chain_tau_f32"):
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.ABI_VERSION == "mcpm 0.12 (gfx950)"
    n_args = [len(_lib.SIGNATURES[n][1]) for n in ("mcpm_chain_moments_f32", "mcpm_chain_tau_f32")]
    assert n_args == [12, 15]


# ---- Chains ---------------------------------------------------------------------------------------------------------
def _small(ch, n=12):
    rng = np.random.default_rng(8)
    return ch.Chains({"a": rng.standard_normal((3, n)), "f": rng.standard_normal((3, n, 2, 4)) + 5.,
                      "n_evals": rng.integers(1, 9, (3, n))}, backend="host")


@pytest.mark.parametrize("n,thinning", [(12, 4), (11, 4), (13, 3), (12, None), (5, 1)])
def test_thin(ch, n, thinning):
    c = _small(ch, n)
    n_split = 1 if thinning is None else int(max(np.rint(n / thinning), 1))
    last, mom = c.thin(thinning), c.thin(thinning, moment=(0, 1, 2))
    mom1 = c.thin(thinning, moment=1)
    for k in ("a", "f"):
        parts = np.array_split(np.asarray(c[k]), n_split, axis=1)
        np.testing.assert_array_equal(last[k], np.stack([p[:, -1] for p in parts], axis=1))
        want = np.stack([np.sum(p[..., None] ** np.arange(3), axis=1) for p in parts], axis=1)
        assert mom[k].shape == want.shape
        np.testing.assert_allclose(mom[k], want, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(mom1[k], want[..., 1], rtol=1e-13, atol=1e-13)
    ne = np.stack([p.sum(axis=1) for p in np.array_split(c["n_evals"], n_split, axis=1)], axis=1)
    np.testing.assert_array_equal(last["n_evals"], ne)
    np.testing.assert_array_equal(mom["n_evals"], ne)
    m3 = c.thin(thinning, moment=3)      # beyond the second moment: host power sums
    np.testing.assert_allclose(m3["a"], np.stack([np.sum(p ** 3, axis=1) for p in np.array_split(c["a"], n_split, axis=1)], axis=1), rtol=1e-13)


def test_metric_n_evals_rule_last_and_moments(ch):
    c = _small(ch)
    out = c.metric(lambda x: np.asarray(x).mean(axis=(0, 1)))
    assert out["n_evals"] == c["n_evals"].sum() and out["f"].shape == (2, 4)
    out = c.metric(lambda x, y: np.asarray(x) - np.asarray(y), c, axis=())
    np.testing.assert_array_equal(out["n_evals"], c["n_evals"])
    assert not out["a"].any()
    last = c.last()
    np.testing.assert_array_equal(last["f"], c["f"][:, -1])
    np.testing.assert_array_equal(last["n_evals"], c["n_evals"].sum(axis=1))
    mom = c.moment()
    np.testing.assert_allclose(mom["f"], np.sum(c["f"][..., None] ** np.arange(3), axis=1), rtol=1e-13)
    np.testing.assert_allclose(c.moment(m=2)["a"], np.sum(c["a"] ** 2, axis=1), rtol=1e-13)
    cm = c.cmoment()
    assert cm["f"].shape == (3, 2, 4, 2)
    np.testing.assert_allclose(cm["f"][..., 0], c["f"].mean(axis=1), rtol=1e-13)
    np.testing.assert_allclose(cm["f"][..., 1], c["f"].std(axis=1), rtol=1e-13)
    np.testing.assert_array_equal(cm["n_evals"], c["n_evals"].sum(axis=1))
    cen = mom.center_moment()
    np.testing.assert_allclose(cen["f"][..., 0], cm["f"][..., 0], rtol=1e-12)
    np.testing.assert_allclose(cen["f"][..., 1], cm["f"][..., 1], rtol=1e-9)      # (sum x^2 / N - mean^2 cancels at mean 5)


def test_mse_cmoment_eval_times_mse_and_ess_metrics(ch):
    c = _small(ch)
    truth = {"a": np.array([0.1, 1.2]), "f": np.stack([np.full((2, 4), 5.), np.full((2, 4), .9)], axis=-1)}
    mse = c.mse_cmoment(truth)
    for k in ("a", "f"):
        x = np.asarray(c[k])
        m0, s0 = truth[k][..., 0], truth[k][..., 1]
        want = np.stack([np.mean(((x.mean(1) - m0) / s0) ** 2 / 3), np.mean(2 * ((x.std(1) - s0) / s0) ** 2 / 3)])
        np.testing.assert_allclose(mse[k], want, rtol=1e-12)
    assert mse["n_evals"] == c["n_evals"].sum()
    np.testing.assert_allclose(c.mse_cmoment(truth, axis=0)["f"].shape, (2, 2, 4))
    etm = c.eval_times_mse(truth)
    np.testing.assert_allclose(etm["f"], mse["f"] * c["n_evals"].sum(), rtol=1e-15)
    me, mg, epe = c.multi_ess(), c.multi_gr(), c.eval_per_ess()
    for k in ("a", "f"):
        np.testing.assert_allclose(me[k], ref.multi_ess(np.asarray(c[k])), rtol=1e-11)
        np.testing.assert_allclose(mg[k], ref.multi_gr(np.asarray(c[k])), rtol=1e-12)
        np.testing.assert_allclose(epe[k], c["n_evals"].sum() / me[k], rtol=1e-15)
    fields = ch.Chains({"f": c["f"]}, backend="host")
    np.testing.assert_allclose(fields.multi_ess(axis=0)["f"], ref.multi_ess(np.asarray(c["f"]), axis=0), rtol=1e-11)


class _StandInLogDensity:
    n_rbins = 3

    class fwd:
        init_shape = (2, 3, 4)

    def names(self):
        return ["Omega_m", "ngbars_", "white_mesh_", "b1"]


def test_flat_layout_matches_unpack_and_from_flat(ch):
    from montecosmo_amd import samplers
    flat = samplers.FlatLogDensity(_StandInLogDensity())
    lay = flat.layout()
    q = torch.arange(5 + 24, dtype=torch.float32)
    un = flat.unpack(q)
    assert list(lay) == ["Omega_m", "ngbars_", "b1", "white_mesh_"] and set(lay) == set(un)
    for name, (start, stop, shape) in lay.items():
        np.testing.assert_array_equal(q[start:stop].reshape(shape).numpy(), np.asarray(un[name], dtype=np.float32))
    draws = np.random.default_rng(2).standard_normal((2, 6, 29)).astype(np.float32)
    for d in (draws, torch.from_numpy(draws)):
        c = ch.Chains.from_flat(d, lay)
        assert tuple(c["Omega_m"].shape) == (2, 6) and tuple(c["ngbars_"].shape) == (2, 6, 3) and tuple(c["white_mesh_"].shape) == (2, 6, 2, 3, 4)
        np.testing.assert_array_equal(np.asarray(c["white_mesh_"]), draws[:, :, 5:].reshape(2, 6, 2, 3, 4))
        np.testing.assert_array_equal(np.asarray(c["b1"]), draws[:, :, 4])
    with pytest.raises(ValueError):
        ch.Chains.from_flat(draws, {"x": (0, 30, (30,))})


def _fake_run(rng, n_warm, n_keep, d):
    infos = [{"warmup": i < n_warm, "n_evals": int(rng.integers(1, 9)), "accept_stat": float(rng.uniform()), "step_size": .1,
              "logdensity": float(rng.standard_normal()), "diverging": False} for i in range(n_warm + n_keep)]
    return {"samples": [torch.from_numpy(rng.standard_normal(d).astype(np.float32)) for _ in range(n_keep)], "infos": infos,
            "last_state": {"q": torch.zeros(d)}}


def test_load_runs_round_trip(ch, tmp_path):
    from montecosmo_amd import samplers
    rng = np.random.default_rng(4)
    d, paths, runs = 7, [str(tmp_path / f"chain{c}") for c in range(2)], {}
    for c, path in enumerate(paths):
        for i, (warm, keep) in enumerate([(3, 4), (0, 5), (0, 5)], start=1):      # run 1 carries warm-up rows
            if i == 3 and c == 1:
                continue      # the second chain stops a run short ...
            runs[c, i] = _fake_run(rng, warm, keep, d)
            samplers.save_run(runs[c, i], i, path)
    with pytest.raises(ValueError):
        ch.Chains.load_runs(paths, 1, 3)      # ... so the chains are ragged over the whole range
    lay = {"s": (0, 1, ()), "v": (1, 7, (2, 3))}
    c = ch.Chains.load_runs(paths, 1, 2, layout=lay)
    want = np.stack([np.concatenate([np.stack([s.numpy() for s in runs[k, i]["samples"]]) for i in (1, 2)]) for k in range(2)])
    assert tuple(c["v"].shape) == (2, 9, 2, 3)
    np.testing.assert_array_equal(c["s"], want[:, :, 0])
    np.testing.assert_array_equal(c["v"], want[:, :, 1:].reshape(2, 9, 2, 3))
    ne = np.stack([np.array([i["n_evals"] for r in (1, 2) for i in runs[k, r]["infos"] if not i["warmup"]]) for k in range(2)])
    np.testing.assert_array_equal(c["n_evals"], ne)
    assert "warmup" not in c and c["accept_stat"].shape == (2, 9)
    one = ch.Chains.load_runs(paths[1], 1, 5)      # runs 3 .. 5 are not there: the range ends, as in the reference
    assert one["samples"].shape == (1, 9, 7)
    with pytest.raises(FileNotFoundError):
        ch.Chains.load_runs(paths, 0, 2)
    twice = ch.Chains.load_runs(paths, 1, 2, layout=lay, transforms=[lambda p: p.thin(3)])
    assert twice["v"].shape == (2, 3, 2, 3)


def test_summary(ch, capsys):
    rng = np.random.default_rng(6)
    c = ch.Chains({"a": ref.ar1(rng, .5, (4, 200)), "v": ref.ar1(rng, 0., (4, 200, 2)), "n_evals": np.ones((4, 200))}, backend="host")
    s = c.summary()
    assert list(s) == ["a"]
    a = np.asarray(c["a"])
    row = s["a"]
    np.testing.assert_allclose([row["mean"], row["std"], row["median"], row["5.0%"], row["95.0%"]],
                               [a.mean(), a.std(), np.median(a), np.quantile(a, .05), np.quantile(a, .95)], rtol=1e-12)
    np.testing.assert_allclose(row["n_eff"], ref.effective_sample_size(a), rtol=1e-11)
    np.testing.assert_allclose(row["r_hat"], ref.split_gelman_rubin(a), rtol=1e-12)
    text = capsys.readouterr().out
    assert "n_eff" in text and "r_hat" in text and text.count("\n") == 2
    s = c.summary(names=["v"])
    assert list(s) == ["v[0]", "v[1]"]
    np.testing.assert_allclose(s["v[1]"]["n_eff"], ref.effective_sample_size(np.asarray(c["v"]))[1], rtol=1e-11)
