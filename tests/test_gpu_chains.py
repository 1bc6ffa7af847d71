"""Chain diagnostics on the GPU (montecosmo_amd/chains.py, csrc/chains.hip) against the float64 restatement tests/_chains_f64.py.

tau is compared, not ess (tau can sit near 0).  Per dimension |tau - tau_ref| <= 16 N L 2^-53 with L the restatement's number of lags
summed: the worst-case reordering bound (each gamma is a sum of at most N products bounded by the variance, the quotient brings a factor
below 3, tau doubles the sum of L lags); a float32 accumulator would miss it by five orders.  n_lags equals L exactly except where some
|P_j| of the restatement is below that same tolerance (the pair may fall on either side of zero): those dimensions are compared on tau
only and counted, and the count stays under 1 % of the dimensions.  mean and m2 are within 4 N 2^-53 relative of sum |x| and
sum (x - m)^2, R-hat within 1e-12 relative.  Everything else is bitwise: repeats, aligned against misaligned views, a dimension alone
against the same dimension among others, strided segments against copies, chunked uploads against resident data."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _chains_f64 as ref  # noqa: E402

EPS = 2. ** -53


def _make(name):
    """float32 draws of the named case."""
    shape, phi, seed, offset = {
        "c1n4d1": ((1, 4, 1), 0., 1, 0.),
        "c2n4d63": ((2, 4, 63), 0., 2, 0.),
        "c3n5d64": ((3, 5, 64), 0., 3, 0.),              # odd N: the last lag is dropped, the middle draw is outside the split
        "c4n257d65": ((4, 257, 65), .7, 4, 0.),
        "c4n200d130": ((4, 200, 130), .98, 5, 0.),        # long sums across several lag blocks
        "c4n1000d4099": ((4, 1000, 4099), None, 6, 0.),   # phi = 0.9 in half of the dimensions, 0 in the rest
        "c3n200d130off": ((3, 200, 130), 0., 7, 100.),    # chain c offset by 100 c: never a pair <= 0, every lag is summed; large means
        "c3n201d130off": ((3, 201, 130), 0., 8, 100.),
    }[name]
    rng = np.random.default_rng(seed)
    if phi is None:
        phi = np.where(np.arange(shape[2]) % 2, .9, 0.)
    x = ref.ar1(rng, phi, shape)
    x += offset * np.arange(shape[0]).reshape(-1, 1, 1)
    return x.astype(np.float32)


CASES = ["c1n4d1", "c2n4d63", "c3n5d64", "c4n257d65", "c4n200d130", "c4n1000d4099", "c3n200d130off", "c3n201d130off"]
_cache = {}


def _case(name):
    """(x float32, restatement) of a case, made once and shared; nothing changes them."""
    if name not in _cache:
        x = _make(name)
        x64 = x.astype(np.float64)
        with np.errstate(all="ignore"):
            tau, lags, pairs = ref.tau_and_lags(x64, return_pairs=True)
            r = dict(tau=tau, lags=lags, pairs=pairs, gr=ref.gelman_rubin(x64),
                     sgr=ref.split_gelman_rubin(x64) if x.shape[1] >= 4 else None)
        x.setflags(write=False)
        _cache[name] = (x, r)
    return _cache[name]


def _dev(a, gpu, misaligned=False):
    """The array on the device; misaligned: as the view buf[1:] of a buffer one element longer (no 16-byte alignment)."""
    t = torch.from_numpy(np.array(a, order="C")).to(gpu)      # (a copy: the shared cases are read-only)
    if not misaligned:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=gpu)
    view = buf[1:]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 != 0
    return view.reshape(t.shape)


def _check_tau(tau, lags, x, r, what=""):
    n = x.shape[1]
    tol = 16. * n * r["lags"] * EPS
    err = np.abs(tau - r["tau"])
    unsure = np.any(np.abs(r["pairs"]) < tol, axis=0)
    print(what, "shape", x.shape, "max |tau - ref|", err.max(), "max err / tol", (err / tol).max(), "L mean", r["lags"].mean(), "L max",
          r["lags"].max(), "unsure", int(unsure.sum()), "of", unsure.size)
    assert tau.dtype == np.float64 and lags.dtype == np.int32
    assert np.all(err <= tol)
    assert unsure.sum() == 0 or unsure.sum() < .01 * unsure.size
    np.testing.assert_array_equal(lags[~unsure], r["lags"][~unsure])


@pytest.mark.parametrize("name", CASES)
def test_shapes_aligned_and_misaligned(gpu, name):
    from montecosmo_amd import chains
    x, r = _case(name)
    c, n, d = x.shape
    x64 = x.astype(np.float64)
    if name.endswith("off"):
        assert np.all(r["lags"] == n - n % 2) and np.all(r["pairs"][1:] > 0)      # it runs out of lags
    got = []
    for mis in (False, True):
        t = _dev(x, gpu, mis)
        tau, lags = chains.autocorr_time(t, backend="hip", return_lags=True)
        mean, m2 = chains.segment_moments(t, backend="hip")
        gr = chains.gelman_rubin(t, backend="hip")
        sgr = chains.split_gelman_rubin(t, backend="hip") if n >= 4 else None
        got.append((tau, lags, mean, m2, gr, sgr))
    for a, b in zip(*got):
        if a is not None:
            np.testing.assert_array_equal(a, b)      # NaN-free here, so equality is bitwise
    tau, lags, mean, m2, gr, sgr = got[0]
    _check_tau(tau, lags, x, r, name)
    m_ref = x64.mean(axis=1)
    m2_ref = np.sum((x64 - m_ref[:, None]) ** 2, axis=1)
    assert np.all(np.abs(mean[:, 0] - m_ref) * n <= 4 * n * EPS * np.abs(x64).sum(axis=1))
    assert np.all(np.abs(m2[:, 0] - m2_ref) <= 4 * n * EPS * m2_ref)
    np.testing.assert_allclose(gr, r["gr"], rtol=1e-12)
    if sgr is not None:
        np.testing.assert_allclose(sgr, r["sgr"], rtol=1e-12)
    ess = chains.effective_sample_size(t, backend="hip")
    np.testing.assert_array_equal(ess, c * n / tau)
    cm, cs = chains.chain_moments(t)      # 'auto' takes the device for float32 draws
    np.testing.assert_array_equal(cm, mean[:, 0])
    np.testing.assert_array_equal(cs, np.sqrt(m2[:, 0] / n))


def test_repeat_is_bitwise(gpu):
    from montecosmo_amd import chains
    t = _dev(_case("c4n200d130")[0], gpu)
    a = chains.autocorr_time(t, backend="hip", return_lags=True) + (chains.split_gelman_rubin(t), chains.multi_ess(t), chains.multi_gr(t))
    b = chains.autocorr_time(t, backend="hip", return_lags=True) + (chains.split_gelman_rubin(t), chains.multi_ess(t), chains.multi_gr(t))
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_a_dimension_does_not_know_its_neighbours(gpu):
    from montecosmo_amd import chains
    x, _ = _case("c4n1000d4099")
    t = _dev(x, gpu)
    tau, lags = chains.autocorr_time(t, backend="hip", return_lags=True)
    sgr = chains.split_gelman_rubin(t)
    assert lags.min() < lags.max()      # lanes of one wave stop at different sweeps
    for col in (0, 63, 64, 4098):
        one = _dev(x[:, :, col:col + 1], gpu)
        t1, l1 = chains.autocorr_time(one, backend="hip", return_lags=True)
        assert t1[0] == tau[col] and l1[0] == lags[col]
        assert chains.split_gelman_rubin(one)[0] == sgr[col]
    perm = np.random.default_rng(0).permutation(x.shape[2])
    tp, lp = chains.autocorr_time(_dev(x[:, :, perm], gpu), backend="hip", return_lags=True)
    np.testing.assert_array_equal(tp, tau[perm])
    np.testing.assert_array_equal(lp, lags[perm])
    np.testing.assert_array_equal(chains.split_gelman_rubin(_dev(x[:, :, perm], gpu)), sgr[perm])


@pytest.mark.parametrize("name", ["c3n5d64", "c4n257d65"])
def test_strided_segments_equal_copies(gpu, name):
    from montecosmo_amd import chains
    x, _ = _case(name)
    c, n, d = x.shape
    h = n // 2
    t = _dev(x, gpu)
    halves = np.stack([x[:, :h], x[:, n - h:]], axis=1)      # [C, 2, h, D]: segment 2 c + p
    cat = _dev(halves.reshape(2 * c, h, d), gpu)
    np.testing.assert_array_equal(chains.split_gelman_rubin(t, backend="hip"), chains.gelman_rubin(cat, backend="hip"))
    mean, m2 = chains.segment_moments(t, 2, h, 0, n - h, backend="hip")
    mean_c, m2_c = chains.segment_moments(cat, backend="hip")
    np.testing.assert_array_equal(mean.reshape(2 * c, d), mean_c[:, 0])
    np.testing.assert_array_equal(m2.reshape(2 * c, d), m2_c[:, 0])
    # thin: blocks of two lengths (N not divisible) against sliced copies
    ch = chains.Chains({"f": t, "n_evals": np.ones((c, n))}, backend="hip")
    thinning = 2 if n < 10 else 50
    n_split = int(max(np.rint(n / thinning), 1))
    assert n % n_split
    mom = ch.thin(thinning, moment=(0, 1, 2))["f"]
    last = ch.thin(thinning)["f"]
    bounds = np.cumsum([0] + [len(p) for p in np.array_split(np.arange(n), n_split)])
    assert mom.shape == (c, n_split, d, 3)
    for b in range(n_split):
        lo, hi = bounds[b], bounds[b + 1]
        piece = chains.Chains({"f": _dev(x[:, lo:hi], gpu)}, backend="hip")
        np.testing.assert_array_equal(mom[:, b], piece.moment()["f"])
        np.testing.assert_array_equal(last[:, b], x[:, hi - 1].astype(np.float64))
        np.testing.assert_allclose(mom[:, b, :, 2], np.sum(x[:, lo:hi].astype(np.float64) ** 2, axis=1), rtol=1e-13)


def test_unbiased_autocovariance(gpu):
    from montecosmo_amd import chains
    x, _ = _case("c4n257d65")
    with np.errstate(all="ignore"):
        tau_r, lags_r, pairs = ref.tau_and_lags(x.astype(np.float64), bias=False, return_pairs=True)
    tau, lags = chains.autocorr_time(_dev(x, gpu), bias=False, backend="hip", return_lags=True)
    _check_tau(tau, lags, x, dict(tau=tau_r, lags=lags_r, pairs=pairs), "bias=False")
    assert np.any(tau != chains.autocorr_time(_dev(x, gpu), backend="hip"))


def test_constant_and_nan_dimensions(gpu):
    from montecosmo_amd import chains
    x, _ = _case("c4n257d65")
    t = _dev(x, gpu)
    tau, lags = chains.autocorr_time(t, backend="hip", return_lags=True)
    gr = chains.gelman_rubin(t)
    keep = np.ones(x.shape[2], dtype=bool)
    keep[[3, 64]] = False
    y = x.copy()
    y[:, :, 3] = 2.5                 # constant in every chain: 0 / 0
    y[2, 100, 64] = np.nan           # one NaN draw
    y[1, :, 10] = -1.25              # one constant chain among four: W > 0, finite, as the formulas give it
    keep2 = keep.copy()
    keep2[10] = False
    ty, ly = chains.autocorr_time(_dev(y, gpu), backend="hip", return_lags=True)      # (the call returns)
    gy = chains.gelman_rubin(_dev(y, gpu))
    assert np.isnan(ty[3]) and np.isnan(ty[64]) and np.isnan(gy[3]) and np.isnan(gy[64])
    assert ly[64] == x.shape[1] - x.shape[1] % 2
    np.testing.assert_array_equal(ty[keep2], tau[keep2])
    np.testing.assert_array_equal(ly[keep2], lags[keep2])
    np.testing.assert_array_equal(gy[keep2], gr[keep2])
    with np.errstate(all="ignore"):
        tau_r, lags_r = ref.tau_and_lags(y[:, :, 10:11].astype(np.float64))
    assert np.isfinite(ty[10]) and abs(ty[10] - tau_r[0]) <= 16 * x.shape[1] * lags_r[0] * EPS


def test_indexing_past_2_to_the_31(gpu):
    from montecosmo_amd import chains
    n, d, far = 16, 64, 2 ** 31
    x = ref.ar1(np.random.default_rng(9), .5, (2, n, d)).astype(np.float32)
    buf = torch.empty(far + 4096, dtype=torch.float32, device=gpu)
    buf[:n * d] = _dev(x[0], gpu).reshape(-1)
    buf[far:far + n * d] = _dev(x[1], gpu).reshape(-1)
    view = buf.as_strided((2, n, d), (far, d, 1))      # the two chains 2^31 elements apart: read in place by stride_chain
    tight = _dev(x, gpu)
    a = chains.autocorr_time(view, backend="hip", return_lags=True) + chains.segment_moments(view, backend="hip")
    b = chains.autocorr_time(tight, backend="hip", return_lags=True) + chains.segment_moments(tight, backend="hip")
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(chains.split_gelman_rubin(view), chains.split_gelman_rubin(tight))
    np.testing.assert_allclose(a[2][:, 0], x.astype(np.float64).mean(axis=1), rtol=1e-13, atol=1e-15)
    del buf, view


def test_chunked_upload_of_host_arrays_is_bitwise_the_resident_call(gpu, monkeypatch):
    from montecosmo_amd import chains, metrics
    x, _ = _case("c4n257d65")
    t = _dev(x, gpu)
    want = chains.autocorr_time(t, backend="hip", return_lags=True) + (chains.split_gelman_rubin(t), chains.gelman_rubin(t)) \
        + chains.chain_moments(t) + (chains.multi_ess(t), chains.multi_gr(t))
    monkeypatch.setattr(metrics, "CHUNK_BYTES", 4 * 4 * 257 * 25)      # 25 of the 65 dimensions per upload: three chunks
    uploads = []
    real = chains._Resident
    monkeypatch.setattr(chains, "_Resident", lambda t: uploads.append(t.shape[2]) or real(t))
    got = chains.autocorr_time(x, backend="hip", return_lags=True)
    assert uploads == [25, 25, 15]
    got = got + (chains.split_gelman_rubin(x), chains.gelman_rubin(x)) + chains.chain_moments(x) + (chains.multi_ess(x), chains.multi_gr(x))
    for u, v in zip(got, want):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(chains.multi_ess(torch.from_numpy(x.copy())), want[-2])      # a host tensor goes the same way


def test_multi_ess_and_multi_gr_match_restatement(gpu):
    from montecosmo_amd import chains
    x, r = _case("c4n1000d4099")
    c, n, d = x.shape
    t = _dev(x, gpu)
    # ess = C N / tau: its relative error is tau's, and a harmonic mean's is at most its terms' (plus the rounding of the mean itself)
    rel = np.max(16. * n * r["lags"] * EPS / np.abs(r["tau"])) + 1e-13
    ess_r = c * n / r["tau"]
    got, want = chains.multi_ess(t), ref.harmean(ess_r)
    print("multi_ess", got, "restatement", want, "bound", rel)
    assert got.shape == () and abs(got - want) <= rel * abs(want)
    got_gr = chains.multi_gr(t)
    np.testing.assert_allclose(got_gr, np.sqrt(np.mean(r["gr"] ** 2)), rtol=1e-12)
    x4 = x[:, :, :4096].reshape(c, n, 64, 64)
    t4 = _dev(x4, gpu)
    got = chains.multi_ess(t4, axis=0)
    want = ref.harmean(ess_r[:4096].reshape(64, 64), axis=0)
    assert got.shape == (64,) and np.all(np.abs(got - want) <= rel * np.abs(want))
    np.testing.assert_allclose(chains.multi_gr(t4, axis=1), np.sqrt(np.mean(r["gr"][:4096].reshape(64, 64) ** 2, axis=1)), rtol=1e-12)
    ch = chains.Chains({"f": t, "n_evals": np.full((c, n), 3)})
    np.testing.assert_array_equal(ch.multi_ess()["f"], chains.multi_ess(t))
    np.testing.assert_array_equal(ch.eval_per_ess()["f"], 3 * c * n / chains.multi_ess(t))


def test_from_flat_slices_are_read_in_place(gpu):
    from montecosmo_amd import chains
    rng = np.random.default_rng(12)
    flat = rng.standard_normal((2, 40, 3 + 4 * 5)).astype(np.float32)
    t = _dev(flat, gpu)
    ch = chains.Chains.from_flat(t, {"a": (0, 1, ()), "b": (1, 3, (2,)), "w": (3, 23, (4, 5))})
    assert ch["w"].data_ptr() == t.data_ptr() + 12 and not ch["w"].is_contiguous()
    for k, sl in (("a", slice(0, 1)), ("b", slice(1, 3)), ("w", slice(3, 23))):
        copy = _dev(flat[:, :, sl], gpu).reshape(ch[k].shape)
        np.testing.assert_array_equal(chains.autocorr_time(ch[k], backend="hip"), chains.autocorr_time(copy, backend="hip"))
        np.testing.assert_array_equal(chains.split_gelman_rubin(ch[k]), chains.split_gelman_rubin(copy))
    s = ch.summary(names=["a", "b"])
    assert list(s) == ["a", "b[0]", "b[1]"]
    np.testing.assert_allclose(s["b[1]"]["n_eff"], ref.effective_sample_size(flat[:, :, 2].astype(np.float64)), rtol=1e-9)


def test_error_codes_launch_nothing(gpu):
    from montecosmo_amd import _lib
    import ctypes as C
    x = torch.zeros(2 * 8 * 4, dtype=torch.float32, device=gpu)
    mean = torch.zeros((2, 4), dtype=torch.float64, device=gpu)
    m2, tau, lags = torch.zeros_like(mean), torch.full((4,), 7., dtype=torch.float64, device=gpu), torch.zeros(4, dtype=torch.int32, device=gpu)
    s = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    lib = _lib.lib
    E_ARG = -6
    args = _lib.marshal("mcpm_chain_tau_f32", (s, x, 0, 4, 2, 32, 1, 0, 8, 4, mean, m2, 1, tau, lags))
    for pos, bad in ((8, 1), (3, 0), (1, None), (10, None), (13, None), (14, None)):      # n_draw < 2, n_dim < 1, null pointers
        a = list(args)
        a[pos] = bad
        assert lib.mcpm_chain_tau_f32(*a) == E_ARG
    args = _lib.marshal("mcpm_chain_moments_f32", (s, x, 0, 4, 2, 32, 1, 0, 8, 4, mean, m2))
    for pos, bad in ((3, 0), (1, None), (10, None), (11, None), (5, -1)):
        a = list(args)
        a[pos] = bad
        assert lib.mcpm_chain_moments_f32(*a) == E_ARG
    torch.cuda.synchronize()
    assert torch.all(tau == 7.)


def test_powtranscoh_chains(gpu):
    from montecosmo_amd import chains, model
    rng = np.random.default_rng(13)
    shape = (16, 16, 16)
    fwd = model.FieldLevelForward(final_shape=shape, cell_length=10.)
    truth = rng.standard_normal(shape).astype(np.float32)
    meshes = (truth + .5 * rng.standard_normal((2, 3) + shape)).astype(np.float32)
    ch = chains.Chains({"m": _dev(meshes, gpu), "n_evals": np.ones((2, 3))})
    out = fwd.powtranscoh_chains(ch, _dev(truth, gpu), names="m")
    assert "kptc_m" not in ch and set(out) == {"m", "n_evals", "kptc_m"} and len(out["kptc_m"]) == 4
    for c in range(2):
        for i in range(3):
            single = fwd.powtranscoh(_dev(truth, gpu), _dev(meshes[c, i], gpu))
            for got, want in zip(out["kptc_m"], single):      # equal up to the float32 transforms, should a batch of six take another path than one
                assert got.shape[:2] == (2, 3)
                np.testing.assert_allclose(got[c, i], want, rtol=1e-5, equal_nan=True)
