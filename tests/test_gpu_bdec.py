"""Order statistics of chains on the GPU (montecosmo_amd/bdec.py, csrc/bdec.hip) against the float64 restatement tests/_bdec_f64.py.

Order statistics, the sorted block, the smallest interval with its index and the counts against a truth are copies of input values and
integers: they are compared exactly (np.testing.assert_array_equal: zeros by value, NaN by position; where the sign of a zero is the
point it is compared on its own).  The draws come from a continuous distribution, so neither equal neighbours nor equal window lengths
decide a comparison, except in the adversarial rows, where the rule for ties (the first smallest window) is what is tested.
Interpolated quantiles are compared at 1e-12 relative to max(|x_(i-1)|, |x_(i)|): four float64 roundings bound the true difference
near 1e-15, 1e-12 leaves room for fused multiply-adds and is still five orders below one float32 ulp, so a wrong rank cannot pass.
Everything else is bitwise: repeats, a dimension alone against the same dimension among others, strided views against copies, chunked
uploads against resident data, the general path (more pooled draws than the LDS tile holds) against the LDS path."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _bdec_f64 as ref  # noqa: E402

PS = np.array([0., .05, .5, .95, 1.])
P_SCI = .9


@pytest.fixture(scope="module")
def bd():
    from montecosmo_amd import bdec
    return bdec


def _draws(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _dev(a, gpu, misaligned=False, pad_draws=0):
    """(C, N, D) on the device; misaligned: one element into a buffer; pad_draws: chains N + pad_draws draws apart (stride_chain != N stride_draw)."""
    a = np.asarray(a)
    c, n, d = a.shape
    buf = torch.zeros(c * (n + pad_draws) * d + 1, dtype=torch.float32, device=gpu)
    view = buf[1 if misaligned else 0:][:c * (n + pad_draws) * d].reshape(c, n + pad_draws, d)[:, :n]
    view.copy_(torch.from_numpy(np.array(a, order="C")).to(gpu))
    assert (view.data_ptr() % 16 != 0) == misaligned
    return view


def _one_call(bd, t, truth, L, ranks):
    """Everything one kernel call (or the general path) makes, as numpy arrays."""
    st = bd._dev_stats(t, ranks=ranks, L=L, truth=truth, want_sorted=True)
    return {k: v.cpu().numpy() for k, v in st.items()}


def _check_one_call(got, pooled, truth, L, ranks):
    m, d = pooled.shape
    xs = ref.sort_total(pooled)
    assert got["sorted"].dtype == np.float32 and got["sci_idx"].dtype == np.int32 and got["below"].dtype == np.int32
    np.testing.assert_array_equal(got["sorted"], xs)
    np.testing.assert_array_equal(np.signbit(got["sorted"]), np.signbit(xs))
    np.testing.assert_array_equal(got["rank"], xs[ranks])
    low, high, idx = ref.sci_noweights(pooled, (L + .25) / m if L < m - 1 else 1.)
    assert ref.sci_length((L + .25) / m if L < m - 1 else 1., m) == L
    np.testing.assert_array_equal(got["sci"][0], low)
    np.testing.assert_array_equal(got["sci"][1], high)
    np.testing.assert_array_equal(got["sci_idx"], idx)
    below, equal = ref.counts(pooled, truth)
    np.testing.assert_array_equal(got["below"], below)
    np.testing.assert_array_equal(got["equal"], equal)


def _check_quantile(q, pooled, ps):
    xs = ref.sort_total(pooled)
    n = xs.shape[0]
    want = ref.quantile(pooled, ps)
    assert q.dtype == np.float64 and q.shape == want.shape
    worst = 0.
    for j, pj in enumerate(ps):
        if n == 1:
            np.testing.assert_array_equal(q[j], want[j])
            continue
        i = ref.rank_high(pj, n)
        scale = np.maximum(np.abs(xs[i - 1]), np.abs(xs[i]))
        ok = np.isfinite(want[j]) & np.isfinite(scale)
        np.testing.assert_array_equal(q[j][~ok], want[j][~ok])
        err = np.abs(q[j][ok] - want[j][ok])
        if ok.any() and scale[ok].max() > 0:
            worst = max(worst, float((err[scale[ok] > 0] / scale[ok][scale[ok] > 0]).max(initial=0.)))
        assert np.all(err <= 1e-12 * scale[ok])
    print("quantile: worst |q - ref| / max(|x_(i-1)|, |x_(i)|) =", worst)


def _public(bd, x, truth):
    ci, idx = bd.sci_noweights(x, P_SCI, axis=(0, 1), backend="hip", return_index=True)
    below, equal = bd.rank_counts(x, truth, axis=(0, 1), backend="hip")
    return dict(ci=ci, idx=idx, q=bd.quantile(x, PS, axis=(0, 1), backend="hip"), below=below, equal=equal,
                sorted=bd.sort_draws(x, axis=(0, 1), backend="hip"), med=bd.qbci(x, .8, axis=(0, 1), backend="hip"))


def _assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(np.signbit(a[k]), np.signbit(b[k]), err_msg=k)


# (C, N): M = 1, 2, 3, 63, 64, 65, 1000, 1025; three chains at M = 3 and 63
SHAPES = [(1, 1), (1, 2), (3, 1), (3, 21), (1, 64), (1, 65), (1, 1000), (1, 1025)]


@pytest.mark.parametrize("d", [1, 63, 65, 257])
@pytest.mark.parametrize("c,n", SHAPES)
def test_shapes_aligned_and_misaligned(gpu, bd, c, n, d):
    x = _draws(100 * n + d, (c, n, d))
    pooled = x.reshape(c * n, d).astype(np.float64)
    m = c * n
    truth = _draws(7, (d,))
    truth[::3] = x[c - 1, n // 2, ::3]      # some truths are draws: equal counts of one
    L = ref.sci_length(P_SCI, m)
    ranks = sorted({0, m // 2, m - 1})
    got = []
    for mis in (False, True):
        t = _dev(x, gpu, mis, pad_draws=2)
        assert t.stride(0) != n * t.stride(1)
        got.append(_one_call(bd, t, truth, L, ranks))
        _check_one_call(got[-1], pooled, truth, L, ranks)
    _assert_same(*got)
    q = bd.quantile(t, PS, axis=(0, 1), backend="hip")
    _check_quantile(q, pooled, PS)
    ci, idx = bd.sci_noweights(t, P_SCI, axis=(0, 1), backend="hip", return_index=True)
    assert ci.shape == (d, 2) and ci.dtype == np.float64
    np.testing.assert_array_equal(ci, got[0]["sci"].T.astype(np.float64))
    np.testing.assert_array_equal(idx, got[0]["sci_idx"])
    np.testing.assert_array_equal(bd.quantile(t, PS, axis=(0, 1)), q)      # 'auto' takes the device for float32 draws


@pytest.mark.parametrize("c,n", [(4, 1000), (1, 5000), (3, 3000), (2, 16384), (1, 32769)])
def test_every_tile_shape_up_to_the_real_threshold(gpu, bd, c, n):
    """Rows of 4096, 8192, 16384 and 32768 keys: tiles of 8, 4, 2 and 1 dimensions, the last tile ragged (D = 9); 4 x 1000 is the shape the
    field is run at, 2 x 16384 fills the largest row the LDS holds, and one draw more takes the general path."""
    d = 9
    m = c * n
    assert (m <= bd.LDS_MAX_M) == (m != 32769)
    x = _draws(m, (c, n, d))
    pooled = x.reshape(m, d).astype(np.float64)
    truth = _draws(9, (d,))
    L = ref.sci_length(.95, m)
    ranks = [0, 1, m // 3, m - 2, m - 1]
    t = _dev(x, gpu, misaligned=True, pad_draws=1)
    got = _one_call(bd, t, truth, L, ranks)
    _check_one_call(got, pooled, truth, L, ranks)
    _check_quantile(bd.quantile(t, PS, axis=(0, 1), backend="hip"), pooled, PS)


@pytest.mark.parametrize("m", [100, 101])
def test_either_side_of_the_lds_threshold(gpu, bd, monkeypatch, m):
    """With the threshold at 100 pooled draws, 100 go through the kernel and 101 through the general path; both equal the restatement, and the
    general path equals the kernel on the same draws."""
    d = 65
    x = _draws(m, (1, m, d))
    pooled = x[0].astype(np.float64)
    truth = _draws(8, (d,))
    L = ref.sci_length(P_SCI, m)
    ranks = [0, 17, m - 1]
    kernel = [_one_call(bd, _dev(x, gpu, mis), truth, L, ranks) for mis in (False, True)]
    calls = []
    real = bd._dev_general
    monkeypatch.setattr(bd, "_dev_general", lambda *a: calls.append(1) or real(*a))
    monkeypatch.setattr(bd, "LDS_MAX_M", 100)
    for mis in (False, True):
        t = _dev(x, gpu, mis)
        got = _one_call(bd, t, truth, L, ranks)
        _check_one_call(got, pooled, truth, L, ranks)
        _assert_same(got, kernel[0])
        _check_quantile(bd.quantile(t, PS, axis=(0, 1), backend="hip"), pooled, PS)
    assert len(calls) == (0 if m == 100 else 4)
    _assert_same(kernel[0], kernel[1])


def _adversarial(m):
    rng = np.random.default_rng(11)
    base = np.sort(rng.standard_normal(m)).astype(np.float32)
    cols = [base, base[::-1], np.full(m, 1.5, np.float32), np.where(rng.random(m) < .5, -2., 3.).astype(np.float32),
            np.where(rng.random(m) < .5, -0., 0.).astype(np.float32)]
    inf = rng.standard_normal(m).astype(np.float32)
    inf[rng.random(m) < .3] = np.inf
    inf[rng.random(m) < .3] = -np.inf
    one_nan = rng.standard_normal(m).astype(np.float32)
    one_nan[m // 3] = np.nan
    neg_nan = rng.standard_normal(m).astype(np.float32)
    neg_nan[[0, m - 1]] = -np.nan      # a NaN with its sign bit set is a NaN like the others: last
    all_inf = np.full(m, np.inf, np.float32)
    cols += [inf, one_nan, neg_nan, np.full(m, np.nan, np.float32), all_inf]
    return np.stack(cols, axis=1)[None]      # (1, m, 10)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("m", [2, 65])
def test_adversarial_rows(gpu, bd, monkeypatch, m, general):
    """Sorted, reversed, all equal, two values, +-0 mixed, +-inf, one NaN, negative NaNs, all NaN, all +inf; L = 0, M - 1 and in between;
    through the kernel and through the general path."""
    if general:
        monkeypatch.setattr(bd, "LDS_MAX_M", 1)
    x = _adversarial(m)
    assert np.signbit(x[0, :, 4]).any() and not np.signbit(x[0, :, 4]).all() and np.signbit(x[0, 0, 7])
    pooled = x[0].astype(np.float64)
    truth = np.array([x[0, m // 2, 0], 0., 1.5, 3., -0., np.inf, 0., 0., 0., np.inf], dtype=np.float32)
    t = _dev(x, gpu)
    for L in sorted({0, m // 2, m - 1}):
        got = _one_call(bd, t, truth, L, [0, m - 1])
        _check_one_call(got, pooled, truth, L, [0, m - 1])
        assert np.isnan(got["sci"][:, 6:9]).all() and np.all(got["sci_idx"][6:9] == -1) and np.all(got["sci_idx"][[2, 9]] == 0)
    assert np.isnan(got["sorted"][m - 1, 6:9]).all() and np.isnan(got["sorted"][:, 8]).all()
    if m > 2:
        assert not np.isnan(got["sorted"][:m - 2, 7]).any() and np.isnan(got["sorted"][m - 2:, 7]).all()
    with np.errstate(all="ignore"):
        _check_quantile(bd.quantile(t, PS, axis=(0, 1), backend="hip"), pooled, PS)


def test_repeat_is_bitwise(gpu, bd):
    x = _draws(21, (3, 70, 130))
    truth = _draws(22, (130,))
    t = _dev(x, gpu, pad_draws=1)
    _assert_same(_public(bd, t, truth), _public(bd, t, truth))


def test_a_dimension_does_not_know_its_neighbours(gpu, bd):
    x = _draws(23, (2, 150, 257))
    truth = _draws(24, (257,))
    whole = _public(bd, _dev(x, gpu), truth)
    for col in (0, 31, 32, 256):
        alone = _public(bd, _dev(x[:, :, col:col + 1], gpu), truth[col:col + 1])
        other = x.copy()
        other[:, :, :col] = 7.
        other[:, :, col + 1:] = np.nan
        among = _public(bd, _dev(other, gpu), truth)
        for k, v in whole.items():
            np.testing.assert_array_equal(alone[k][..., 0, :] if k in ("ci", "med") else alone[k][..., 0],
                                          v[..., col, :] if k in ("ci", "med") else v[..., col], err_msg=k)
            np.testing.assert_array_equal(among[k][..., col, :] if k in ("ci", "med") else among[k][..., col],
                                          v[..., col, :] if k in ("ci", "med") else v[..., col], err_msg=k)
    perm = np.random.default_rng(0).permutation(257)
    moved = _public(bd, _dev(x[:, :, perm], gpu), truth[perm])
    for k, v in whole.items():
        np.testing.assert_array_equal(moved[k], v[..., perm, :] if k in ("ci", "med") else v[..., perm], err_msg=k)


def test_strided_views_equal_their_copies(gpu, bd):
    from montecosmo_amd import chains
    flat = _draws(25, (3, 40, 3 + 4 * 5 + 70))
    t = _dev(flat, gpu)
    for a, b in ((0, 1), (1, 3), (3, 23), (23, 93)):      # a slice flat[:, :, a:b] of flat states
        view = t[:, :, a:b]
        assert b - a == 1 or not view.is_contiguous()
        truth = _draws(26, (b - a,))
        _assert_same(_public(bd, view, truth), _public(bd, _dev(flat[:, :, a:b], gpu), truth))
    truth = _draws(27, (93,))
    _assert_same(_public(bd, t[:, ::2], truth), _public(bd, _dev(flat[:, ::2], gpu), truth))      # every second draw
    ch = chains.Chains.from_flat(t, {"a": (0, 1, ()), "w": (3, 23, (4, 5))}, backend="hip")
    assert ch["w"].data_ptr() == t.data_ptr() + 12 and not ch["w"].is_contiguous()
    np.testing.assert_array_equal(ch.credint()["w"], bd.sci_noweights(_dev(flat[:, :, 3:23], gpu), .95, axis=(0, 1)).reshape(4, 5, 2))
    np.testing.assert_array_equal(ch.quantile(PS)["a"], bd.quantile(_dev(flat[:, :, 0:1], gpu), PS, axis=(0, 1))[:, 0])


@pytest.mark.parametrize("general", [False, True])
def test_chunked_upload_of_host_arrays_is_bitwise_the_resident_call(gpu, bd, monkeypatch, general):
    from montecosmo_amd import chains, metrics
    if general:
        monkeypatch.setattr(bd, "LDS_MAX_M", 64)
    x = _draws(28, (4, 57, 65))
    truth = _draws(29, (65,))
    want = _public(bd, _dev(x, gpu), truth)
    monkeypatch.setattr(metrics, "CHUNK_BYTES", 4 * 4 * 57 * 25)      # 25 of the 65 dimensions per upload: three chunks
    uploads = []
    real = chains._Resident
    monkeypatch.setattr(chains, "_Resident", lambda t: uploads.append(t.shape[2]) or real(t))
    ci = bd.sci_noweights(x, P_SCI, axis=(0, 1), backend="hip")
    assert uploads == [25, 25, 15]
    np.testing.assert_array_equal(ci, want["ci"])
    _assert_same(_public(bd, x, truth), want)
    _assert_same(_public(bd, torch.from_numpy(x.copy()), truth), want)      # a host tensor goes the same way


@pytest.mark.parametrize("general", [False, True])
def test_peak_memory_stays_under_the_outputs_and_two_chunks(gpu, bd, monkeypatch, general):
    """A condition of the design: beside resident draws the call allocates its outputs and at most 2 CHUNK_BYTES of scratch."""
    from montecosmo_amd import metrics
    chunk = 1 << 20
    monkeypatch.setattr(metrics, "CHUNK_BYTES", chunk)
    if general:
        monkeypatch.setattr(bd, "LDS_MAX_M", 64)
    c, n, d = 2, 600, 2000      # 9.6 MB of draws
    g = torch.Generator(device=gpu).manual_seed(3)
    t = torch.randn((c, n, d), device=gpu, generator=g)
    ps = [.05, .5, .95]
    bd.quantile(t[:, :, :8], ps, axis=(0, 1), backend="hip"), bd.sci_noweights(t[:, :, :8], .95, axis=(0, 1), backend="hip")      # (code objects loaded)
    # outputs on the device: the values at the six ranks (float32) and the three float64 quantiles; the interval (float32 pair, its
    # float64 copy), its index and the one rank every call returns
    for what, fn, out_bytes in (("quantile", lambda: bd.quantile(t, ps, axis=(0, 1), backend="hip"), (6 * 4 + 3 * 8) * d),
                                ("credint", lambda: bd.sci_noweights(t, .95, axis=(0, 1), backend="hip"), (2 * 4 + 4 + 4 + 2 * 8) * d)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(gpu)
        before = torch.cuda.max_memory_allocated(gpu)
        fn()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(gpu) - before
        print(what, "general" if general else "lds", "rise", rise, "outputs", out_bytes, "bound", out_bytes + 2 * chunk)
        assert rise < out_bytes + 2 * chunk
        assert rise < c * n * d * 4 / 2      # and nothing near the size of the draws


def test_indexing_past_2_to_the_31(gpu, bd):
    n, d, far = 16, 5, 2 ** 31
    x = _draws(30, (2, n, d))
    truth = _draws(31, (d,))
    buf = torch.empty(far + 4096, dtype=torch.float32, device=gpu)
    buf[:n * d] = torch.from_numpy(x[0].copy()).to(gpu).reshape(-1)
    buf[far:far + n * d] = torch.from_numpy(x[1].copy()).to(gpu).reshape(-1)
    view = buf.as_strided((2, n, d), (far, d, 1))      # the two chains 2^31 elements apart: read in place by stride_chain
    got = _public(bd, view, truth)
    _assert_same(got, _public(bd, _dev(x, gpu), truth))
    np.testing.assert_array_equal(got["sorted"], ref.sort_total(x.reshape(2 * n, d).astype(np.float64)))
    del buf, view


def test_error_codes_launch_nothing(gpu):
    from montecosmo_amd import _lib
    c, n, d = 2, 8, 4
    x = torch.zeros(c * n * d, dtype=torch.float32, device=gpu)
    f = lambda *shape: torch.full(shape, 7., dtype=torch.float32, device=gpu)
    i = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=gpu)
    out, sci, sci_idx, truth, below, equal, srt = f(2, d), f(2, d), i(d), f(d), i(d), i(d), f(c * n, d)
    s = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    ranks = (C.c_int * 2)(0, 15)
    E_ARG, E_UNSUPPORTED = -6, -8
    good = (s, x, 0, d, c, n * d, n, d, ranks, 2, out, 3, sci, sci_idx, truth, below, equal, srt)
    args = _lib.marshal("mcpm_bdec_sort_f32", good)
    lib = _lib.lib
    bad = [(1, None), (8, None), (10, None), (9, 0), (9, 65), (8, (C.c_int * 2)(0, 16)), (8, (C.c_int * 2)(-1, 3)), (11, -1), (11, 16), (13, None),
           (15, None), (16, None), (5, -1), (7, -1), (2, -1), (3, 0), (4, 0), (6, 0)]
    for pos, value in bad:
        a = list(args)
        a[pos] = value
        assert lib.mcpm_bdec_sort_f32(*a) == E_ARG, (pos, value)
    a = list(args)
    a[4], a[6], a[8] = 1, 32769, (C.c_int * 2)(0, 1)      # one row above the LDS tile
    assert lib.mcpm_bdec_sort_f32(*a) == E_UNSUPPORTED
    with pytest.raises(_lib.McpmError, match="mcpm_bdec_sort_f32 failed with code -6"):
        _lib.call("mcpm_bdec_sort_f32", *good[:9], 0, *good[10:])
    torch.cuda.synchronize()
    for t in (out, sci, sci_idx, truth, below, equal, srt):
        assert torch.all(t == 7)
    assert lib.mcpm_bdec_sort_f32(*args) == 0      # and the same arguments, unspoilt, do run
    torch.cuda.synchronize()
    assert torch.all(srt == 0) and torch.all(sci == 0) and torch.all(sci_idx == 0) and torch.all(below == c * n) and torch.all(equal == 0)


def test_end_to_end_credint_and_coverage(gpu):
    """4 x 500 draws of a 17-dimensional Gaussian posterior with the truth drawn from the same law: the intervals and the coverage are
    exactly the restatement's (no statistical gate)."""
    from montecosmo_amd import chains
    rng = np.random.default_rng(32)
    mean, std = rng.standard_normal(17), .5 + rng.random(17)
    flat = (mean + std * rng.standard_normal((4, 500, 17))).astype(np.float32)
    truth = {"b": mean[:1].reshape(()) + std[0] * rng.standard_normal(()), "f": (mean[1:] + std[1:] * rng.standard_normal(16)).reshape(4, 4)}
    t = torch.from_numpy(flat).to(gpu)
    ch = chains.Chains.from_flat(t, {"b": (0, 1, ()), "f": (1, 17, (4, 4))})
    pooled = flat.reshape(2000, 17).astype(np.float64)
    for p in (.95, .5):
        ci = ch.credint(p)
        low, high, _ = ref.sci_noweights(pooled, p)
        assert ci["b"].shape == (2,) and ci["f"].shape == (4, 4, 2)
        np.testing.assert_array_equal(ci["b"], [low[0], high[0]])
        np.testing.assert_array_equal(ci["f"].reshape(16, 2), np.stack([low[1:], high[1:]], axis=-1))
        cov = ch.coverage(truth, p)
        assert cov["b"] == ref.coverage(pooled[:, :1], truth["b"], p) and cov["f"] == ref.coverage(pooled[:, 1:], truth["f"], p)
    med = ch.credint(.9, type="med")["f"].reshape(16, 2)
    p_low = (1. - np.float64(.9)) / 2.
    _check_quantile(np.moveaxis(med, -1, 0), pooled[:, 1:], np.array([p_low, p_low + .9]))
    np.testing.assert_array_equal(ch.quantile([.5])["f"], chains.quantile(ch["f"], [.5]))
    host = chains.Chains.from_flat(flat.astype(np.float64), {"f": (1, 17, (4, 4))}, backend="host")
    np.testing.assert_array_equal(host.credint()["f"], ch.credint()["f"])      # float64 copies of the same float32 draws on the host
    assert host.coverage({"f": truth["f"]}) == ch.coverage({"f": truth["f"]})
