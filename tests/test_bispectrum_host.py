"""Host side of the binned bispectrum (montecosmo_amd/metrics.py `bispectrum`): the float64 FFT restatement tests/_bispectrum_f64.py
against a direct sum over closed mode triples and against analytic plane waves, the default edges and triangle list, and the new
symbols of the C ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from montecosmo_amd import metrics
import _bispectrum_f64 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", [(8, 6, 4), (6, 6, 6), (4, 10, 6)])
def test_fft_estimator_equals_direct_sum(shape):
    """S / M is the sum of d(k1) d(k2) d(k3) over the closed triples and ntri their count, also where the edges run past the Nyquist
    wavenumber and triples close only modulo the mesh.  Found here: 7e-16 of A; the gate leaves room for another FFT back end."""
    rng = np.random.default_rng(sum(shape))
    g = rng.standard_normal(shape)
    mesh = g + 0.5 * (g ** 2 - 1)
    box = np.asarray(shape, dtype=np.float64)
    kf, knyq = 2 * np.pi / box.max(), np.pi
    edges = np.linspace(0.5 * kf, 1.8 * knyq, 5)
    r = ref.bispectrum(mesh, box_size=box, kedges=edges)
    assert len(r["tri"]) == 20
    s_dir, n_dir = ref.direct(mesh, box_size=box, kedges=edges)
    M = np.prod(shape)
    err = np.abs(r["S"] / M - s_dir) * M
    print("max |S - S_direct| / A =", np.max(err / r["A"]))
    assert np.all(err <= 1e-12 * r["A"])
    assert n_dir.sum() > 0
    np.testing.assert_array_equal(np.rint(r["ntri"]).astype(np.int64), n_dir)
    assert np.all(np.abs(r["ntri"] - n_dir) <= 1e-12 * r["AN"] / M)


def test_plane_waves():
    """Three collinear waves 2 A_a cos(k_a x + phi_a) with k_1 + k_2 + k_3 = 0, each alone (with its conjugate) in a narrow bin of an
    anisotropic box: S / M = 2 Re(c_1 c_2 c_3) with c_a = M A_a e^{i phi_a}, from the two closed triples (k_1, k_2, k_3) and its conjugate."""
    shape, box = (12, 10, 8), np.array([12., 10.7, 8.3])
    ms = np.array([[1, 0, 0], [3, 0, 0], [-4, 0, 0]])      # (on 12 cells 4 + 4 + 4 closes too, modulo the mesh: triangle (4, 4, 4))
    amp, phi = np.array([0.7, 1.3, 0.4]), np.array([0.3, -1.1, 2.0])
    x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    mesh = sum(2 * a * np.cos(2 * np.pi * sum(mi * xi / n for mi, xi, n in zip(m, x, shape)) + p) for m, a, p in zip(ms, amp, phi))
    kabs = 2 * np.pi * np.abs(ms[:, 0]) / box[0]
    edges = np.concatenate([[.99 * k, 1.01 * k] for k in kabs])      # bins 0, 2, 4 hold the waves, 1 and 3 lie between them
    r = ref.bispectrum(mesh, box_size=box, kedges=edges)
    M = np.prod(shape)
    c = M * amp * np.exp(1j * phi)
    expect = 2 * (c[0] * c[1] * c[2]).real
    t = [tuple(row) for row in r["tri"]].index((0, 2, 4))
    assert abs(r["S"][t] / M - expect) <= 1e-12 * abs(expect)
    assert abs(r["ntri"][t] - 2) <= 1e-12
    others = np.array([bool({1, 3} & set(row)) for row in r["tri"]])      # triangles not made of the three waves' bins
    assert others.sum() == 25 and np.all(np.abs(r["S"][others] / M) <= 1e-12 * abs(expect))
    s_dir, n_dir = ref.direct(mesh, box_size=box, kedges=edges)
    assert n_dir[t] == 2 and abs(s_dir[t] - expect) <= 1e-12 * abs(expect)
    assert np.all(np.abs(r["S"] / M - s_dir) <= 1e-12 * abs(expect))      # (the aliased (4, 4, 4) among them)
    t444 = [tuple(row) for row in r["tri"]].index((4, 4, 4))
    assert abs(r["S"][t444] / M - 2 * (c[2] ** 3).real) <= 1e-12 * abs(expect)


def test_default_edges_and_triangles():
    shape, box = (64, 48, 40), (640., 480., 500.)
    edges = metrics._bispec_edges(shape, box)
    kmax = 2 / 3 * np.pi * min(64 / 640., 48 / 480., 40 / 500.)
    n = int(kmax / (3 * 2 * np.pi / 480.))
    assert n == 4 and len(edges) == n
    np.testing.assert_allclose(edges, (np.arange(n) + .5) * kmax / n, rtol=1e-15)
    assert edges[-1] < kmax
    np.testing.assert_allclose(metrics._bispec_edges(shape, box, 7), (np.arange(7) + .5) * kmax / 7, rtol=1e-15)
    assert len(metrics._bispec_edges(shape, box, 0.02)) == int(kmax / 0.02)
    np.testing.assert_array_equal(metrics._bispec_edges(shape, box, [0.01, 0.02, 0.05]), [0.01, 0.02, 0.05])
    # the closure rule: i <= j <= l and the lower edge of l below the sum of the upper edges of i and j
    e = np.array([0., 1., 2., 3., 4.5, 9.])
    tri = metrics._bispec_triangles(e)
    want = [(i, j, l) for i in range(5) for j in range(i, 5) for l in range(j, 5) if e[l] < e[i + 1] + e[j + 1]]
    assert [tuple(t) for t in tri] == want and (0, 0, 2) not in want and (0, 0, 1) in want and (0, 1, 4) not in want
    # equal-width bins from zero: every (i, j, l) with l <= i + j + 1
    tri = metrics._bispec_triangles(np.arange(7.))
    assert all(l <= i + j + 1 for i, j, l in tri) and len(tri) == sum(1 for i in range(6) for j in range(i, 6) for l in range(j, 6) if l <= i + j + 1)
    # the caps
    assert metrics.MAX_BISPEC_BINS == 32 and metrics.MAX_TRIANGLES == 8192
    assert len(metrics._bispec_edges(shape, box, list(np.linspace(0.01, 0.3, 33)))) == 33
    with pytest.raises(ValueError):
        metrics._bispec_edges(shape, box, list(np.linspace(0.01, 0.3, 34)))
    with pytest.raises(ValueError):
        metrics._bispec_edges((512, 512, 512), (1000., 1000., 1000.))      # the default spacing would give 56 edges
    with pytest.raises(ValueError):
        metrics._bispec_edges(shape, box, [0.1, 0.3, 0.2])
    with pytest.raises(ValueError):
        metrics._bispec_triangles(e, np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        metrics._bispec_triangles(e, np.zeros((metrics.MAX_TRIANGLES + 1, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        metrics._bispec_triangles(e, [[0, 1, 5]])
    with pytest.raises(ValueError):
        metrics._bispec_triangles(e, [[0., 1., 2.]])
    assert len(metrics._bispec_triangles(np.arange(33.))) <= metrics.MAX_TRIANGLES      # 32 bins: the default list fits


def test_new_symbols_declared_and_exported():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("mcpm_bispectrum_workspace", "mcpm_bispectrum_split_c64", "mcpm_bispectrum_sums_f32"):
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert "#define MCPM_BISPECTRUM_MAX_BINS 32" in header and "#define MCPM_BISPECTRUM_MAX_TRIANGLES 8192" in header
    assert '#define MCPM_ABI_VERSION "mcpm 0.12 (gfx950)"' in header
    assert _lib.lib.mcpm_version() == b"mcpm 0.12 (gfx950)"      # three symbols added, nothing changed: the ABI string stays
    # argument errors come back as codes before anything is launched
    n = C.c_int64(-1)
    assert _lib.lib.mcpm_bispectrum_workspace(16, 12, 10, 4, 20, 1, C.byref(n)) == 0 and n.value > 0
    assert _lib.lib.mcpm_bispectrum_workspace(16, 12, 9, 4, 20, 1, C.byref(n)) == -1       # MCPM_E_SHAPE: odd nz
    for bad in ((16, 12, 10, 33, 20, 1), (16, 12, 10, 4, 0, 1), (16, 12, 10, 4, 8193, 1), (16, 12, 10, 4, 20, 0)):
        assert _lib.lib.mcpm_bispectrum_workspace(*bad, C.byref(n)) == -6      # MCPM_E_ARG
    with pytest.raises(_lib.McpmError):
        _lib.call("mcpm_bispectrum_workspace", 16, 12, 10, 33, 20, 1, C.byref(n))
    assert _lib.lib.mcpm_bispectrum_sums_f32(None, None, 100, 4, 1, None, 20, None, 0, None) == -6
    edges = np.array([0.1, 0.3, 0.2])
    ktab = np.zeros(16 + 12 + 6)
    f64p = C.POINTER(C.c_double)
    assert _lib.lib.mcpm_bispectrum_split_c64(None, 16, 12, 10, None, 0, 1, ktab.ctypes.data_as(f64p), None, edges.ctypes.data_as(f64p), 3,
                                              None) == -6      # null output, before the edges are looked at
