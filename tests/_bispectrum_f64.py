"""Float64 numpy restatement of the binned bispectrum (montecosmo_amd/metrics.py `bispectrum`), the checker of
tests/test_bispectrum_host.py and tests/test_gpu_bispectrum.py.  Two estimators of the same numbers: the FFT (Scoccimarro) one, shell
fields F_b and sums over cells, exactly as metrics.bispectrum defines it, and a direct sum of d(k1) d(k2) d(k3) over all mode triples
of the full FFT that close modulo the mesh.  Wavevectors and the paint window come from the oracle, as in _spectrum_f64.py."""
import numpy as np

from oracle import pm_oracle as o

import _spectrum_f64 as spec_ref


def all_triangles(n_bins):
    return np.array([(i, j, l) for i in range(n_bins) for j in range(i, n_bins) for l in range(j, n_bins)], dtype=np.int64)


def _half_spectrum(mesh, mesh_shape, deconv):
    """(d, mesh_shape): float64 rfftn of a real mesh, or the complex input itself, divided by the paint window."""
    mesh = np.asarray(mesh)
    if np.iscomplexobj(mesh):
        d = mesh.astype(np.complex128)
        mesh_shape = tuple(mesh_shape or o.ch2rshape(mesh.shape))
    else:
        d = np.fft.rfftn(mesh.astype(np.float64))
        mesh_shape = tuple(mesh.shape)
    return d / o.rectangular_hat(o.rfftk(mesh_shape), order=deconv), mesh_shape


def shell_fields(d, mesh_shape, box_size, kedges):
    """F_b(x) = sum_{k in bin b} d(k) e^{ikx}, [n_bins, *mesh_shape]: M * irfftn of the half-spectrum masked to bin b."""
    kx, ky, kz = o.rfftk(tuple(mesh_shape), np.asarray(box_size, dtype=np.float64))
    kmesh = np.sqrt((kx ** 2 + ky ** 2) + kz ** 2)
    dig = np.digitize(kmesh, kedges) - 1
    M = np.prod(mesh_shape)
    return np.stack([M * np.fft.irfftn(np.where(dig == b, d, 0.), s=mesh_shape, axes=(0, 1, 2)) for b in range(len(kedges) - 1)])


def bispectrum(mesh, box_size=None, kedges=None, triangles=None, deconv=0, mesh_shape=None):
    """The FFT estimator in float64.  Returns a dict: S = sum_x F_i F_j F_l and A = sum_x |F_i F_j F_l| (the scale against which a
    rounding error of S is judged), SN and AN the same of the indicator fields I_b, ntri = SN / M, bk = (V^2 / M^3) (S / M) / ntri,
    kmean and pk of the same bins, qk = bk / (P_i P_j + P_j P_l + P_l P_i); every per-triangle array follows `triangles`."""
    d, mesh_shape = _half_spectrum(mesh, mesh_shape, deconv)
    box_size = np.asarray(mesh_shape, dtype=np.float64) if box_size is None else np.asarray(box_size, dtype=np.float64)
    kedges = np.asarray(kedges, dtype=np.float64)
    tri = all_triangles(len(kedges) - 1) if triangles is None else np.asarray(triangles, dtype=np.int64)
    M, V = float(np.prod(mesh_shape)), float(box_size.prod())
    F = shell_fields(d, mesh_shape, box_size, kedges)
    I = shell_fields(np.ones_like(d), mesh_shape, box_size, kedges)
    S = np.array([np.sum(F[i] * F[j] * F[l]) for i, j, l in tri])
    A = np.array([np.sum(np.abs(F[i] * F[j] * F[l])) for i, j, l in tri])
    SN = np.array([np.sum(I[i] * I[j] * I[l]) for i, j, l in tri])
    AN = np.array([np.sum(np.abs(I[i] * I[j] * I[l])) for i, j, l in tri])
    _, kmean, pk, _ = spec_ref.spectrum(d, box_size=box_size, kedges=list(kedges), mesh_shape=mesh_shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ntri = SN / M
        bk = (V ** 2 / M ** 3) * (S / M) / ntri
        qk = bk / (pk[tri[:, 0]] * pk[tri[:, 1]] + pk[tri[:, 1]] * pk[tri[:, 2]] + pk[tri[:, 2]] * pk[tri[:, 0]])
    return dict(tri=tri, S=S, A=A, SN=SN, AN=AN, ntri=ntri, bk=bk, kmean=kmean, pk=pk, qk=qk, F=F, I=I)


def direct(mesh, box_size=None, kedges=None, triangles=None, deconv=0, mesh_shape=None):
    """(S / M, ntri) by the direct sum: over every ordered triple of modes of the FULL FFT with k1 in bin i, k2 in bin j, k3 in bin l and
    k1 + k2 + k3 = 0 modulo the mesh, the sum of d(k1) d(k2) d(k3) (real up to rounding: the conjugate triple is in the sum too) and the
    integer count of the triples."""
    d, mesh_shape = _half_spectrum(mesh, mesh_shape, deconv)
    box_size = np.asarray(mesh_shape, dtype=np.float64) if box_size is None else np.asarray(box_size, dtype=np.float64)
    kedges = np.asarray(kedges, dtype=np.float64)
    tri = all_triangles(len(kedges) - 1) if triangles is None else np.asarray(triangles, dtype=np.int64)
    full = np.fft.fftn(np.fft.irfftn(d, s=mesh_shape, axes=(0, 1, 2)))      # the full spectrum of the (deconvolved) real mesh
    kx, ky, kz = o.fftk(tuple(mesh_shape), box_size)
    dig = (np.digitize(np.sqrt((kx ** 2 + ky ** 2) + kz ** 2), kedges) - 1).reshape(-1)
    full = full.reshape(-1)
    idx = np.stack(np.unravel_index(np.arange(full.size), mesh_shape), axis=1)      # integer mode numbers, modulo the mesh
    shape = np.asarray(mesh_shape)
    sums, counts = np.zeros(len(tri)), np.zeros(len(tri), dtype=np.int64)
    for t, (i, j, l) in enumerate(tri):
        m1, m2 = np.flatnonzero(dig == i), np.flatnonzero(dig == j)
        if not len(m1) or not len(m2):
            continue
        k3 = (-(idx[m1][:, None, :] + idx[m2][None, :, :])) % shape
        f3 = np.ravel_multi_index((k3[..., 0], k3[..., 1], k3[..., 2]), mesh_shape)
        ok = dig[f3] == l
        counts[t] = ok.sum()
        sums[t] = np.sum((full[m1][:, None] * full[m2][None, :] * full[f3])[ok]).real
    return sums, counts
