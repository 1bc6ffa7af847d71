"""Float64 numpy restatement of the binned spectrum estimator (montecosmo/metrics.py `_waves` / `_spectrum`), the checker of
tests/test_spectrum_host.py and tests/test_gpu_spectrum.py.  Wavevectors, the paint window and safe division come from the
oracle; the binning is np.digitize + np.bincount on the full half-spectrum mesh."""
import numpy as np
from scipy.special import legendre

from oracle import pm_oracle as o


def waves(mesh_shape, box_size, kedges, include_corners, los):
    """(kedges, kmesh, mumesh, rfftw) of `_waves`: edges from None / int / float / list, |k|, mu and the Hermitian weights."""
    mesh_shape = np.asarray(mesh_shape)
    box_size = np.asarray(box_size, dtype=np.float64)
    kx, ky, kz = o.rfftk(tuple(int(s) for s in mesh_shape), box_size)
    kmesh = np.sqrt((kx ** 2 + ky ** 2) + kz ** 2)
    mumesh = o.safe_div((kx * los[0] + ky * los[1]) + kz * los[2], kmesh)
    if kedges is None or isinstance(kedges, (int, float)):
        kmin = 0.
        kmax = kmesh.max() if include_corners else np.pi * (mesh_shape / box_size).min()
        if kedges is None:
            n = max(int((kmax - kmin) / (len(mesh_shape) ** .5 * 2 * np.pi / box_size.min())), 1)
        elif isinstance(kedges, int):
            n = kedges
        else:
            n = max(int((kmax - kmin) / kedges), 1)
        dk = (kmax - kmin) / n
        kedges = np.linspace(kmin, kmax, n, endpoint=False) + dk / 2
    rfftw = np.full(kmesh.shape, 2.)
    rfftw[..., 0] = 1.
    if mesh_shape[-1] % 2 == 0:
        rfftw[..., -1] = 1.
    return np.asarray(kedges, dtype=np.float64), kmesh, mumesh, rfftw


def spectrum(mesh0, mesh1=None, box_size=None, box_center=(0., 0., 0.), ells=0, kedges=None, include_corners=True,
             deconv=(0, 0), mesh_shape=None):
    """(kcount, kmean, pow, pabs) of `_spectrum` in float64.  Complex inputs are half-spectra (give `mesh_shape` when nz is
    not 2 (nzh - 1)); real inputs are transformed with np.fft.rfftn.  `pabs` is the same bin sum of |weights|: the scale
    against which a bin's rounding error is judged (equal to |pow| for an auto monopole)."""
    box_center = np.asarray(box_center, dtype=np.float64)
    los = o.safe_div(box_center, np.linalg.norm(box_center))
    if isinstance(deconv, int):
        deconv = (deconv, deconv)

    def spec(m):
        m = np.asarray(m)
        if np.iscomplexobj(m):
            return m.astype(np.complex128)
        return np.fft.rfftn(m.astype(np.float64))

    real_shape = tuple(np.asarray(mesh0).shape) if not np.iscomplexobj(mesh0) else None
    mesh_shape = np.array(real_shape or mesh_shape or o.ch2rshape(np.asarray(mesh0).shape))
    kcell = o.rfftk(tuple(int(s) for s in mesh_shape))
    d0 = spec(mesh0) / o.rectangular_hat(kcell, order=deconv[0])
    if mesh1 is None:
        mmk = d0.real ** 2 + d0.imag ** 2
    else:
        d1 = spec(mesh1) / o.rectangular_hat(kcell, order=deconv[1])
        mmk = d0 * d1.conj()

    box_size = mesh_shape.astype(np.float64) if box_size is None else np.asarray(box_size, dtype=np.float64)
    kedges, kmesh, mumesh, rfftw = waves(mesh_shape, box_size, kedges, include_corners, los)
    n_bins = len(kedges) + 1
    dig = np.digitize(kmesh.reshape(-1), kedges)
    kcount = np.bincount(dig, weights=rfftw.reshape(-1), minlength=n_bins)[1:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        kmean = np.bincount(dig, weights=(kmesh * rfftw).reshape(-1), minlength=n_bins)[1:-1] / kcount
        norm = (box_size / mesh_shape ** 2).prod()
        pow, pabs = {}, {}
        for ell in np.atleast_1d(ells):
            ell = int(ell)
            wts = (mmk * (2 * ell + 1) * legendre(ell)(mumesh) * rfftw).reshape(-1)
            if mesh1 is None:
                p = np.bincount(dig, weights=wts, minlength=n_bins)[1:-1]
            else:
                pr = np.bincount(dig, weights=wts.real, minlength=n_bins)[1:-1]
                pi = np.bincount(dig, weights=wts.imag, minlength=n_bins)[1:-1]
                p = (pr ** 2 + pi ** 2) ** .5
            pa = np.bincount(dig, weights=np.abs(wts), minlength=n_bins)[1:-1]
            pow[ell] = p * (norm / kcount)
            pabs[ell] = pa * (norm / kcount)
    if isinstance(ells, int):
        return kcount, kmean, pow[ells], pabs[ells]
    return kcount, kmean, pow, pabs
