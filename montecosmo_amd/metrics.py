"""Binned power spectra, transfer functions and coherences of meshes (montecosmo/metrics.py:60-210) on the HIP path.

    kmean, pow = metrics.spectrum(mesh, box_size=box, ells=[0, 2, 4], box_center=(0, 0, 2000.))
    ks, pow1, trans, coh = metrics.powtranscoh(truth, posterior_meshes, box_size=box)    # leading batch axis on every output

Inputs are real meshes or complex64 half-spectra (numpy arrays or torch tensors); real meshes go through the batched
`mcpm_fft_r2c`.  The edges, the per-axis |k| tables and the deconvolution factors are worked out on the host in float64 as
the reference's `_waves` / `rfftk` / `rectangular_hat` do; `mcpm_spectrum_bins_c64` (csrc/spectrum.hip) makes every bin sum
in one pass over the spectra (both autos and the cross spectrum of `powtranscoh` together), bitwise reproducibly.  A leading
batch axis on `mesh1` (and on `mesh0` for `spectrum`) replaces the reference's `nvmap` over chains; batches go to the
device in chunks of bounded memory.  Outputs are float64 numpy arrays; empty bins are NaN, as 0/0 is in the reference.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import nbody, _lib
from .utils import safe_div, ch2rshape

MAX_EDGES = 4096               # MCPM_SPECTRUM_MAX_EDGES
CHUNK_BYTES = 1 << 32          # device memory a batch chunk may take (spectra, real staging, workspace)

__all__ = ["spectrum", "transfer", "coherence", "powtranscoh", "MAX_EDGES"]


# ------------------------------------------------------------------------------------------------
# host side: shapes, edges, tables
def _mesh_shape(t, real):
    """Real mesh shape of one (unbatched) input of shape t."""
    if len(t) != 3:
        raise ValueError(f"only 3D meshes (with an optional leading batch axis) are supported, got shape {tuple(t)}")
    shape = tuple(int(s) for s in t) if real else ch2rshape(t)
    if shape[-1] % 2:
        raise ValueError(f"the last axis of the mesh must be even, got mesh shape {shape}")
    return shape


def _kedges(mesh_shape, box_size, kedges=None, include_corners=True):
    """Bin edges of montecosmo/metrics.py:_waves (:60-110): None, an int (number of edges), a float (dk) or a list."""
    mesh_shape = np.asarray(mesh_shape)
    box_size = np.asarray(box_size, dtype=np.float64)
    if isinstance(kedges, (type(None), int, float)):
        dim = len(mesh_shape)
        kmin = 0.
        kmax = np.pi * (mesh_shape / box_size).min()
        if include_corners:      # the largest |k| of the half-spectrum: every axis at its largest |k_i|, summed as _waves does
            kvec = nbody.rfftk(tuple(mesh_shape), box_size)
            kmax = np.sqrt(sum(np.max(ki ** 2) for ki in kvec))
        if kedges is None:
            dk = dim ** .5 * 2 * np.pi / box_size.min()
            n_kedges = max(int((kmax - kmin) / dk), 1)
        elif isinstance(kedges, int):
            n_kedges = kedges
        else:
            n_kedges = max(int((kmax - kmin) / kedges), 1)
        dk = (kmax - kmin) / n_kedges
        kedges = np.linspace(kmin, kmax, n_kedges, endpoint=False)
        kedges += dk / 2
    kedges = np.asarray(kedges, dtype=np.float64).reshape(-1)
    if len(kedges) > MAX_EDGES:
        raise ValueError(f"at most {MAX_EDGES} bin edges, got {len(kedges)}")
    if not np.all(np.isfinite(kedges)) or not np.all(np.diff(kedges) > 0):
        raise ValueError("bin edges must be finite and strictly increasing")
    return kedges


def _ktable(mesh_shape, box_size):
    """[kx | ky | kz] of rfftk(mesh_shape, box_size), float64."""
    return np.concatenate([k.reshape(-1) for k in nbody.rfftk(mesh_shape, box_size)]).astype(np.float64)


def _deconv_table(mesh_shape, order):
    """Per-axis factors 1 / sinc(k_cell / 2 pi)^order, [x | y | z]; None for order 0."""
    if order == 0:
        return None
    return np.concatenate([1. / np.sinc(k.reshape(-1) / (2 * np.pi)) ** order for k in nbody.rfftk(mesh_shape)])


def _norm_args(box_size, box_center, mesh_shape):
    box_size = np.asarray(mesh_shape, dtype=np.float64) if box_size is None else np.asarray(box_size, dtype=np.float64)
    box_center = np.asarray(box_center, dtype=np.float64)
    los = safe_div(box_center, np.linalg.norm(box_center)).astype(np.float64)
    return box_size, los


# ------------------------------------------------------------------------------------------------
# device side
def _prepare(mesh):
    """-> (tensor [B, ...] on the device, real input?, batched?, mesh shape)."""
    t = torch.as_tensor(mesh)
    real = not t.is_complex()
    if t.ndim not in (3, 4):
        raise ValueError(f"only 3D meshes (with an optional leading batch axis) are supported, got shape {tuple(t.shape)}")
    batched = t.ndim == 4
    shape = _mesh_shape(t.shape[1:] if batched else t.shape, real)
    return (t if batched else t[None]), real, batched, shape


def _to_spec(t, real, shape, dev):
    """complex64 half-spectra [b, nx, ny, nz/2+1] on the device for the rows of t."""
    if not real:
        return t.to(device=dev, dtype=torch.complex64).contiguous()
    x = t.to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty((x.shape[0],) + tuple(nbody.r2chshape(shape)), dtype=torch.complex64, device=dev)
    nbody.get_plan(shape).call("mcpm_fft_r2c", x, out, int(x.shape[0]))
    return out


def _f64p(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _bin_sums(mesh0, mesh1, box_size, box_center, ells, kedges, include_corners, deconv):
    """Raw bin sums: (kedges, B or None, sums [B, n_acc, n_bins], mesh_shape, box_size); see include/mcpm.h for n_acc."""
    t0, real0, bat0, shape = _prepare(mesh0)
    two = mesh1 is not None
    if two:
        t1, real1, bat1, shape1 = _prepare(mesh1)
        if shape1 != shape:
            raise ValueError(f"mesh shapes differ: {shape} and {shape1}")
        if bat0 and bat1 and t0.shape[0] != t1.shape[0]:
            raise ValueError(f"batch sizes differ: {t0.shape[0]} and {t1.shape[0]}")
    else:
        t1, real1, bat1 = None, False, False
    batch = max(t0.shape[0], t1.shape[0] if two else 1)
    batched = bat0 or bat1
    if isinstance(deconv, int):
        deconv = (deconv, deconv)
    ell_list = [int(l) for l in np.atleast_1d(ells)]
    if not ell_list or min(ell_list) < 0 or max(ell_list) > 8 or len(ell_list) > 9:
        raise ValueError("multipoles must be 1 .. 9 integers in 0 .. 8")
    box_size, los = _norm_args(box_size, box_center, shape)
    edges = _kedges(shape, box_size, kedges, include_corners)
    ktab = _ktable(shape, box_size)
    dc0 = _deconv_table(shape, deconv[0])
    dc1 = _deconv_table(shape, deconv[1]) if two else None

    dev = nbody._device()
    nx, ny, nz = shape
    n_ells, n_bins = len(ell_list), len(edges) - 1
    n_acc = 2 + n_ells * (4 if two else 1)
    out = np.zeros((batch, n_acc, max(n_bins, 0)), dtype=np.float64)
    if n_bins < 1:      # fewer than two edges: no bin, as in the reference
        return edges, batched, out, np.asarray(shape), box_size, ell_list, two
    ws1 = C.c_int64()
    _lib.call("mcpm_spectrum_workspace", nx, ny, nz, len(edges), n_ells, int(two), 1, C.byref(ws1))
    mh = nx * ny * (nz // 2 + 1)
    per_row = ws1.value + (16 * mh if two else 8 * mh) + 8 * nx * ny * nz
    chunk = int(max(1, min(batch, CHUNK_BYTES // per_row)))
    ells_c = (C.c_int * n_ells)(*ell_list)
    los_c = np.ascontiguousarray(los, dtype=np.float64)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    s0_fixed = None if bat0 else _to_spec(t0, real0, shape, dev)
    s1_fixed = None if (not two or bat1) else _to_spec(t1, real1, shape, dev)
    for lo in range(0, batch, chunk):
        hi = min(lo + chunk, batch)
        s0 = _to_spec(t0[lo:hi], real0, shape, dev) if bat0 else s0_fixed
        s1 = (_to_spec(t1[lo:hi], real1, shape, dev) if bat1 else s1_fixed) if two else None
        ws = C.c_int64()
        _lib.call("mcpm_spectrum_workspace", nx, ny, nz, len(edges), n_ells, int(two), hi - lo, C.byref(ws))
        work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
        res = torch.empty((hi - lo, n_acc, n_bins), dtype=torch.float64, device=dev)
        _lib.call("mcpm_spectrum_bins_c64", stream, nx, ny, nz, s0, mh if bat0 else 0, s1, mh if bat1 else 0, hi - lo, ktab, dc0, dc1, edges,
                  len(edges), los_c, ells_c, n_ells, work, ws.value, res)
        out[lo:hi] = res.cpu().numpy()
    return edges, batched, out, np.asarray(shape), box_size, ell_list, two


def _finish(sums, batched, shape, box_size, ell_list, ells, two, which):
    """Bin sums -> (kcount, kmean, pow) of `which` ('cross', 'auto0', 'auto1')."""
    norm = (box_size / shape ** 2).prod()
    kcount = sums[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        kmean = sums[:, 1] / kcount
        pow = {}
        for j, ell in enumerate(ell_list):
            if not two:
                p = sums[:, 2 + j]
            elif which == "cross":
                p = (sums[:, 4 + 4 * j] ** 2 + sums[:, 5 + 4 * j] ** 2) ** .5
            else:
                p = sums[:, 2 + 4 * j + (which == "auto1")]
            pow[ell] = p * (norm / kcount)
    if not batched:
        kcount, kmean, pow = kcount[0], kmean[0], {l: p[0] for l, p in pow.items()}
    if isinstance(ells, (int, np.integer)):
        return kcount, kmean, pow[int(ells)]
    return kcount, kmean, pow


# ------------------------------------------------------------------------------------------------
# public interface (montecosmo/metrics.py:113-210)
def _spectrum(mesh0, mesh1=None, box_size=None, box_center: tuple = (0., 0., 0.), ells: int | list = 0,
              kedges: int | float | list = None, include_corners=True, deconv: int | tuple = (0, 0)):
    """Auto (mesh1 None) or cross spectrum multipoles: (kcount, kmean, pow); pow is an array for an int `ells`, else {ell: array}.
    The cross spectrum is the modulus of the complex bin sum."""
    _, batched, sums, shape, box_size, ell_list, two = _bin_sums(mesh0, mesh1, box_size, box_center, ells, kedges,
                                                                 include_corners, deconv)
    return _finish(sums, batched, shape, box_size, ell_list, ells, two, "cross")


def spectrum(mesh0, mesh1=None, box_size=None, box_center: tuple = (0., 0., 0.), ells: int | list = 0,
             kedges: int | float | list = None, include_corners=True):
    kcount, kmean, pow = _spectrum(mesh0, mesh1, box_size, box_center, ells, kedges, include_corners)
    return kmean, pow


def _pow3(mesh0, mesh1, box_size, kedges, include_corners):
    """(kmean, pow0, pow1, pow01) of the two meshes from one pass."""
    _, batched, sums, shape, box_size, ell_list, two = _bin_sums(mesh0, mesh1, box_size, (0., 0., 0.), 0, kedges,
                                                                 include_corners, (0, 0))
    out = [_finish(sums, batched, shape, box_size, ell_list, 0, two, w) for w in ("auto0", "auto1", "cross")]
    return out[0][1], out[0][2], out[1][2], out[2][2]


def transfer(mesh0, mesh1, box_size, kedges: int | float | list = None, include_corners=True):
    ks, pow0, pow1, _ = _pow3(mesh0, mesh1, box_size, kedges, include_corners)
    return ks, (pow1 / pow0) ** .5


def coherence(mesh0, mesh1, box_size, kedges: int | float | list = None, include_corners=True):
    ks, pow0, pow1, pow01 = _pow3(mesh0, mesh1, box_size, kedges, include_corners)
    return ks, pow01 / (pow0 * pow1) ** .5


def powtranscoh(mesh0, mesh1, box_size, kedges: int | float | list = None, include_corners=True):
    """(k, pow1, (pow1 / pow0)^.5, pow01 / (pow0 pow1)^.5) from one pass over both meshes."""
    ks, pow0, pow1, pow01 = _pow3(mesh0, mesh1, box_size, kedges, include_corners)
    return ks, pow1, (pow1 / pow0) ** .5, pow01 / (pow0 * pow1) ** .5
