"""Binned power spectra, transfer functions and coherences of meshes (montecosmo/metrics.py:60-210) on the HIP path.

    kmean, pow = metrics.spectrum(mesh, box_size=box, ells=[0, 2, 4], box_center=(0, 0, 2000.))
    ks, pow1, trans, coh = metrics.powtranscoh(truth, posterior_meshes, box_size=box)    # leading batch axis on every output

Inputs are real meshes or complex64 half-spectra (numpy arrays or torch tensors); real meshes go through the batched
`mcpm_fft_r2c`.  The edges, the per-axis |k| tables and the deconvolution factors are worked out on the host in float64 as
the reference's `_waves` / `rfftk` / `rectangular_hat` do; `mcpm_spectrum_bins_c64` (csrc/spectrum.hip) makes every bin sum
in one pass over the spectra (both autos and the cross spectrum of `powtranscoh` together), bitwise reproducibly.  A leading
batch axis on `mesh1` (and on `mesh0` for `spectrum`) replaces the reference's `nvmap` over chains; batches go to the
device in chunks of bounded memory.  Outputs are float64 numpy arrays; empty bins are NaN, as 0/0 is in the reference.

    tri, kmean, ntri, bk = metrics.bispectrum(mesh, box_size=box)      # every closed triangle of the default bins

is the first statistic beyond the power spectrum (the reference lists 'bispec' as still to do): the FFT estimator, one shell field per
k bin (`mcpm_bispectrum_split_c64`, the batched `mcpm_fft_c2r`) and one sum over cells per triangle of bins (`mcpm_bispectrum_sums_f32`,
csrc/bispectrum.hip), bitwise reproducibly, with the same bins and the same batch axis as `spectrum`.

The real-space half of the module (montecosmo/metrics.py:214-313, :545-553) bins cells by a per-cell value instead of |k|:

    rcount, rmean, mse = metrics.mse_radius(truth, posterior_meshes, rmesh, cell_length)      # by distance, default shells
    vcount, vmean, mse = metrics.mse_value(truth, posterior_meshes, cell_length, vedges=50)  # by density, 50 quantile bins

`mcpm_binned_sums_f32` (csrc/binned.hip) makes the count, the sum of the binning values and the sum of the target of every batch row
in one pass, bitwise reproducibly; the squared error is formed inside the pass.  Every comparison with an edge is made in float64
(the reference compares float32 jax arrays with edges found from them), targets are read as float32, and a leading batch axis on the
target (`mesh1`, `mesh`, `targets`) gives `taggr` a leading axis.  `aggr_fn` other than the mean is a slow host path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import nbody, _lib
from .chains import multi_ess, multi_gr, harmean, geomean      # the chain metrics of montecosmo/metrics.py:562-579 (chains.py)
from .utils import safe_div, ch2rshape

MAX_EDGES = 4096               # MCPM_SPECTRUM_MAX_EDGES
CHUNK_BYTES = 1 << 32          # device memory a batch chunk may take (spectra, real staging, workspace)
MAX_BISPEC_BINS = 32           # MCPM_BISPECTRUM_MAX_BINS
MAX_TRIANGLES = 8192           # MCPM_BISPECTRUM_MAX_TRIANGLES

__all__ = ["spectrum", "transfer", "coherence", "powtranscoh", "bispectrum", "bin_and_aggregate", "mse_radius", "mse_value", "mse_wave",
           "distr_radial", "multi_ess", "multi_gr", "harmean", "geomean", "MAX_EDGES", "MAX_BISPEC_BINS", "MAX_TRIANGLES"]


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


def _centred_edges(spec, lo, hi, check=None):
    """n edges at the centres of n equal cells of [lo, hi): n = spec for an int, as many cells of width spec as fit (at least one) for a
    float.  check(n), if given, may refuse the count before the edges are made."""
    n = int(spec) if isinstance(spec, (int, np.integer)) else max(int((hi - lo) / float(spec)), 1)
    if check is not None:
        check(n)
    d = (hi - lo) / n
    edges = np.linspace(lo, hi, n, endpoint=False)
    edges += d / 2
    return edges


def _valid_edges(edges, max_count, strict, min_count=0):
    """The final checks of every list of edges -> float64 [n]: at most max_count of them (and, for a caller that cannot do with fewer, at
    least min_count), finite, strictly increasing (`strict`) or non-decreasing."""
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    if min_count and not min_count <= len(edges) <= max_count:
        raise ValueError(f"{min_count - 1} .. {max_count - 1} bins ({min_count} .. {max_count} edges), got {len(edges)} edges")
    if len(edges) > max_count:
        raise ValueError(f"at most {max_count} bin edges, got {len(edges)}")
    steps = np.diff(edges)
    if not np.all(np.isfinite(edges)) or not np.all(steps > 0 if strict else steps >= 0):
        raise ValueError("bin edges must be finite and " + ("strictly increasing" if strict else "non-decreasing"))
    return edges


def _kedges(mesh_shape, box_size, kedges=None, include_corners=True):
    """Bin edges of montecosmo/metrics.py:_waves (:60-110): None, an int (number of edges), a float (dk) or a list."""
    mesh_shape = np.asarray(mesh_shape)
    box_size = np.asarray(box_size, dtype=np.float64)
    if isinstance(kedges, (type(None), int, float)):
        kmax = np.pi * (mesh_shape / box_size).min()
        if include_corners:      # the largest |k| of the half-spectrum: every axis at its largest |k_i|, summed as _waves does
            kvec = nbody.rfftk(tuple(mesh_shape), box_size)
            kmax = np.sqrt(sum(np.max(ki ** 2) for ki in kvec))
        if kedges is None:
            kedges = len(mesh_shape) ** .5 * 2 * np.pi / box_size.min()
        kedges = _centred_edges(kedges, 0., kmax)
    return _valid_edges(kedges, MAX_EDGES, True)


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


def _batch_chunks(dev, batch, row_bytes, res_shape, ws_fn, *ws_args):
    """The batch in chunks of bounded memory: yields (lo, hi, work, work_bytes, res) with rows lo .. hi-1 of the batch, the workspace
    `ws_fn(*ws_args, hi - lo)` asks for and a float64 result of shape res_shape(hi - lo), both fresh on the device.  A row takes row_bytes
    besides its workspace; a chunk stays under CHUNK_BYTES (or is one row).  The one-row query is made at once, the rest as the loop runs."""
    def ws_bytes(b):
        ws = C.c_int64()
        _lib.call(ws_fn, *ws_args, b, C.byref(ws))
        return ws.value

    chunk = int(max(1, min(batch, CHUNK_BYTES // (ws_bytes(1) + row_bytes))))

    def chunks():
        for lo in range(0, batch, chunk):
            hi = min(lo + chunk, batch)
            ws = ws_bytes(hi - lo)
            yield (lo, hi, torch.empty(ws, dtype=torch.uint8, device=dev), ws,
                   torch.empty(res_shape(hi - lo), dtype=torch.float64, device=dev))
    return chunks()


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
    mh = nx * ny * (nz // 2 + 1)
    chunks = _batch_chunks(dev, batch, (16 * mh if two else 8 * mh) + 8 * nx * ny * nz, lambda b: (b, n_acc, n_bins),
                           "mcpm_spectrum_workspace", nx, ny, nz, len(edges), n_ells, int(two))
    ells_c = (C.c_int * n_ells)(*ell_list)
    los_c = np.ascontiguousarray(los, dtype=np.float64)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    s0_fixed = None if bat0 else _to_spec(t0, real0, shape, dev)
    s1_fixed = None if (not two or bat1) else _to_spec(t1, real1, shape, dev)
    for lo, hi, work, ws, res in chunks:
        s0 = _to_spec(t0[lo:hi], real0, shape, dev) if bat0 else s0_fixed
        s1 = (_to_spec(t1[lo:hi], real1, shape, dev) if bat1 else s1_fixed) if two else None
        _lib.call("mcpm_spectrum_bins_c64", stream, nx, ny, nz, s0, mh if bat0 else 0, s1, mh if bat1 else 0, hi - lo, ktab, dc0, dc1, edges,
                  len(edges), los_c, ells_c, n_ells, work, ws, res)
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


# ------------------------------------------------------------------------------------------------
# binned bispectrum (not in the reference: montecosmo/model.py:60 lists 'bispec' as the observable still to do)
def _bispec_edges(mesh_shape, box_size, kedges=None):
    """Bin edges of `bispectrum`: None, an int, a float or a list, read as `_kedges` reads them, except that the int / float / None
    cases stop at kmax = (2/3) pi min(mesh_shape / box_size), below which no aliased triangle closes, and that None spaces the edges
    by three fundamentals, 3 * 2 pi / min(box_size)."""
    mesh_shape = np.asarray(mesh_shape)
    box_size = np.asarray(box_size, dtype=np.float64)
    if isinstance(kedges, (bool, np.bool_)):
        raise ValueError("edges must be None, an int, a float or a list")
    if isinstance(kedges, (type(None), int, float, np.integer, np.floating)):
        def check(n):
            if not 2 <= n <= MAX_BISPEC_BINS + 1:
                raise ValueError(f"1 .. {MAX_BISPEC_BINS} bins (2 .. {MAX_BISPEC_BINS + 1} edges), got {n} edges: pass kedges")

        kmax = 2. / 3. * np.pi * (mesh_shape / box_size).min()
        kedges = _centred_edges(3 * 2 * np.pi / box_size.min() if kedges is None else kedges, 0., kmax, check)
    return _valid_edges(kedges, MAX_BISPEC_BINS + 1, True, min_count=2)


def _bispec_triangles(edges, triangles=None):
    """(T, 3) int64 bin triples in the caller's row order.  None: every i <= j <= l with edges[l] < edges[i+1] + edges[j+1], the bins
    between which a closed triangle k1 + k2 + k3 = 0 can exist."""
    n_bins = len(edges) - 1
    if triangles is None:
        tri = np.array([(i, j, l) for i in range(n_bins) for j in range(i, n_bins) for l in range(j, n_bins)
                        if edges[l] < edges[i + 1] + edges[j + 1]], dtype=np.int64).reshape(-1, 3)
    else:
        tri = np.asarray(triangles)
        if tri.ndim != 2 or tri.shape[1] != 3 or not np.issubdtype(tri.dtype, np.integer):
            raise ValueError(f"triangles must be an integer array of shape (T, 3), got {tri.dtype} {tri.shape}")
        tri = tri.astype(np.int64)
    if not 1 <= len(tri) <= MAX_TRIANGLES:
        raise ValueError(f"1 .. {MAX_TRIANGLES} triangles, got {len(tri)}")
    if tri.min() < 0 or tri.max() >= n_bins:
        raise ValueError(f"triangle bin indices must be in 0 .. {n_bins - 1}")
    return tri


def _bispec_spec(t, real, shape, dev):
    """_to_spec, one row per transform, so that a row's spectrum has the bits of its single call whatever the batch; a real view that does
    not start on a 16-byte boundary is copied first (the transforms load vectors)."""
    if not real:
        return _to_spec(t, real, shape, dev)
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    out = torch.empty((t.shape[0],) + tuple(nbody.r2chshape(shape)), dtype=torch.complex64, device=dev)
    plan = nbody.get_plan(shape)
    for r in range(t.shape[0]):
        plan.call("mcpm_fft_r2c", t[r], out[r], 1)
    return out


def _shell_spectra(rows, real, shape, dev, ktab, dc, edges):
    """complex64 [b, n_bins, nx, ny, nz/2+1]: the (deconvolved) half-spectrum of every row of `rows` (None: the unit spectrum, one row)
    split by k bin, zero outside the bin."""
    nx, ny, nz = shape
    n_bins, mh = len(edges) - 1, nx * ny * (nz // 2 + 1)
    spec = None if rows is None else _bispec_spec(rows, real, shape, dev)
    b = 1 if spec is None else int(spec.shape[0])
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    shells = torch.empty((b, n_bins, nx, ny, nz // 2 + 1), dtype=torch.complex64, device=dev)
    _lib.call("mcpm_bispectrum_split_c64", stream, nx, ny, nz, spec, mh if spec is not None else 0, b, ktab, dc, edges, len(edges), shells)
    return shells


def _shell_fields(rows, real, shape, dev, ktab, dc, edges):
    """float32 [b, n_bins, nx, ny, nz]: F_bin(x) of every row of `rows` (None: I_bin(x), of the unit spectrum, one row): the shell
    split and, per row, one unnormalised C2R of its n_bins spectra (the same transform whatever the batch: a row keeps its bits)."""
    shells = _shell_spectra(rows, real, shape, dev, ktab, dc, edges)
    fields = torch.empty(tuple(shells.shape[:2]) + tuple(shape), dtype=torch.float32, device=dev)
    plan = nbody.get_plan(shape)
    for r in range(shells.shape[0]):
        plan.call("mcpm_fft_c2r", shells[r], fields[r], int(shells.shape[1]))
    return fields


def _triple_sums(t, real, shape, ktab, dc, edges, tri_sorted):
    """float64 [B, T]: sum over cells of F_i F_j F_l for every row of t (None: of I_i I_j I_l, one row), in chunks of bounded memory."""
    dev = nbody._device()
    nx, ny, nz = shape
    n_bins, n_tri, m, mh = len(edges) - 1, len(tri_sorted), nx * ny * nz, nx * ny * (nz // 2 + 1)
    batch = 1 if t is None else int(t.shape[0])
    chunks = _batch_chunks(dev, batch, (n_bins + 1) * (8 * mh + 4 * m), lambda b: (b, n_tri),
                           "mcpm_bispectrum_workspace", nx, ny, nz, n_bins, n_tri)
    tri_dev = torch.from_numpy(np.ascontiguousarray(tri_sorted, dtype=np.int32)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = np.zeros((batch, n_tri), dtype=np.float64)
    for lo, hi, work, ws, res in chunks:
        fields = _shell_fields(None if t is None else t[lo:hi], real, shape, dev, ktab, dc, edges)
        _lib.call("mcpm_bispectrum_sums_f32", stream, fields, m, n_bins, hi - lo, tri_dev, n_tri, work, ws, res)
        out[lo:hi] = res.cpu().numpy()
    return out


_NTRI_CACHE = {}      # (mesh_shape, box_size, edges, sorted triangles) -> ntri; the few most recent geometries
_NTRI_CACHE_SIZE = 8


def bispectrum(mesh, box_size=None, kedges: int | float | list = None, triangles=None, deconv: int = 0, reduced=False):
    """Binned bispectrum of a mesh, the FFT (Scoccimarro) estimator: (tri, kmean, ntri, bk), with qk appended when `reduced`.

    With d = rfftn(mesh) (unnormalised, divided by the paint window of order `deconv`), bins kedges[b] <= |k| < kedges[b+1] as in
    `spectrum`, F_b(x) = sum_{k in bin b} d(k) e^{ikx} and I_b the same with d = 1, a triangle of bins (i, j, l) has
    S = sum_x F_i F_j F_l, ntri = sum_x I_i I_j I_l / M and bk = (V^2 / M^3) (S / M) / ntri (M cells, V = prod box_size).  ntri counts the
    ordered mode triples k1 + k2 + k3 = 0 with k1 in i, k2 in j, k3 in l, where the sum closes MODULO THE MESH: the default edges stop
    at 2/3 of the Nyquist wavenumber, below which no aliased triple closes; edges given by the caller may go further, and triangles that
    reach past 2/3 Nyquist then count aliased triples as well.  ntri is measured through the same float32 transforms as S, so it is an
    integer to about 1e-6 of sum_x |I_i I_j I_l| / M only; a triangle whose bins hold no mode has ntri = 0 exactly and bk = NaN.

    mesh: a real mesh or a complex64 half-spectrum (Hermitian, as rfftn of a real mesh is), numpy or torch, with an optional leading
    batch axis, which `bk` and `qk` then carry.  kedges: see `_bispec_edges`; at most MAX_BISPEC_BINS bins.  triangles: None (every
    i <= j <= l that can close) or an integer array (T, 3) of bin indices in any order, repeats allowed, T <= MAX_TRIANGLES; outputs
    follow its row order, and the order inside a row does not change a bit of the result.  tri (T, 3), kmean (n_bins,), ntri (T,),
    bk ([B,] T), qk = bk / (P_i P_j + P_j P_l + P_l P_i) with P the binned power of the same mesh: float64 numpy arrays."""
    t, real, batched, shape = _prepare(mesh)
    box_size = np.asarray(shape, dtype=np.float64) if box_size is None else np.asarray(box_size, dtype=np.float64)
    edges = _bispec_edges(shape, box_size, kedges)
    tri = _bispec_triangles(edges, triangles)
    if not isinstance(deconv, (int, np.integer)) or deconv < 0:
        raise ValueError(f"deconv must be a non-negative int, got {deconv!r}")
    tri_sorted = np.sort(tri, axis=1)
    ktab = _ktable(shape, box_size)
    dc = _deconv_table(shape, int(deconv))
    m, vol = float(np.prod(shape)), float(box_size.prod())

    key = (shape, box_size.tobytes(), edges.tobytes(), tri_sorted.tobytes())
    ntri = _NTRI_CACHE.get(key)
    if ntri is None:
        ntri = _triple_sums(None, False, shape, ktab, None, edges, tri_sorted)[0] / m
        while len(_NTRI_CACHE) >= _NTRI_CACHE_SIZE:
            _NTRI_CACHE.pop(next(iter(_NTRI_CACHE)))
        _NTRI_CACHE[key] = ntri
    sums = _triple_sums(t, real, shape, ktab, dc, edges, tri_sorted)
    with np.errstate(divide="ignore", invalid="ignore"):
        bk = (vol ** 2 / m ** 3) * (sums / m) / ntri
    _, kmean, pk = _spectrum(t if reduced else t[:1], box_size=box_size, kedges=edges, deconv=int(deconv))
    out = (tri, kmean[0], ntri.copy(), bk if batched else bk[0])
    if reduced:
        pi, pj, pl = (pk[:, tri[:, a]] for a in range(3))
        with np.errstate(divide="ignore", invalid="ignore"):
            qk = bk / (pi * pj + pj * pl + pl * pi)
        out += (qk if batched else qk[0],)
    return out


# ------------------------------------------------------------------------------------------------
# real-space bins (montecosmo/metrics.py:214-313, :545-553): host side
def _check_edges(edges):
    return _valid_edges(edges, MAX_EDGES, False)


def _quantiles(values, q):
    """np.quantile(values.astype(float64), q) (method 'linear'), bit for bit, for a tensor of any size on any device: one sort where
    the values are, a gather of the two order statistics per level, numpy's interpolation on the host in float64."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if not np.all((q >= 0) & (q <= 1)):      # (a NaN level fails too)
        raise ValueError("quantile levels must be in [0, 1]")
    s = torch.sort(torch.as_tensor(values).reshape(-1)).values
    n = s.numel()
    pos = (n - 1) * q
    lo = np.floor(pos)
    t = pos - lo
    lo = lo.astype(np.int64)
    idx = torch.from_numpy(np.concatenate([lo, np.minimum(lo + 1, n - 1)])).to(s.device)
    ab = s[idx].to(torch.float64).cpu().numpy()
    a, b = ab[:len(q)], ab[len(q):]
    d = b - a
    return np.where(t < .5, a + d * t, b - d * (1 - t))


def _vedges(values, vedges, min_count=1, cell_length=None):
    """-> (edges, min_count) of bin_and_aggregate (montecosmo/metrics.py:223-235): a list is used as given, an int is a number of edges,
    a float a bin width, None the width sqrt(3) cell_length that keeps radial shells connected; the int and float cases put the edges
    at the centres of equal cells of [vmin, vmax], the range of `values` (a tensor, where it lives), or of [0, 1] when min_count is
    None.  With min_count None the edges are quantile levels: they become the quantiles of `values`, and min_count becomes 1.
    Unlike _kedges, repeated edges pass (quantiles of tied data repeat); decreasing or non-finite ones raise ValueError."""
    if vedges is None:
        if cell_length is None:
            raise ValueError("edges None need a cell_length")
        vedges = 3 ** .5 * float(cell_length)
    if isinstance(vedges, (bool, np.bool_)):
        raise ValueError("edges must be a list, an int or a float")
    if isinstance(vedges, (int, np.integer, float, np.floating)):
        is_int = isinstance(vedges, (int, np.integer))
        if is_int and not 1 <= vedges <= MAX_EDGES:      # known before the values are looked at
            raise ValueError(f"1 .. {MAX_EDGES} bin edges, got {vedges}")
        if min_count is None:
            vmin, vmax = 0., 1.
        else:
            vmin, vmax = float(values.min()), float(values.max())

        def check(n):
            if n > MAX_EDGES:
                raise ValueError(f"at most {MAX_EDGES} bin edges, got {n}")

        vedges = _centred_edges(vedges, vmin, vmax, check)
    vedges = np.asarray(vedges, dtype=np.float64).reshape(-1)
    if min_count is None:
        if len(vedges) > MAX_EDGES:
            raise ValueError(f"at most {MAX_EDGES} bin edges, got {len(vedges)}")
        vedges = _quantiles(values, vedges)
        min_count = 1
    return _check_edges(vedges), min_count


def _batch_of(target, values, what):
    """None when `target` has the cells of `values`, B when it carries one more leading axis of length B; ValueError otherwise."""
    if tuple(target.shape) == tuple(values.shape):
        return None
    if target.ndim == values.ndim + 1 and tuple(target.shape[1:]) == tuple(values.shape):
        return int(target.shape[0])
    if target.numel() == values.numel():      # the reference flattens both
        return None
    if values.ndim == target.ndim + 1 and tuple(values.shape[1:]) == tuple(target.shape):
        raise ValueError(f"the binning values may not be batched (shape {tuple(values.shape)} against {what} of shape {tuple(target.shape)}): "
                         "the count filter would make the result ragged")
    raise ValueError(f"{what} of shape {tuple(target.shape)} does not match binning values of shape {tuple(values.shape)}")


def _finish_bins(vcount, vsum, tsum, min_count, batched):
    keep = vcount >= min_count
    vcount = vcount[keep]
    with np.errstate(divide="ignore", invalid="ignore"):
        vmean = vsum[keep] / vcount
        taggr = tsum[:, keep] / vcount
    return vcount, vmean, (taggr if batched else taggr[0])


def _binned_host(values, t0, t1, scale, vedges, min_count, aggr_fn, mask, cell_length):
    """The slow path of an `aggr_fn` other than the mean (a median, say): everything on the host in float64, one bin at a time."""
    to64 = lambda x: torch.as_tensor(x).detach().cpu().numpy().astype(np.float64).reshape(-1)
    v, tg = to64(values), to64(t0)
    if t1 is not None:
        tg = (tg - to64(t1)) ** 2 * scale
    if mask is not None:
        m = torch.as_tensor(mask).cpu().numpy().astype(bool).reshape(-1)
        v, tg = v[m], tg[m]
    edges, min_count = _vedges(torch.from_numpy(v), vedges, min_count, cell_length)
    n_bins = len(edges) + 1
    dig = np.digitize(v, edges)
    vcount = np.bincount(dig, minlength=n_bins)[1:-1].astype(np.float64)
    vsum = np.bincount(dig, weights=v, minlength=n_bins)[1:-1]
    keep = vcount >= min_count
    taggr = np.array([aggr_fn(tg[dig == i]) for i in range(1, n_bins - 1)], dtype=np.float64).reshape(n_bins - 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return vcount[keep], vsum[keep] / vcount[keep], taggr[keep]


# ------------------------------------------------------------------------------------------------
# real-space bins: device side
def _binned(values, t0, t1, scale, vedges, min_count, aggr_fn=None, mask=None, cell_length=None):
    """(vcount, vmean, taggr): cells binned by `values`; the target is t0 (t1 None) or (t0 - t1)^2 scale.  The batched input, if any,
    is t1 in the squared-error mode and t0 in the plain mode.  Every argument check comes before the first device call."""
    v, a0 = torch.as_tensor(values), torch.as_tensor(t0)
    a1 = None if t1 is None else torch.as_tensor(t1)
    if a1 is None:
        batch = _batch_of(a0, v, "targets")
    else:
        if a0.numel() != v.numel():
            _batch_of(a0, v, "mesh0")      # raises with the reason
            raise ValueError(f"mesh0 of shape {tuple(a0.shape)} may not be batched against binning values of shape {tuple(v.shape)}")
        batch = _batch_of(a1, a0, "mesh1")
    n = v.numel()
    if n < 1:
        raise ValueError("no cells to bin")
    if mask is not None:
        mask = torch.as_tensor(mask)
        if mask.numel() != n:
            raise ValueError(f"mask of shape {tuple(mask.shape)} does not match binning values of shape {tuple(v.shape)}")
    if aggr_fn is not None:
        if batch is not None:
            raise ValueError("aggr_fn is applied on the host to one target at a time: pass unbatched targets")
        return _binned_host(v, a0, a1, scale, vedges, min_count, aggr_fn, mask, cell_length)
    if not isinstance(vedges, (type(None), int, float, np.integer, np.floating)) and min_count is not None:
        vedges = _check_edges(vedges)
    elif isinstance(vedges, (int, np.integer)) and not isinstance(vedges, (bool, np.bool_)) and not 1 <= vedges <= MAX_EDGES:
        raise ValueError(f"1 .. {MAX_EDGES} bin edges, got {vedges}")

    dev = nbody._device()
    vd = v.detach().to(device=dev, dtype=v.dtype if v.dtype in (torch.float32, torch.float64) else torch.float64).reshape(-1).contiguous()
    md = None if mask is None else mask.to(device=dev).reshape(-1).contiguous()
    if md is not None and md.dtype not in (torch.bool, torch.uint8):
        md = md != 0
    edges, min_count = _vedges(vd if md is None else vd[md.bool()], vedges, min_count, cell_length)
    n_bins = len(edges) - 1
    B = 1 if batch is None else batch
    if n_bins < 1:      # fewer than two edges: no bin, as in the reference
        return np.zeros(0), np.zeros(0), np.zeros((B, 0) if batch is not None else 0)

    f32 = lambda x, rows: x.detach().to(device=dev, dtype=torch.float32).reshape(rows, n).contiguous()
    bat = a0 if a1 is None else a1      # the input that may carry the batch axis
    fixed0 = f32(a0, 1) if (a1 is not None or batch is None) else None
    chunks = _batch_chunks(dev, B, 4 * n, lambda b: (2 + b, n_bins), "mcpm_binned_workspace", n, len(edges))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out_t = np.zeros((B, n_bins), dtype=np.float64)
    for lo, hi, work, ws, res in chunks:
        rows = f32(bat[lo:hi] if batch is not None else bat, hi - lo) if (a1 is not None or batch is not None) else None
        d0, s0 = (fixed0, 0) if fixed0 is not None else (rows, n)
        d1, s1 = (rows, n if batch is not None else 0) if a1 is not None else (None, 0)
        _lib.call("mcpm_binned_sums_f32", stream, n, vd, int(vd.dtype == torch.float64), d0, s0, d1, s1, float(scale), md, hi - lo, edges,
                  len(edges), work, ws, res)
        res = res.cpu().numpy()
        vcount, vsum = res[0], res[1]      # the same bits from every chunk
        out_t[lo:hi] = res[2:]
    return _finish_bins(vcount, vsum, out_t, min_count, batch is not None)


# ------------------------------------------------------------------------------------------------
# real-space bins: public interface.  `mask` (not in the reference; cells where it is zero are skipped) lets full meshes of a cut sky be
# binned in place, without the compaction mesh[..., mask] the reference makes first.
def bin_and_aggregate(targets, values, vedges: int | float | list, min_count=1, aggr_fn=None, mask=None):
    """Bin the cells by `values` and aggregate `targets` per bin: (vcount, vmean, taggr), bins with vcount < min_count removed.
    min_count None: `vedges` are quantile levels (an int or a float spaces them over [0, 1]).  aggr_fn None: the mean, on the device;
    any other aggr_fn (np.median, ...) runs on the host, bin by bin, on the float64 targets -- the slow path, unbatched only."""
    return _binned(values, targets, None, 1., vedges, min_count, aggr_fn, mask)


def mse_radius(mesh0, mesh1, rmesh, cell_length, redges: int | float | list = None, aggr_fn=None, mask=None):
    """Mean squared error between mesh0 and mesh1 binned by radius, in (Mpc/h)^3: (rcount, rmean, mse).  redges None: shells
    sqrt(3) cell_length wide, the narrowest that stay connected."""
    return _binned(rmesh, mesh0, mesh1, float(cell_length) ** 3, redges, 1, aggr_fn, mask, cell_length)


def mse_value(mesh0, mesh1, cell_length, vedges: int | float | list, min_count=None, aggr_fn=None):
    """Mean squared error between mesh0 and mesh1 binned by the value of mesh0, in (Mpc/h)^3: (vcount, vmean, mse)."""
    return _binned(mesh0, mesh0, mesh1, float(cell_length) ** 3, vedges, min_count, aggr_fn)


def mse_wave(mesh0, mesh1, box_size, kedges: int | float | list = None, include_corners=True):
    """Mean squared error between mesh0 and mesh1 binned by wave number, in (Mpc/h)^3: (kcount, kmean, pow), the spectrum of the difference."""
    t0, t1 = torch.as_tensor(mesh0), torch.as_tensor(mesh1)
    if t1.is_cuda and not t0.is_cuda:
        t0 = t0.to(t1.device)
    elif t0.is_cuda and not t1.is_cuda:
        t1 = t1.to(t0.device)
    return _spectrum(t1 - t0, box_size=box_size, kedges=kedges, include_corners=include_corners)


def distr_radial(mesh, rmesh, cell_length, redges: int | float | list = None, aggr_fn=None, mask=None):
    """Radial distribution of the mesh, in (h/Mpc)^3: (rcount, rmean, mean of the mesh per shell / cell_length^3)."""
    rcount, rmean, maggr = _binned(rmesh, mesh, None, 1., redges, 1, aggr_fn, mask, cell_length)
    return rcount, rmean, maggr / float(cell_length) ** 3
