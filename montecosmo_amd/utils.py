"""Host helpers with the names of montecosmo/utils.py that the PM path uses (utils.py:21-29, :769-782,
:1163-1168, :1186-1210)."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def safe_div(x, y):
    """Division where x / 0 := 0 (utils.py:21-29)."""
    y = np.asarray(y)
    nz = y != 0
    return np.where(nz, x / np.where(nz, y, 1), 0)


def ch2rshape(shape):
    """Complex Hermitian shape -> real shape, last real dim assumed even (utils.py:769-776)."""
    shape = tuple(int(s) for s in shape)
    return shape[:-1] + (2 * (shape[-1] - 1),)


def r2chshape(shape):
    """Real shape -> complex Hermitian shape (utils.py:778-782)."""
    shape = tuple(int(s) for s in shape)
    return shape[:-1] + (shape[-1] // 2 + 1,)


def scale_shape(shape, scale=1.):
    """Valid (even) scaled mesh shape (utils.py:1163-1168)."""
    return tuple(int(2 * np.rint(s * scale / 2)) for s in shape)


def mesh2masked(mesh, mask=None):
    """mesh[..., mask]: the observed cells of a mesh (or of a batch of meshes) as a vector (utils.py:1171-1175); numpy or torch, the
    mask goes where the mesh is.  mask None: the mesh itself."""
    if mask is None:
        return mesh
    if torch.is_tensor(mesh):
        return mesh[..., torch.as_tensor(mask, device=mesh.device).bool()]
    return np.asarray(mesh)[..., _host_mask(mask)]


def masked2mesh(masked, mask=None):
    """Inverse of mesh2masked with zeros in the unobserved cells (utils.py:1178-1183); keeps the dtype of `masked`."""
    if mask is None:
        return masked
    if torch.is_tensor(masked):
        m = torch.as_tensor(mask, device=masked.device).bool()
        out = torch.zeros(tuple(masked.shape[:-1]) + tuple(m.shape), dtype=masked.dtype, device=masked.device)
        out[..., m] = masked
        return out
    masked, m = np.asarray(masked), _host_mask(mask)
    out = np.zeros(masked.shape[:-1] + m.shape, dtype=masked.dtype)
    out[..., m] = masked
    return out


def _host_mask(mask):
    return (mask.cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)).astype(bool)


def radecrad2cart(ra, dec, radius):
    """ra, dec (degrees) and radius -> cartesian coordinates (..., 3) (utils.py:1186-1196); host float64."""
    ra, dec = np.deg2rad(np.asarray(ra, dtype=np.float64)), np.deg2rad(np.asarray(dec, dtype=np.float64))
    x, y, z = np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)
    return np.moveaxis(np.asarray(radius, dtype=np.float64) * np.stack((x, y, z)), 0, -1)


def cart2radecrad(cart):
    """Cartesian coordinates (..., 3) -> ra in [0, 360], dec in [-90, 90] (degrees) and radius (utils.py:1199-1210); host float64.
    The origin maps to (0, 0, 0) (safe_div)."""
    cart = np.asarray(cart, dtype=np.float64)
    radius = np.linalg.norm(cart, axis=-1)
    x, y, z = np.moveaxis(cart, -1, 0)
    ra = np.rad2deg(np.arctan2(y, x)) % 360.
    dec = np.rad2deg(np.arcsin(np.clip(safe_div(z, radius), -1., 1.)))
    return ra, dec, radius


def _dev(x, dtype):
    # `nbody` imports this module (it re-exports the helpers above, as the reference does), so it can only be imported here at call time
    from . import nbody
    return nbody._c64(x) if dtype is torch.complex64 else nbody._f32(x)


def _stream_of(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def chreshape(mesh, shape):
    """Reshape a complex Hermitian tensor to the half-spectrum shape `shape`, truncating or padding so that the
    Hermitian symmetry and the mean (hence the average power) are preserved (utils.py:981-1013).  HIP kernel
    `mcpm_chreshape_c64`; returns a complex64 device tensor."""
    x = _dev(mesh, torch.complex64)
    out = torch.empty(tuple(int(v) for v in shape), dtype=torch.complex64, device=x.device)
    _lib.call("mcpm_chreshape_c64", _stream_of(x), x, *ch2rshape(x.shape), out, *ch2rshape(shape))
    return out


def chreshape_vjp(out_bar, in_shape):
    """VJP of `chreshape`: cotangent of the reshaped spectrum -> cotangent of the input of half-spectrum shape
    `in_shape` (real-pair convention dL = Re sum conj(bar) dz)."""
    ob = _dev(out_bar, torch.complex64)
    ib = torch.empty(tuple(int(v) for v in in_shape), dtype=torch.complex64, device=ob.device)
    _lib.call("mcpm_chreshape_vjp_c64", _stream_of(ob), ob, *ch2rshape(ob.shape), ib, *ch2rshape(in_shape))
    return ib


def _norm_factor(norm, shape):
    """rg2cgh(x, norm) / rg2cgh(x, "backward"): the norms of utils.py:826-835 differ by a constant only
    (backward sqrt(M/2), ortho 1/sqrt(2), forward 1/sqrt(2 M))."""
    M = float(shape[0]) * float(shape[1]) * float(shape[2])
    if norm == "ortho":
        return M ** -0.5
    if norm == "forward":
        return 1.0 / M
    raise ValueError(f"unknown norm {norm!r}: 'backward', 'ortho', 'forward' (and 'amp' for cgh2rg)")


def rg2cgh(mesh, norm="backward"):
    """Permute and reweight a real Gaussian tensor (3D, even sizes) into a complex Gaussian Hermitian tensor
    distributed as rfftn of a real Gaussian tensor (utils.py:892-906).  HIP kernel mcpm_rg2cgh_f32."""
    x = _dev(mesh, torch.float32)
    out = torch.empty(r2chshape(x.shape), dtype=torch.complex64, device=x.device)
    _lib.call("mcpm_rg2cgh_f32", _stream_of(x), x, *x.shape, out)
    return out * _norm_factor(norm, x.shape) if norm != "backward" else out


def rg2cgh_vjp(meshk_bar):
    """VJP of rg2cgh: cotangent of the complex tensor (real-pair convention) -> cotangent of the real tensor."""
    kb = _dev(meshk_bar, torch.complex64)
    shape = ch2rshape(kb.shape)
    out = torch.empty(shape, dtype=torch.float32, device=kb.device)
    _lib.call("mcpm_rg2cgh_vjp_f32", _stream_of(kb), kb, *shape, out)
    return out


def cgh2rg(meshk, norm="backward"):
    """Permute and reweight a complex Gaussian Hermitian tensor into a real Gaussian tensor (utils.py:909-921): the
    inverse of rg2cgh.  norm="amp" lays a per-mode amplitude (the real part of `meshk`) out like the real tensor.
    HIP kernels mcpm_cgh2rg_f32 / mcpm_cgh2rg_amp_f32."""
    k = _dev(meshk, torch.complex64)
    shape = ch2rshape(k.shape)
    out = torch.empty(shape, dtype=torch.float32, device=k.device)
    _lib.call("mcpm_cgh2rg_amp_f32" if norm == "amp" else "mcpm_cgh2rg_f32", _stream_of(k), k, *shape, out)
    return out / _norm_factor(norm, shape) if norm not in ("backward", "amp") else out
