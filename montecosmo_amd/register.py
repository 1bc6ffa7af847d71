"""The on-disk "register" of a mock (reference: run/register.py:8-18 writes it, montecosmo/model.py:518-553 loads it): ONE
self-describing file per mock from which `FieldLevelModel(register=path)` takes its geometry, painting parameters, meshes
and fiducial cosmology.  This module reads and writes that schema and turns it into the arguments of this package's
`FieldLevelForward` / `FieldLevelLogDensity`.  `register_catalog` produces one here, from a galaxy catalogue and its randoms or from a
simulation box (the reference's `FieldLevelModel.register_catalog`, model.py:1287-1362); `tools/register_catalog.py` is its command line.

Schema (key: meaning; * = mandatory)
  * cell_length, box_center, box_rotvec      geometry (final_shape = count_mesh.shape)
  * init_oversamp, paint_oversamp            mesh oversampling
  * cosmo_fid/{Omega_m, sigma8}              fiducial cosmology of the mock (-> latents loc / loc_fid)
  * count_mesh                               painted tracer counts at final_shape (sum == n_tracers)
    selec_mesh, mask_mesh                    selection at paint_shape / footprint at final_shape (cut sky)
    n_tracers, n_randoms                     weighted catalog sizes
    a_obs, curved_sky                        full sky: 1 / (1 + z), False; cut sky: None (light cone), True
    paint_order, interlace_order, paint_deconv, kernel_type, cell_budget, padding
    lin_kpow                                 (2, N): k and P(k) / sigma8^2
    white_mesh | white_fake                  whitened initial conditions, half-spectrum at r2chshape(init_shape)
    png_type                                 'fNL' | 'bias' (absent / None: no primordial non-Gaussianity)
    bias_type                                'lagrangian' | 'eulerian' (model.py:68; absent / None: 'lagrangian')
    ap_auto                                  Alcock-Paczynski (model.py:64): True automatic (the catalogue was gridded with cosmo_fid),
                                             False alpha_iso / alpha_ap parameters, absent / None: none

Container: HDF5 through h5py, as the reference's `h5save` / `h5load` (utils.py:76-160) lay it out: one dataset per key,
nested dicts as groups, None left out.  h5py is an optional dependency (it is absent from the build image): `.npz` files with
'/'-joined keys carry the same schema everywhere, and `save_register` / `load_register` choose by the file suffix.
"""
import os

import numpy as np

MANDATORY = ("cell_length", "box_center", "box_rotvec", "init_oversamp", "paint_oversamp", "cosmo_fid", "count_mesh")
OPTIONAL = ("selec_mesh", "mask_mesh", "n_tracers", "n_randoms", "a_obs", "curved_sky", "paint_order", "interlace_order",
            "paint_deconv", "kernel_type", "cell_budget", "padding", "lin_kpow", "white_mesh", "white_fake", "png_type", "ap_auto", "bias_type")


def _flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        if v is None:
            continue                                    # h5save skips None (utils.py:104-106): absent == None on load
        if isinstance(v, dict):
            out.update(_flatten(v, prefix + k + "/"))
        else:
            out[prefix + k] = np.asarray(v)
    return out


def _unflatten(flat):
    out = {}
    for k, v in flat.items():
        node = out
        *groups, leaf = k.split("/")
        for g in groups:
            node = node.setdefault(g, {})
        v = np.asarray(v)
        if v.dtype.kind in ("S", "U") and v.ndim == 0:
            v = str(v.item().decode() if isinstance(v.item(), bytes) else v.item())
        elif v.ndim == 0:
            v = v.item()                                # 0-d scalar -> native python (utils.py:150-153)
        node[leaf] = v
    return out


def validate(reg):
    missing = [k for k in MANDATORY if k not in reg]
    if missing:
        raise KeyError(f"register is missing mandatory keys {missing}")
    unknown = [k for k in reg if k not in MANDATORY + OPTIONAL]
    if unknown:
        raise KeyError(f"register has keys outside the schema: {unknown}")
    for k in ("Omega_m", "sigma8"):
        if k not in reg["cosmo_fid"]:
            raise KeyError(f"cosmo_fid/{k} missing")
    if np.ndim(reg["count_mesh"]) != 3:
        raise ValueError("count_mesh must be a 3-D mesh (its shape is the model's final_shape)")
    return reg


def save_register(path, reg):
    """Writes `reg` (a dict following the schema above) to `path` (.h5 / .hdf5 through h5py, .npz otherwise)."""
    validate(reg)
    flat = _flatten(reg)
    if str(path).endswith((".h5", ".hdf5")):
        try:
            import h5py
        except ImportError as e:
            raise ImportError("writing an HDF5 register needs h5py; use a .npz path (same schema) where it is absent") from e
        with h5py.File(str(path), "w") as f:
            for k, v in flat.items():
                f.create_dataset(k, data=v.astype("S") if v.dtype.kind == "U" else v)
    else:
        np.savez(str(path), **{k.replace("/", "__"): v for k, v in flat.items()})
    return path


def load_register(path):
    """The dict `save_register` (or the reference's run/register.py) wrote."""
    if str(path).endswith((".h5", ".hdf5")):
        try:
            import h5py
        except ImportError as e:
            raise ImportError("reading an HDF5 register needs h5py") from e
        flat = {}
        with h5py.File(str(path), "r") as f:
            f.visititems(lambda name, obj: flat.__setitem__(name, obj[()]) if isinstance(obj, h5py.Dataset) else None)
    else:
        with np.load(str(path) if os.path.exists(str(path)) else str(path) + ".npz", allow_pickle=False) as z:
            flat = {k.replace("__", "/"): z[k] for k in z.files}
    return validate(_unflatten(flat))


def model_arguments(reg, **overrides):
    """What montecosmo/model.py:518-553 takes from a register, as keyword arguments for this package:
       forward   -> FieldLevelForward(**forward)  (geometry, oversampling, sky, painting, tabulated linear power)
       density   -> FieldLevelLogDensity(fwd, count_obs=density['count_mesh'], ..., selec_mesh=, mask_mesh=)
       loc       -> fiducial values of the latents: Omega_m, sigma8 from cosmo_fid, and ngbars = n_tracers / (observed cells
                    x cell_length^3) (model.py:546-549)
       white_mesh-> the registered initial conditions (or None).
    `overrides` replace forward arguments (evolution, nbody_n_steps, ...); `lik_type` among them (or in the register) goes to the
    density arguments instead: FieldLevelLogDensity(..., lik_type=density['lik_type'])."""
    validate(reg)
    lik_type = overrides.pop("lik_type", reg.get("lik_type"))
    count = np.asarray(reg["count_mesh"], dtype=np.float64)
    mask = None if reg.get("mask_mesh") is None else np.asarray(reg["mask_mesh"], dtype=bool)
    fwd = dict(final_shape=tuple(int(s) for s in count.shape), cell_length=float(reg["cell_length"]),
               box_center=tuple(float(v) for v in np.ravel(reg["box_center"])), box_rotvec=tuple(float(v) for v in np.ravel(reg["box_rotvec"])),
               init_oversamp=float(reg["init_oversamp"]), paint_oversamp=float(reg["paint_oversamp"]))
    for k in ("a_obs", "curved_sky", "paint_order", "interlace_order", "paint_deconv"):
        if k in reg:
            fwd[k] = reg[k]
    if reg.get("png_type") not in (None, "None"):      # 'fNL' or 'bias' (model.py:84); absent or None: no primordial non-Gaussianity
        fwd["png_type"] = str(reg["png_type"])
    if reg.get("bias_type") not in (None, "None"):     # 'lagrangian' or 'eulerian' (model.py:68); absent or None: the model's default, 'lagrangian'
        fwd["bias_type"] = str(reg["bias_type"])
    if reg.get("ap_auto") not in (None, "None"):       # True / False (model.py:64); absent or None: no Alcock-Paczynski
        from . import bricks
        v = reg["ap_auto"]
        if isinstance(v, str):                         # a container that hands strings back: 'True' / 'False', nothing else
            if v not in ("True", "False"):
                raise ValueError(f"register: ap_auto must be True, False or None, got {v!r}")
            v = v == "True"
        fwd["ap_auto"] = bool(v)
        fid = bricks.Planck18(sigma8=float(reg["cosmo_fid"]["sigma8"]))      # the cosmology register_catalog gridded the catalogue with
        fid.Omega_c = float(reg["cosmo_fid"]["Omega_m"]) - fid.Omega_b
        fwd["cosmo_fid"] = fid
    if reg.get("kernel_type", "rectangular") != "rectangular":
        raise NotImplementedError("FieldLevelForward paints with kernel_type='rectangular' (nbody.paint itself takes 'kaiser_bessel')")
    if reg.get("lin_kpow") is not None:
        lk = np.asarray(reg["lin_kpow"], dtype=np.float64)
        fwd["lin_kpow"] = (lk[0], lk[1])
    fwd.update(overrides)
    n_cells = int(mask.sum()) if mask is not None else count.size
    n_tracers = float(reg.get("n_tracers", count[mask].sum() if mask is not None else count.sum()))
    ngbar = n_tracers / (n_cells * float(reg["cell_length"]) ** 3)
    sel = reg.get("selec_mesh")
    sel = None if (sel is None or np.ndim(sel) == 0) else np.asarray(sel, dtype=np.float64)
    white = reg.get("white_mesh", reg.get("white_fake"))
    density = dict(count_mesh=count, selec_mesh=sel, mask_mesh=mask)
    if lik_type not in (None, "None"):
        density["lik_type"] = str(lik_type)
    return dict(forward=fwd, density=density,
                loc=dict(Omega_m=float(reg["cosmo_fid"]["Omega_m"]), sigma8=float(reg["cosmo_fid"]["sigma8"]), ngbars=ngbar),
                white_mesh=None if white is None else np.asarray(white))


def register_catalog(cell_budget: float, cosmo_fid, data, random=None, box_size=None, box_center=None, box_rotvec=None, a_obs=None,
                     los=None, padding: float = 0., init_oversamp: float = 3 / 2, paint_oversamp: float = 7 / 4, paint_order: int = 2,
                     interlace_order: int = 2, paint_deconv: bool = True, kernel_type: str = 'rectangular', chunk=None):
    """Register a catalogue into the meshes and metadata an inference-ready model needs (model.py:1287-1362):

    * cut sky (`random` given): `data` and `random` are (RA, DEC, Z, WEIGHT) dict-likes, or lists / tuples of them.  The geometry is
      fitted to the randoms, the selection (painted at init_shape, reshaped to paint_shape) and the footprint mask (final_shape) come
      from the randoms and the count from the data.  a_obs = None (light cone), curved sky.
    * full sky (`random` None): `data` holds cartesian 'pos' (and optional 'vel', 'WEIGHT'), as a dict-like or any iterable of them;
      `box_size` is the periodic box and there is no selection or mask.  With 'vel', redshift-space distortion at `a_obs` along `los`.

    Objects go to the device at most `chunk` at a time (default 2^24).  Returns a dict in this module's schema (host numpy arrays,
    the reference's keys) for `save_register`.  Wrong combinations, negative or non-finite weights, non-finite coordinates and a 'vel'
    of another shape than 'pos' raise ValueError (the columns are scanned once, where the catalogue enters), a one-shot iterator on
    the cut sky TypeError, another kernel_type NotImplementedError -- all before any device work (a lazily read full-sky iterator is
    checked table by table as it is read)."""
    from . import bricks, nbody, utils
    cut_sky = random is not None
    chunk = bricks.CATALOG_CHUNK if chunk is None else int(chunk)
    if kernel_type != 'rectangular':
        raise NotImplementedError("register_catalog paints with kernel_type='rectangular' (nbody.paint itself takes 'kaiser_bessel')")
    if chunk < 1:
        raise ValueError("chunk must be a positive number of objects")
    if not cell_budget > 0 or padding < 0:
        raise ValueError("cell_budget must be positive and padding non-negative")
    if cut_sky:
        if a_obs is not None or los is not None:
            raise ValueError("For cut-sky catalog, a_obs and los must be None (light-cone, curved-sky)")
        data, random = bricks.checked_tables(data, bricks.SKY_KEYS, "data"), bricks.checked_tables(random, bricks.SKY_KEYS, "random")
        curved_sky = True
        final_shape, cell_length, box_center, box_rotvec, n_randoms = bricks._cutsky_box(
            random, cosmo_fid, cell_budget, padding, box_size, box_center, box_rotvec, chunk, "random")
    else:
        if a_obs is None or los is None or box_size is None or box_center is None:
            raise ValueError("For full-sky catalog, a_obs, los, box_size, and box_center must be provided")
        data = bricks.checked_tables(data, ('pos',), "data", optional=('vel',), iterable_ok=True)      # an iterator: checked as it is read
        box_rotvec = np.zeros(3) if box_rotvec is None else np.asarray(box_rotvec, dtype=np.float64)
        final_shape, cell_length = bricks.get_mesh_shape(box_size, cell_budget, padding=0.)
        curved_sky = False
    paint = dict(paint_order=paint_order, interlace_order=interlace_order, paint_deconv=paint_deconv, chunk=chunk)
    box_size = np.multiply(final_shape, cell_length)      # box_size update due to rounding and padding
    init_shape = utils.scale_shape(final_shape, init_oversamp)
    paint_shape = utils.scale_shape(final_shape, paint_oversamp)

    if cut_sky:
        selec_mesh, mask_mesh = bricks.cutsky2selection(random, cosmo_fid, mask_shape=final_shape, selec_shape=init_shape,
                                                        paint_shape=paint_shape, box_size=box_size, box_center=box_center,
                                                        box_rotvec=box_rotvec, **paint)
        selec_mesh = nbody.irfftn(utils.chreshape(nbody.rfftn(selec_mesh), utils.r2chshape(paint_shape)))
        selec_mesh, mask_mesh = selec_mesh.cpu().numpy(), mask_mesh.cpu().numpy()
        count_mesh = bricks.cutsky2count(data, cosmo_fid, final_shape, paint_shape, box_size=box_size, box_center=box_center,
                                         box_rotvec=box_rotvec, **paint).cpu().numpy()
        n_tracers = bricks.weighted_size(data)
    else:
        count_mesh = bricks.fullsky2count(data, cosmo_fid, a_obs, los=los, box_size=box_size, box_center=box_center,
                                          box_rotvec=box_rotvec, final_shape=final_shape, paint_shape=paint_shape, **paint).cpu().numpy()
        box_center = np.multiply(np.asarray(los, dtype=np.float64), nbody.a2chi(cosmo_fid, a_obs))      # real box_center, coherent with the los
        n_tracers = float(count_mesh.sum(dtype=np.float64))
        selec_mesh = mask_mesh = n_randoms = None

    return validate({
        'cell_length': float(cell_length), 'box_center': np.asarray(box_center), 'box_rotvec': np.asarray(box_rotvec),
        'init_oversamp': float(init_oversamp), 'paint_oversamp': float(paint_oversamp),
        'cosmo_fid': {'Omega_m': float(cosmo_fid.Omega_m), 'sigma8': float(cosmo_fid.sigma8)},
        'count_mesh': count_mesh,
        'selec_mesh': selec_mesh, 'mask_mesh': mask_mesh,
        'n_tracers': n_tracers, 'n_randoms': n_randoms,
        'a_obs': a_obs, 'curved_sky': curved_sky,
        'paint_order': int(paint_order), 'interlace_order': int(interlace_order),
        'paint_deconv': bool(paint_deconv), 'kernel_type': kernel_type,
        'cell_budget': float(cell_budget), 'padding': float(padding),
    })
