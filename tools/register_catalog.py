"""Catalogue -> register file.

    python tools/register_catalog.py --data data.npz --random randoms.npz --cell-budget 2e7 --padding 0.2 -o mock.npz     # cut sky
    python tools/register_catalog.py --data box.npz --box-size 2000 --a-obs 0.7 --cell-budget 2e7 -o mock.npz             # full sky

Cut sky: both files hold the columns RA, DEC (degrees), Z and WEIGHT.  Full sky: `pos` (N, 3) in Mpc/h and optionally `vel`, `WEIGHT`;
the box is periodic with side --box-size and corner at the origin unless --box-center says otherwise.  Several --data / --random files are
read as chunks of one catalogue.  .npz files only; .fits files are read when `fitsio` is installed.  The register is written with
`save_register` (.npz, or .h5 with h5py) and its geometry printed."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_table(path, columns):
    if path.endswith((".fits", ".fits.gz", ".fit")):
        try:
            import fitsio
        except ImportError:
            raise SystemExit(f"{path}: reading FITS needs fitsio, which is not installed; convert the catalogue to .npz")
        return fitsio.read(path, columns=list(columns))
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", nargs="+", required=True)
    ap.add_argument("--random", nargs="+", default=None, help="randoms (cut sky); without them the data are a periodic box")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--cell-budget", type=float, required=True)
    ap.add_argument("--padding", type=float, default=0.)
    ap.add_argument("--box-size", type=float, nargs="+", default=None, help="one side or three (full sky: required)")
    ap.add_argument("--box-center", type=float, nargs=3, default=None)
    ap.add_argument("--box-rotvec", type=float, nargs=3, default=None)
    ap.add_argument("--a-obs", type=float, default=None)
    ap.add_argument("--los", type=float, nargs=3, default=None)
    ap.add_argument("--init-oversamp", type=float, default=3 / 2)
    ap.add_argument("--paint-oversamp", type=float, default=7 / 4)
    ap.add_argument("--paint-order", type=int, default=2)
    ap.add_argument("--interlace-order", type=int, default=2)
    ap.add_argument("--no-paint-deconv", action="store_true")
    ap.add_argument("--chunk", type=int, default=None, help="objects on the device at a time (default 2^24)")
    ap.add_argument("--Omega-m", type=float, default=None, help="fiducial cosmology: Planck18 with this Omega_m")
    ap.add_argument("--sigma8", type=float, default=None)
    a = ap.parse_args(argv)

    from montecosmo_amd import bricks, register
    cosmo = bricks.Planck18(**({} if a.sigma8 is None else {"sigma8": a.sigma8}))
    if a.Omega_m is not None:
        cosmo.Omega_c = a.Omega_m - cosmo.Omega_b
    box_size = None if a.box_size is None else (a.box_size * 3 if len(a.box_size) == 1 else a.box_size)
    if box_size is not None and len(box_size) != 3:
        ap.error("--box-size takes one value or three")
    cut_sky = a.random is not None
    cols = ("RA", "DEC", "Z", "WEIGHT")
    data = [read_table(p, cols) for p in a.data]
    random = [read_table(p, cols) for p in a.random] if cut_sky else None
    kw = dict(box_size=box_size, box_center=a.box_center, box_rotvec=a.box_rotvec, a_obs=a.a_obs, los=a.los)
    if not cut_sky:
        kw["los"] = (0., 0., 1.) if a.los is None else a.los
        if box_size is not None and a.box_center is None:
            kw["box_center"] = tuple(b / 2 for b in box_size)      # positions in [0, box_size[: the corner is the origin
    reg = register.register_catalog(a.cell_budget, cosmo, data, random, padding=a.padding, init_oversamp=a.init_oversamp,
                                    paint_oversamp=a.paint_oversamp, paint_order=a.paint_order, interlace_order=a.interlace_order,
                                    paint_deconv=not a.no_paint_deconv, chunk=a.chunk, **kw)
    register.save_register(a.output, reg)
    shape = reg["count_mesh"].shape
    print(f"{'cut sky' if cut_sky else 'full sky'} register -> {a.output}")
    print(f"  final_shape {shape}  cell_length {reg['cell_length']:.6g} Mpc/h  box_size {tuple(np.multiply(shape, reg['cell_length']).round(3))}")
    print(f"  box_center {tuple(np.round(reg['box_center'], 3))}  box_rotvec {tuple(np.round(reg['box_rotvec'], 6))}")
    print(f"  n_tracers {reg['n_tracers']:.8g}" + (f"  n_randoms {reg['n_randoms']:.8g}  observed cells {int(reg['mask_mesh'].sum())} of "
                                                  f"{reg['mask_mesh'].size}" if cut_sky else f"  a_obs {reg['a_obs']}"))


if __name__ == "__main__":
    main()
