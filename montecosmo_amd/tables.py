"""The cosmology's look-up tables as the kernels take them: which arrays, in which order, uploaded once, kept how long.  A layout is a tuple
of names: the order of the float64 arrays in the one device tensor an entry point of include/mcpm.h reads.  `host_tables` builds them,
`on_device` returns them as a `Table` from the one store, `Table.bars` takes a cotangent apart by the same names, and `fd_pair` is the
central difference the table Jacobians are taken by.  No other module spells a table order or keeps a cosmology-keyed cache."""
import copy

import numpy as np
import torch

from . import power      # (nbody and bricks import this module: it reaches them when it is called)

# chi ascending with the scale factor at each node (the look-up chi2a), then the growth grid `a` and the growth tables on it
LIGHTCONE = ("chi", "a_of_chi", "a", "g", "f")                          # mcpm_observe_pos*_f32, mcpm_kaiser_sky*_f32
LIGHTCONE_VJP = ("chi", "a_of_chi", "a", "g", "g2", "f", "f2")          # mcpm_lightcone_tables_vjp_f32 (g2 raw: the -3/7 is the kernel's)
AP = ("chi", "a_of_chi", "a_fid", "chi_fid")                            # chi2a of the sampled cosmology, then a2chi of the fiducial one
DISTANCE = ("a_dist", "chi_dist")                                       # a | chi as the distance table stores them: sky2cell, sky_extent
CHI2A = ("chi", "a_of_chi")                                             # mcpm_interp_f32: the scale factors of the Lagrangian lattice
GROWTH = ("a", "g", "g2", "f", "f2")                                    # mcpm_interp_f32 (xp = 'a', fp = one of the others): growth_dev
POWER = ("ks", "pows")                                                  # mcpm_power_mult_f32, mcpm_kaiser_post_c64
TRANS = ("ks", "trans")                                                 # the PNG kernels (mcpm_png_*_f32)
_BACKGROUND, _FID, _POW = {"chi", "a_of_chi", "a_dist", "chi_dist", "a", "g", "g2", "f", "f2"}, {"a_fid", "chi_fid"}, {"ks", "pows", "trans"}
# what a derivative with respect to the cosmology does not move (the grids, the fiducial table): a table cotangent has the layout's others
FIXED = ("a_of_chi", "a", "a_dist", "a_fid", "chi_fid", "ks")


def host_tables(cosmo, layout, fid=None, kpow=None):
    """The arrays of `layout` as a dict of host float64 arrays.  `fid`: the fiducial cosmology (AP); `kpow`: (ks, pows) normalised to
    sigma8 = 1 in place of the Eisenstein & Hu table of `cosmo` (POWER, TRANS)."""
    from . import bricks, nbody
    need, t = set(layout), {}
    if need & _BACKGROUND:
        d = nbody._dist_cache(cosmo)
        t.update(nbody._growth_cache(cosmo), chi=d["chi"][::-1], a_of_chi=d["a"][::-1], a_dist=d["a"], chi_dist=d["chi"])
    if need & _FID:
        d = nbody._dist_cache(fid)
        t.update(a_fid=d["a"], chi_fid=d["chi"])
    if need & _POW:
        t["ks"], t["pows"] = power.lin_power_table(cosmo) if kpow is None else kpow
    if "trans" in need:
        t["trans"] = bricks.trans_phi2delta_table(cosmo, kpow=(t["ks"], t["pows"]))[1]
    return {k: np.ascontiguousarray(t[k], dtype=np.float64) for k in layout}


def _key(cosmo, layout, device, fid, kpow):
    """The values `host_tables` reads for this layout (equal keys, equal tables: `background` is what mcpm_growth_table and
    mcpm_distance_table read, with the table sizes); a given `kpow` counts by identity (the entry keeps it)."""
    from . import nbody
    background = lambda c: (*nbody._cosmo_params(c), nbody.growth_log10_amin, nbody.growth_steps, nbody.dist_log10_amin, nbody.dist_steps)
    need, key = set(layout), (layout, str(device))
    if need & _BACKGROUND or "trans" in need:      # (the transfer table reads a2g)
        key += background(cosmo)
    if need & _FID:
        key += background(fid)
    if need & _POW:
        key += (id(kpow[0]), id(kpow[1])) if kpow is not None else (float(cosmo.Omega_m), float(cosmo.Omega_b), float(cosmo.h), float(cosmo.n_s))
    if "trans" in need:      # its amplitude cancels: no sigma8
        key += (float(cosmo.Omega_m), float(cosmo.n_s))
    return key


def upload(array, device):
    """The one copy of a table to the device: every table this package uploads comes through here."""
    return torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64)).to(device)


class Table:
    """A layout's arrays in one float64 device tensor `t`; `n[name]` is each array's length, `v[name]` its view (for the entry points that
    take `xp` and `fp` as two pointers).  Shared between callers and read-only: the C ABI takes every table as const."""

    def __init__(self, layout, arrays, device, keep=None):
        self.layout, self.n, self.keep = layout, {k: len(arrays[k]) for k in layout}, keep
        self.t = upload(np.concatenate([arrays[k] for k in layout]), device)
        self.v = dict(zip(layout, torch.split(self.t, list(self.n.values()))))

    def bars(self, vec):
        """The inverse map: a cotangent vector over the layout's moving arrays (all but `FIXED`, in order) -> {name: float64 array}."""
        names = [k for k in self.layout if k not in FIXED]
        cuts = np.cumsum([self.n[k] for k in names])[:-1]
        return dict(zip(names, np.split(vec.cpu().numpy() if torch.is_tensor(vec) else np.array(vec), cuts)))


# One gradient on the light cone with png_type, ap_auto=True and the Eisenstein & Hu power asks for 7 tables of its cosmology (all but
# DISTANCE) and the POWER table of the two cosmologies of cosmo_vjp's central difference: 9 entries (tests/test_tables_host.py counts them).
BOUND = 16
_STORE = {}      # key -> Table, oldest first


def on_device(cosmo, layout, device, fid=None, kpow=None):
    """The `Table` of `layout` for this cosmology on `device`, from the store: built and uploaded when its key is new, at the cost of the
    oldest entry once `BOUND` are held (a context that keeps a table keeps it alive)."""
    kpow = None if kpow is None else (kpow[0], kpow[1])      # the two objects whose identity is the key: the entry holds them
    key = _key(cosmo, layout, device, fid, kpow)
    if key not in _STORE:
        while len(_STORE) >= BOUND:
            del _STORE[next(iter(_STORE))]
        _STORE[key] = Table(layout, host_tables(cosmo, layout, fid, kpow), device, keep=kpow)
    return _STORE[key]


def fd_pair(cosmo, name, rel_eps):
    """(h, [cosmology at +h, at -h]) of a central difference over one parameter, h = rel_eps max(|x|, 1e-2); 'Omega_m' varies Omega_c at fixed
    Omega_b.  Each copy has an empty `_workspace` of its own (a plain copy would share the dict): its tables derive from its own attributes."""
    attr = "Omega_c" if name == "Omega_m" else name
    base = float(getattr(cosmo, attr))
    h = rel_eps * max(abs(base), 1e-2)
    pair = [copy.copy(cosmo), copy.copy(cosmo)]
    for c, sgn in zip(pair, (+1, -1)):
        c._workspace = {}
        setattr(c, attr, base + sgn * h)
    return h, pair
