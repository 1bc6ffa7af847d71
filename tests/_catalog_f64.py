"""Float64 numpy statement of the reference's catalogue registration (montecosmo/model.py:1287-1362, bricks.py:882-1103,
utils.py:1186-1210), written from its text on top of the oracle's nufft, paint, chreshape, a2chi and phys2cell_pos.  Checker only."""
import numpy as np

from oracle import pm_oracle as o, background as obg
from oracle.bias_oracle import phys2cell_pos, rotvec_matrix


def radecrad2cart(ra, dec, radius):
    ra, dec = np.deg2rad(ra), np.deg2rad(dec)
    return np.moveaxis(radius * np.stack((np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec))), 0, -1)


def radecz2cart(cosmo, radecz):
    radius = o.a2chi(cosmo, 1 / (1 + np.asarray(radecz['Z'], dtype=np.float64)))
    return radecrad2cart(np.asarray(radecz['RA'], dtype=np.float64), np.asarray(radecz['DEC'], dtype=np.float64), radius)


def minmax_box(pos):
    low, high = pos.min(0), pos.max(0)
    return high - low, (low + high) / 2, np.zeros(pos.shape[-1])


def get_mesh_shape(box_size, cell_budget, padding=0.):
    box_size = np.multiply(box_size, 1 + padding)
    cell_length = float((box_size.prod() / cell_budget) ** (1 / 3))
    return tuple(int(s) for s in 2 * np.rint(box_size / cell_length / 2).astype(int)), cell_length


def cutsky2config(data, cosmo, cell_budget, padding=0., box_size=None, box_center=None, box_rotvec=None):
    computed = minmax_box(radecz2cart(cosmo, data))
    box_size, box_center, box_rotvec = (np.array(p) if p is not None else c for p, c in zip((box_size, box_center, box_rotvec), computed))
    final_shape, cell_length = get_mesh_shape(box_size, cell_budget, padding)
    return final_shape, cell_length, box_center, box_rotvec


def sky2cell(cosmo, data, box_center, box_rotvec, box_size, mesh_shape):
    return phys2cell_pos(radecz2cart(cosmo, data), box_center, rotvec_matrix(box_rotvec), box_size, mesh_shape)


def box2cell(pos, vel, los, vscale, box_center, box_rotvec, box_size, mesh_shape):
    pos, los = np.asarray(pos, dtype=np.float64), np.asarray(los, dtype=np.float64)
    if vel is not None:
        pos = pos + (np.asarray(vel, dtype=np.float64) * vscale * los).sum(-1, keepdims=True) * los
    return phys2cell_pos(pos, box_center, rotvec_matrix(box_rotvec), box_size, mesh_shape)


def _irfftn(spec, shape):
    return np.fft.irfftn(spec, s=shape, axes=(0, 1, 2))


def cutsky2selection(data, cosmo, mask_shape, selec_shape, paint_shape, box_size, box_center, box_rotvec, paint_order=2,
                     interlace_order=2, paint_deconv=True, keep=None):
    """-> (selec_mesh, mask at selec_shape, mask at mask_shape).  `keep`: a bool array, the objects the masks are painted from
    (the fragile-cell rule of the tests); the selection always takes them all."""
    w = np.asarray(data['WEIGHT'], dtype=np.float64)
    pos = sky2cell(cosmo, data, box_center, box_rotvec, box_size, selec_shape)
    selec = _irfftn(o.nufft(pos, selec_shape, paint_shape, w, paint_order, interlace_order, paint_deconv), selec_shape)
    k = slice(None) if keep is None else keep
    mask_selec = o.paint(pos[k], selec_shape, w[k], paint_order) > 0
    selec = selec / selec[mask_selec].mean()
    pos_mask = pos * np.divide(mask_shape, selec_shape)
    mask = o.paint(pos_mask[k], mask_shape, w[k], paint_order) > 0
    return selec, mask_selec, mask


def face_distance(cosmo, data, box_size, box_center, box_rotvec, selec_shape, mask_shape):
    """Per object: its smallest distance to a cell face, in cells, at selec_shape and at mask_shape."""
    pos = sky2cell(cosmo, data, box_center, box_rotvec, box_size, selec_shape)
    pm = pos * np.divide(mask_shape, selec_shape)
    return np.abs(pos - np.rint(pos)).min(-1), np.abs(pm - np.rint(pm)).min(-1)


def register_catalog(cell_budget, cosmo, data, random=None, box_size=None, box_center=None, box_rotvec=None, a_obs=None, los=None,
                     padding=0., init_oversamp=3 / 2, paint_oversamp=7 / 4, paint_order=2, interlace_order=2, paint_deconv=True):
    paint = dict(paint_order=paint_order, interlace_order=interlace_order, paint_deconv=paint_deconv)
    if random is not None:
        final_shape, cell_length, box_center, box_rotvec = cutsky2config(random, cosmo, cell_budget, padding, box_size, box_center, box_rotvec)
    else:
        box_rotvec = np.zeros(3) if box_rotvec is None else np.asarray(box_rotvec)
        final_shape, cell_length = get_mesh_shape(box_size, cell_budget, 0.)
    box_size = np.multiply(final_shape, cell_length)
    init_shape, paint_shape = o.scale_shape(final_shape, init_oversamp), o.scale_shape(final_shape, paint_oversamp)
    out = dict(final_shape=final_shape, init_shape=init_shape, paint_shape=paint_shape, cell_length=cell_length, box_size=box_size,
               box_rotvec=np.asarray(box_rotvec))
    if random is not None:
        selec, mask_selec, mask = cutsky2selection(random, cosmo, final_shape, init_shape, paint_shape, box_size, box_center, box_rotvec, **paint)
        selec = _irfftn(o.chreshape(np.fft.rfftn(selec), o.r2chshape(paint_shape)), paint_shape)
        pos = sky2cell(cosmo, data, box_center, box_rotvec, box_size, final_shape)
        count = _irfftn(o.nufft(pos, final_shape, paint_shape, np.asarray(data['WEIGHT'], dtype=np.float64), **paint), final_shape)
        out.update(selec_mesh=selec, mask_selec=mask_selec, mask_mesh=mask, count_mesh=count, box_center=np.asarray(box_center),
                   n_tracers=float(np.sum(data['WEIGHT'])), n_randoms=float(np.sum(random['WEIGHT'])))
    else:
        vscale = 1. / (a_obs * 100 * obg.Esqr(cosmo, a_obs) ** .5)
        pos = box2cell(data['pos'], data.get('vel'), los, vscale, box_center, box_rotvec, box_size, final_shape)
        w = np.asarray(data['WEIGHT'], dtype=np.float64) if 'WEIGHT' in data else 1.
        count = _irfftn(o.nufft(pos, final_shape, paint_shape, w, **paint), final_shape)
        out.update(count_mesh=count, box_center=np.multiply(los, o.a2chi(cosmo, a_obs)), n_tracers=float(count.sum()))
    return out


def footprint(pos, shape, weights=None, order=2):
    """The exact footprint on float32 positions, as the paint kernels define it: id0 = floor (even order) or round-half-even (odd)
    of the float32 coordinate, fraction f = pos - id0 in float32, per-axis float32 weights (CIC: 1 - f and f), periodic wrap; a cell
    is marked when an object of positive weight has a non-zero weight there on every axis.  Orders 1 and 2."""
    pos = np.asarray(pos, dtype=np.float32)
    keep = np.ones(len(pos), bool) if weights is None else np.asarray(weights, dtype=np.float32) > 0
    pos = pos[keep]
    mask = np.zeros(shape, dtype=bool)
    fl = np.floor(pos)
    fr = pos - fl                                   # float32, exact or rounded as the kernel's `t - floorf(t)`
    b = fl.astype(np.int64)
    if order == 1:
        up = (fr > 0.5) | ((fr == 0.5) & (b % 2 == 1))
        c = (b + up) % np.asarray(shape)
        mask[c[:, 0], c[:, 1], c[:, 2]] = True
        return mask
    assert order == 2
    k = np.stack([np.float32(1) - fr, fr], axis=0)      # (2, N, 3)
    for a in range(2):
        for bb in range(2):
            for e in range(2):
                on = (k[a, :, 0] != 0) & (k[bb, :, 1] != 0) & (k[e, :, 2] != 0)
                c = (b[on] + np.array([a, bb, e])) % np.asarray(shape)
                mask[c[:, 0], c[:, 1], c[:, 2]] = True
    return mask
