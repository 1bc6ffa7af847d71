"""Float64 numpy restatement of the Kaiser model off the flat sky at fixed a (montecosmo/bricks.py:200-231 with the geometry of
`los_scalefactor_mesh`, bricks.py:760-778, and model.py:690-695), the checker of tests/test_kaiser_sky_host.py and
tests/test_gpu_kaiser_sky*.py.  The curved-sky l = 2 part goes through the HARMONIC route of the reference (metrics.py:412-445: real
spherical harmonics from scipy.special.lpmv, one irfftn per m), so that the kernels' tensor form sum_ab l_a l_b irfftn(k_a k_b / k^2 lin)
is checked against an independent path; `mu2_delta_tensor` restates the tensor form for the host test that equates the two.
np.fft.irfftn is applied as numpy applies it (the kz = 0 / Nyquist planes of a product need not be Hermitian); tables through np.interp.

Every operator here is  out = 1 + sum_t w_t(x) irfftn(m_t(k) lin)  with real m_t, w_t: `terms` lists the (m_t, w_t), `kaiser_sky`
sums them and `kaiser_sky_lin_vjp` is the exact transpose  lin_bar = sum_t m_t irfftn_vjp(w_t out_bar)  (real-pair convention)."""
import numpy as np
from scipy.special import lpmv

from oracle import bias_oracle as bo, pm_oracle as o


def cell_positions(cfg, shape):
    """x = (i, j, k) box_size / shape - box_size / 2 + R^T box_center, in cell axes; array shape + (3,)."""
    box = np.asarray(cfg["box_size"], dtype=np.float64)
    c = bo.rotvec_matrix(cfg["box_rotvec"]).T @ np.asarray(cfg["box_center"], dtype=np.float64)
    idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)
    return idx * (box / np.asarray(shape)) - box / 2 + c, c


def default_tables(cosmo):
    """chi ascending, a(chi), and the growth tables of the oracle's cosmology."""
    d, g = o._dist_table(cosmo), o.growth_table(cosmo)
    return {"chi": d["chi"][::-1].copy(), "a_chi": d["a"][::-1].copy(), "a": g["a"], "g": g["g"], "f": g["f"]}


def geometry(cfg, cosmo, shape, tables=None, gf=None):
    """(r, l, g, f) per cell: l is None on the flat sky; g, f are scalars at fixed a_obs (`gf` overrides them)."""
    x, c = cell_positions(cfg, shape)
    if cfg["curved_sky"]:
        r = np.linalg.norm(x, axis=-1)
        l = o.safe_div(x, r[..., None])
    else:
        r, l = np.abs(x @ o.safe_div(c, np.linalg.norm(c))), None
    if gf is not None:
        return r, l, gf[0], gf[1]
    T = default_tables(cosmo) if tables is None else tables
    a = np.interp(r, T["chi"], T["a_chi"]) if cfg["a_obs"] is None else cfg["a_obs"]
    return r, l, np.interp(a, T["a"], T["g"]), np.interp(a, T["a"], T["f"])


def real_sph_harm2(m, vec):
    """Real spherical harmonic Y_2m of the direction of `vec` (..., 3) (metrics.py:373-391); 0 for the zero vector."""
    n = np.linalg.norm(vec, axis=-1)
    ct = o.safe_div(vec[..., 2], n)
    ph = np.arctan2(vec[..., 1], vec[..., 0])
    ma = abs(m)
    fact = {0: 1., 1: 1. / 6., 2: 1. / 24.}[ma]                      # (2 - m)! / (2 + m)!
    norm = (5. / (4. * np.pi) * fact) ** .5
    leg = lpmv(ma, 2, ct)
    y = norm * leg if m == 0 else 2 ** .5 * norm * leg * (np.cos(ma * ph) if m > 0 else np.sin(ma * ph))
    return np.where(n == 0, 0., y)


def kvec_cell(shape):
    return np.stack(np.broadcast_arrays(*o.rfftk(tuple(shape))), axis=-1)


def _irfftn(X, shape):
    return np.fft.irfftn(X, s=tuple(shape), axes=(0, 1, 2))


def mu2_delta(lin, l):
    """(delta, delta / 3 + 8 pi / 15 sum_m Y_2m(l) irfftn(Y_2m(k) lin)) with k in cell units: optim_mu2_delta (metrics.py:412-445)."""
    shape = o.ch2rshape(lin.shape)
    kv = kvec_cell(shape)
    delta = _irfftn(lin, shape)
    out = delta / 3
    for m in range(-2, 3):
        out = out + 8 * np.pi / 15 * real_sph_harm2(m, l) * _irfftn(real_sph_harm2(m, kv) * lin, shape)
    return delta, out


def mu2_delta_tensor(lin, l):
    """sum_ab l_a l_b irfftn(k_a k_b / k^2 lin), k in cell units: the form the kernels evaluate."""
    shape = o.ch2rshape(lin.shape)
    kv = o.rfftk(tuple(shape))
    kk = sum(k ** 2 for k in kv)
    return sum(l[..., a] * l[..., b] * _irfftn(o.safe_div(kv[a] * kv[b], kk) * lin, shape) for a in range(3) for b in range(3))


def flat_mu2(cfg, shape):
    """mu^2 = (k . los)^2 / k^2 with k in h/Mpc and los the direction of R^T box_center (bricks.py:201-204)."""
    kv = o.rfftk(tuple(shape), np.asarray(cfg["box_size"], dtype=np.float64))
    c = bo.rotvec_matrix(cfg["box_rotvec"]).T @ np.asarray(cfg["box_center"], dtype=np.float64)
    los = o.safe_div(c, np.linalg.norm(c))
    return o.safe_div(sum(k * li for k, li in zip(kv, los)) ** 2, sum(k ** 2 for k in kv))


def trans_mesh(trans, cfg, shape):
    kv = o.rfftk(tuple(shape), np.asarray(cfg["box_size"], dtype=np.float64))
    return np.interp(np.sqrt((kv[0] ** 2 + kv[1] ** 2) + kv[2] ** 2), trans[0], trans[1], left=0., right=0.)


def terms(cfg, cosmo, shape, b1E, fNL_bp=0., trans=None, tables=None, gf=None):
    """[(name, m(k), w(x))] with out = 1 + sum w irfftn(m lin), and the geometry (r, g)."""
    r, l, g, f = geometry(cfg, cosmo, shape, tables, gf)
    one = np.ones(o.r2chshape(tuple(shape)))
    if cfg["curved_sky"]:
        kv = kvec_cell(shape)
        out = [("delta", one, g * b1E), ("delta/3", one, g * f / 3)]
        out += [("l2", real_sph_harm2(m, kv), g * f * 8 * np.pi / 15 * real_sph_harm2(m, l)) for m in range(-2, 3)]
    else:
        mu2 = flat_mu2(cfg, shape)
        out = [("delta", one, g * b1E), ("delta/3", one, g * f / 3), ("l2", mu2 - one / 3, g * f * np.ones(tuple(shape)))]
    if trans is not None:
        out.append(("phi", o.safe_div(1., trans_mesh(trans, cfg, shape)), fNL_bp * np.ones(tuple(shape))))
    return out, r, g


def kaiser_sky(cfg, cosmo, lin, b1E, fNL_bp=0., trans=None, tables=None, gf=None, return_parts=False):
    """1 + g(a) [ b1E delta + f(a) mu2_delta ] + fNL_bp phi on the mesh of `lin` (complex half-spectrum).  cfg: 'box_size', 'box_center',
    'box_rotvec', 'a_obs' (None: light cone), 'curved_sky'.  trans = (ks, t) adds phi = irfftn(safe_div(lin, t(|k|))), |k| in h/Mpc.
    tables: {'chi' ascending, 'a_chi', 'a', 'g', 'f'} instead of the cosmology's; gf: (g, f) instead of the look-up at a_obs.
    return_parts: also {'l2': the l = 2 term g f (mu2_delta - delta / 3), 'phi': fNL_bp phi, 'r', 'g'}."""
    lin = np.asarray(lin, dtype=np.complex128)
    shape = o.ch2rshape(lin.shape)
    tt, r, g = terms(cfg, cosmo, shape, b1E, fNL_bp, trans, tables, gf)
    parts = {"l2": 0., "phi": 0., "r": r, "g": g}
    out = np.ones(tuple(shape))
    for name, m, w in tt:
        v = w * _irfftn(m * lin, shape)
        out = out + v
        if name in parts:
            parts[name] = parts[name] + v
    return (out, parts) if return_parts else out


def kaiser_sky_lin_vjp(cfg, cosmo, out_bar, b1E, fNL_bp=0., trans=None, tables=None, gf=None):
    """Exact transpose of `kaiser_sky` in `lin` (real-pair convention): sum_t m_t irfftn_vjp(w_t out_bar)."""
    ob = np.asarray(out_bar, dtype=np.float64)
    tt, _, _ = terms(cfg, cosmo, ob.shape, b1E, fNL_bp, trans, tables, gf)
    return sum(m * o.irfftn_vjp(w * ob) for _, m, w in tt)


def evolve(cfg, cosmo, bias, white, png=None, png_type=None, trans=None):
    """FieldLevelModel.evolve for evolution 'kaiser' on any sky (model.py:686-695), in the shape of oracle.bias_oracle.evolve: the flat sky
    at fixed a_obs goes to the oracle; `png` (with `png_type`) adds fNL_bp phi with the transfer table of cfg['lin_kpow'], or with
    `trans` = (ks, t) in its place (so that a test can move its entries)."""
    if not cfg["curved_sky"] and cfg["a_obs"] is not None and png_type is None:
        return bo.evolve(cfg, cosmo, bias, white)
    import _png_f64 as pf
    kpow = cfg["lin_kpow"]
    if kpow is None:
        from oracle import power_oracle
        kpow = power_oracle.lin_power_table(cosmo)
    lin = bo.white2lin(cosmo.sigma8, white, cfg["init_shape"], cfg["box_size"], kpow)
    lin = o.chreshape(lin, o.r2chshape(cfg["evol_shape"]))
    fNL_bp = 0.
    if png_type is not None:
        fNL_bp = pf.fNL_bias({k: (png or {}).get(k, 0.) for k in pf.PNG_KEYS}, bias, 1., png_type)["fNL_bp"]
        trans = pf.trans_table(cosmo, kpow=cfg["lin_kpow"]) if trans is None else trans
    else:
        trans = None
    out = kaiser_sky(cfg, cosmo, lin, 1. + bias["b1"], fNL_bp, trans)
    cosmo._workspace = {}
    return out, None
