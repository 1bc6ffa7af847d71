"""Float64 numpy restatement of the real-space binned diagnostics (montecosmo/metrics.py `bin_and_aggregate`, `mse_radius`,
`mse_value`, `mse_wave`, `distr_radial`), the checker of tests/test_binned_host.py and tests/test_gpu_binned.py.  Everything is
float64: the values, the edges found from them, the targets.  Each function returns one more array than the module's: the mean of
|target| per kept bin (times whatever factor the function applies to its aggregate), the scale against which the rounding error of
a bin's sum is judged; with an `aggr_fn` it is the same mean of |target|."""
import numpy as np

import _spectrum_f64 as spec


def vedges(values, vedges, min_count=1, cell_length=None):
    """-> (edges, min_count): list as given; int = number of edges; float = bin width; None = sqrt(3) cell_length wide; the int and
    float cases give the centres of n equal cells of [vmin, vmax], the range of the values, or of [0, 1] with min_count None, and
    min_count None turns the edges into quantiles of the values."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    if vedges is None:
        vedges = 3 ** .5 * cell_length
    if isinstance(vedges, (int, float)):
        vmin, vmax = (0., 1.) if min_count is None else (values.min(), values.max())
        n = vedges if isinstance(vedges, int) else max(int((vmax - vmin) / vedges), 1)
        vedges = np.linspace(vmin, vmax, n, endpoint=False) + (vmax - vmin) / n / 2
    vedges = np.asarray(vedges, dtype=np.float64)
    if min_count is None:
        vedges = np.quantile(values, vedges)
        min_count = 1
    return vedges, min_count


def bin_and_aggregate(targets, values, edges, min_count=1, aggr_fn=None, cell_length=None):
    """(vcount, vmean, taggr, tabs); targets may carry one more leading axis than values (taggr and tabs then do too)."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    targets = np.asarray(targets, dtype=np.float64)
    batched = targets.size != values.size
    targets = targets.reshape(-1, values.size)
    edges, min_count = vedges(values, edges, min_count, cell_length)
    n_bins = len(edges) + 1
    dig = np.digitize(values, edges)
    vcount = np.bincount(dig, minlength=n_bins)[1:-1].astype(np.float64)
    keep = vcount >= min_count
    vcount = vcount[keep]
    vmean = np.bincount(dig, weights=values, minlength=n_bins)[1:-1][keep] / vcount
    tabs = np.stack([np.bincount(dig, weights=np.abs(t), minlength=n_bins)[1:-1][keep] / vcount for t in targets])
    if aggr_fn is None:
        taggr = np.stack([np.bincount(dig, weights=t, minlength=n_bins)[1:-1][keep] / vcount for t in targets])
    else:
        taggr = np.stack([np.array([aggr_fn(t[dig == i]) for i in range(1, n_bins - 1)], dtype=np.float64).reshape(n_bins - 2)[keep]
                          for t in targets])
    if not batched:
        taggr, tabs = taggr[0], tabs[0]
    return vcount, vmean, taggr, tabs


def _se(mesh0, mesh1, cell_length):
    return (np.asarray(mesh0, dtype=np.float64) - np.asarray(mesh1, dtype=np.float64)) ** 2 * cell_length ** 3


def mse_radius(mesh0, mesh1, rmesh, cell_length, redges=None, aggr_fn=None):
    return bin_and_aggregate(_se(mesh0, mesh1, cell_length), rmesh, redges, 1, aggr_fn, cell_length)


def mse_value(mesh0, mesh1, cell_length, vedges, min_count=None, aggr_fn=None):
    return bin_and_aggregate(_se(mesh0, mesh1, cell_length), mesh0, vedges, min_count, aggr_fn)


def mse_wave(mesh0, mesh1, box_size, kedges=None, include_corners=True):
    """(kcount, kmean, pow, pabs) of the spectrum of mesh1 - mesh0."""
    return spec.spectrum(np.asarray(mesh1, dtype=np.float64) - np.asarray(mesh0, dtype=np.float64), box_size=box_size, kedges=kedges,
                         include_corners=include_corners)


def distr_radial(mesh, rmesh, cell_length, redges=None, aggr_fn=None):
    rcount, rmean, maggr, mabs = bin_and_aggregate(mesh, rmesh, redges, 1, aggr_fn, cell_length)
    return rcount, rmean, maggr / cell_length ** 3, mabs / cell_length ** 3


def radius_mesh(shape, box_center, cell_length):
    """|x| of the cell corners of an unrotated box of `shape` cells around box_center (the curved-sky radius of the model)."""
    g = np.indices(shape).astype(np.float64)
    x = [(g[i] - shape[i] / 2) * cell_length + box_center[i] for i in range(3)]
    return np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2)
