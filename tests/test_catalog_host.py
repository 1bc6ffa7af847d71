"""Catalogue registration, host side (no GPU): mesh shapes, bounding boxes, sky coordinates, the five exported calls, and every
refusal of `register_catalog`, each of which comes before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _catalog_f64 as ref
from oracle import background as obg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("mcpm_sky2cart_minmax_f64", "mcpm_sky2cell_f32", "mcpm_box2cell_f32", "mcpm_footprint_u8", "mcpm_masked_sum_f64")


def test_get_mesh_shape():
    from montecosmo_amd import bricks
    box = np.array([1000., 1500., 700.])
    keep = box.copy()
    shape, cell = bricks.get_mesh_shape(box, 32 ** 3, padding=0.2)
    assert np.array_equal(box, keep)                                                    # the input is not mutated
    assert all(isinstance(s, int) and s % 2 == 0 and s > 0 for s in shape) and isinstance(cell, float)
    assert cell == pytest.approx(((box * 1.2).prod() / 32 ** 3) ** (1 / 3), rel=1e-15)
    assert shape == tuple(int(2 * np.rint(b * 1.2 / cell / 2)) for b in box)
    assert (shape, cell) == ref.get_mesh_shape(box, 32 ** 3, 0.2)
    shape, cell = bricks.get_mesh_shape((640., 640., 640.), 16 ** 3)
    assert shape == (16, 16, 16) and cell == pytest.approx(40., rel=1e-15)               # (a cube root: the last bit is free)
    assert bricks.get_mesh_shape([100., 200., 300.], 16 ** 3, 0.2)[0] == (8, 18, 26)     # a list or a tuple serves as well


def test_minmax_box():
    from montecosmo_amd import bricks
    pos = np.random.default_rng(0).uniform(-3, 7, (100, 3))
    size, center, rotvec = bricks.minmax_box(pos)
    assert np.array_equal(size, pos.max(0) - pos.min(0)) and np.array_equal(center, (pos.max(0) + pos.min(0)) / 2)
    assert np.array_equal(rotvec, np.zeros(3))


def test_radecrad_round_trip():
    from montecosmo_amd import utils
    rng = np.random.default_rng(1)
    ra = np.concatenate([rng.uniform(0, 360, 50), [0., 360., 0., 123., 180., 359.999999]])
    dec = np.concatenate([rng.uniform(-90, 90, 50), [0., 0., 90., -90., 45., -45.]])
    rad = np.concatenate([rng.uniform(1, 3000, 50), [1., 2., 3., 4., 5., 0.]])
    cart = utils.radecrad2cart(ra, dec, rad)
    assert cart.shape == (56, 3) and np.allclose(cart, ref.radecrad2cart(ra, dec, rad), rtol=0, atol=0)
    assert np.allclose(np.linalg.norm(cart, axis=-1), rad, rtol=1e-14)
    assert np.allclose(cart[52], [0, 0, 3.], atol=1e-15) and np.allclose(cart[53], [0, 0, -4.], atol=1e-15)      # the poles
    assert np.allclose(cart[50], [1., 0, 0], atol=1e-15) and np.allclose(cart[51], [2., 0, 0], atol=1e-15)       # ra = 0 and ra = 360
    ra2, dec2, rad2 = utils.cart2radecrad(cart)
    assert np.all((ra2 >= 0) & (ra2 <= 360)) and np.all(np.abs(dec2) <= 90)      # (-1e-14 % 360 rounds to 360, as in the reference)
    assert np.allclose(rad2, rad, rtol=1e-14) and np.allclose(dec2[:-1], dec[:-1], atol=1e-6)      # (arcsin near the poles: 1e-8 rad)
    assert (ra2[-1], dec2[-1], rad2[-1]) == (0., 0., 0.)                                            # the origin: safe_div
    off_pole = np.abs(dec) < 89.9
    assert np.allclose(((ra2 - ra + 180) % 360 - 180)[off_pole & (rad > 0)], 0, atol=1e-9)          # ra modulo 360 (at a pole it is free)
    assert np.allclose(utils.radecrad2cart(ra2, dec2, rad2), cart, atol=1e-9)                       # and back, poles included


def test_radecz_round_trip():
    from montecosmo_amd import bricks
    cosmo = bricks.Planck18()
    rng = np.random.default_rng(2)
    radecz = {'RA': rng.uniform(0, 360, 40), 'DEC': rng.uniform(-80, 80, 40), 'Z': rng.uniform(0.05, 2., 40)}
    cart = bricks.radecz2cart(cosmo, radecz)
    assert np.allclose(cart, ref.radecz2cart(obg.Planck18(), radecz), rtol=1e-12)
    back = bricks.cart2radecz(cosmo, cart)
    assert all(np.allclose(back[k], radecz[k], rtol=1e-4) for k in radecz)      # two piecewise-linear tables: not exact inverses


def test_header_declares_and_library_exports_the_calls():
    from montecosmo_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcpm.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert raw.mcpm_masked_sum_f64(None, None, None, 0, None) == -6 and raw.mcpm_footprint_u8(None, None, 0, None, 2, None, 0) == -6


def _sky(n=8, **over):
    rng = np.random.default_rng(3)
    d = {'RA': rng.uniform(100, 140, n), 'DEC': rng.uniform(10, 40, n), 'Z': rng.uniform(0.4, 0.7, n), 'WEIGHT': rng.uniform(0.5, 1.5, n)}
    d.update(over)
    return d


def _box(n=8, **over):
    rng = np.random.default_rng(4)
    d = {'pos': rng.uniform(0, 100, (n, 3)), 'vel': rng.standard_normal((n, 3))}
    d.update(over)
    return d


FULL = dict(box_size=(100., 100., 100.), box_center=(0., 0., 0.), a_obs=0.7, los=(0., 0., 1.))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device fails the test: the refusals below come first."""
    from montecosmo_amd import nbody

    def boom():
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(nbody, "_device", boom)


def test_refusals_come_before_device_work(no_device):
    from montecosmo_amd import bricks, model, register
    cosmo = bricks.Planck18()
    rc = register.register_catalog
    for bad in (dict(a_obs=0.7), dict(los=(0., 0., 1.)), dict(a_obs=0.7, los=(0., 0., 1.))):      # cut sky is a light cone on a curved sky
        with pytest.raises(ValueError, match="cut-sky"):
            rc(16 ** 3, cosmo, _sky(), _sky(), **bad)
    for missing in FULL:                                                                          # full sky needs all four
        with pytest.raises(ValueError, match="full-sky"):
            rc(16 ** 3, cosmo, _box(), **{k: v for k, v in FULL.items() if k != missing})
    for w in (-1., np.nan, np.inf):
        bad_w = np.ones(8)
        bad_w[5] = w
        with pytest.raises(ValueError, match="WEIGHT"):
            rc(16 ** 3, cosmo, _sky(), _sky(WEIGHT=bad_w))
        with pytest.raises(ValueError, match="WEIGHT"):
            rc(16 ** 3, cosmo, _sky(WEIGHT=bad_w), _sky())
        with pytest.raises(ValueError, match="WEIGHT"):
            rc(16 ** 3, cosmo, [_sky(), _sky(WEIGHT=bad_w)], (_sky(),))                            # in a later chunk of a list
        with pytest.raises(ValueError, match="WEIGHT"):
            rc(16 ** 3, cosmo, _box(WEIGHT=bad_w), **FULL)
    with pytest.raises(NotImplementedError, match="rectangular"):
        rc(16 ** 3, cosmo, _sky(), _sky(), kernel_type='kaiser_bessel')
    with pytest.raises(NotImplementedError, match="rectangular"):
        rc(16 ** 3, cosmo, _box(), kernel_type='kaiser_bessel', **FULL)
    with pytest.raises(TypeError, match="one-shot"):
        rc(16 ** 3, cosmo, _sky(), (d for d in [_sky()]))                                         # the randoms are read twice
    with pytest.raises(TypeError, match="one-shot"):
        rc(16 ** 3, cosmo, iter([_sky()]), _sky())
    with pytest.raises(TypeError):
        rc(16 ** 3, cosmo, _sky(), [_sky(), 3.])
    with pytest.raises(ValueError, match="chunk"):
        rc(16 ** 3, cosmo, _sky(), _sky(), chunk=0)
    with pytest.raises(KeyError, match="'Z'"):
        rc(16 ** 3, cosmo, _sky(), {k: v for k, v in _sky().items() if k != 'Z'})
    with pytest.raises(ValueError, match="length"):
        rc(16 ** 3, cosmo, _sky(), _sky(Z=np.ones(7)))
    for col in ('RA', 'DEC', 'Z'):                                                                 # a NaN coordinate would slip past fmin / fmax
        bad_c = _sky()[col].copy()
        bad_c[2] = np.nan
        with pytest.raises(ValueError, match=col + " must be finite"):
            rc(16 ** 3, cosmo, _sky(), _sky(**{col: bad_c}))
    with pytest.raises(ValueError, match="vel must have the shape of pos"):
        rc(16 ** 3, cosmo, _box(vel=np.zeros((7, 3))), **FULL)
    with pytest.raises(ValueError, match="vel must have the shape of pos"):
        rc(16 ** 3, cosmo, [_box(), _box(vel=np.zeros(8))], **FULL)
    with pytest.raises(ValueError, match=r"pos must have shape \(N, 3\)"):
        rc(16 ** 3, cosmo, _box(pos=np.zeros((8, 2)), vel=np.zeros((8, 2))), **FULL)
    with pytest.raises(ValueError, match="pos must be finite"):
        rc(16 ** 3, cosmo, _box(pos=np.full((8, 3), np.inf)), **FULL)
    with pytest.raises(ValueError, match="cut-sky"):                                               # the classmethod forwards
        model.FieldLevelForward.register_catalog(16 ** 3, cosmo, _sky(), _sky(), a_obs=0.7)


def test_catalog_tables():
    from montecosmo_amd import bricks
    d = _sky()
    assert bricks.catalog_tables(d) == [d] and bricks.catalog_tables((d, d)) == [d, d]
    rec = np.zeros(4, dtype=[('RA', 'f8'), ('DEC', 'f8'), ('Z', 'f8')])
    assert bricks.catalog_tables(rec)[0] is rec                                                   # a structured array is a table
    gen = (x for x in [d])
    assert bricks.catalog_tables(gen, iterable_ok=True) is gen
    with pytest.raises(TypeError):
        bricks.catalog_tables(gen)


def test_tables_are_checked_once(monkeypatch):
    """checked_tables scans the columns where the catalogue enters; what it returns passes through it again untouched, so the passes
    of register_catalog over one catalogue do not scan it again.  A lazily consumed iterable is checked table by table."""
    from montecosmo_amd import bricks
    calls = []
    check = bricks.check_catalog
    monkeypatch.setattr(bricks, "check_catalog", lambda tables, *a, **k: (calls.append(len(tables)), check(tables, *a, **k))[1])
    tables = bricks.checked_tables([_sky(), _sky(5)], bricks.SKY_KEYS, "random")
    assert calls == [2] and bricks.checked_tables(tables, bricks.SKY_KEYS, "random") is tables and calls == [2]
    assert [len(p['RA']) for p in bricks._pieces(tables, bricks.SKY_KEYS, 3)] == [3, 3, 2, 3, 2] and calls == [2]
    assert bricks.weighted_size(tables) == pytest.approx(sum(t['WEIGHT'].sum() for t in tables), rel=1e-15)
    assert bricks.weighted_size([{'RA': np.zeros(4)}]) == 4.
    lazy = bricks.checked_tables(iter([_box(), _box(vel=np.zeros(3))]), ('pos',), optional=('vel',), iterable_ok=True)
    assert calls == [2] and next(lazy)['pos'].shape == (8, 3) and calls == [2, 1]
    with pytest.raises(ValueError, match="vel"):
        next(lazy)
