"""montecosmo_amd/tables.py on the host (device 'cpu'; the growth and distance integrators are host code of libmcpm.so): every layout against
the order include/mcpm.h states, with its inverse map; what the store's key sees and what it does not; eviction; the upload count; and the
central difference `fd_pair`."""
import numpy as np
import pytest


@pytest.fixture()
def T():
    from montecosmo_amd import tables
    tables._STORE.clear()
    yield tables
    tables._STORE.clear()


def _cosmo(**kw):
    from montecosmo_amd import bricks
    return bricks.Planck18(**{**dict(Omega_c=0.27, w0=-0.95, wa=0.1, Omega_k=0.01), **kw})


def _kpow():
    ks = np.logspace(-3, 1, 64)
    return ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6)


def _expected(layout_name, c, fid, kpow):
    """The concatenation each caller used to spell, in the order of include/mcpm.h."""
    from montecosmo_amd import bricks, nbody, power
    d, g, df = nbody._dist_cache(c), nbody._growth_cache(c), nbody._dist_cache(fid)
    chi, aoc = d["chi"][::-1], d["a"][::-1]
    return {
        # mcpm_observe_pos_f32, mcpm_kaiser_sky_f32: chi ascending [nchi], a(chi) [nchi], a [ngrow], g [ngrow], f [ngrow]
        "LIGHTCONE": [chi, aoc, g["a"], g["g"], g["f"]],
        # mcpm_lightcone_tables_vjp_f32: chi, a(chi), a, g, g2, f, f2
        "LIGHTCONE_VJP": [chi, aoc, g["a"], g["g"], g["g2"], g["f"], g["f2"]],
        # mcpm_observe_pos_ap_f32: chi, a(chi) of the sampled cosmology, then a ascending, chi_fid(a) of the fiducial one
        "AP": [chi, aoc, df["a"], df["chi"]],
        # mcpm_sky2cell_f32, mcpm_sky2cart_minmax_f64: a | chi
        "DISTANCE": [d["a"], d["chi"]],
        # mcpm_interp_f32: xp | fp
        "CHI2A": [chi, aoc],
        "GROWTH": [g["a"], g["g"], g["g2"], g["f"], g["f2"]],
        # mcpm_power_mult_f32: ks | pows;  mcpm_png_*_f32: ks | trans
        "POWER": list(power.lin_power_table(c) if kpow is None else kpow),
        "TRANS": list(bricks.trans_phi2delta_table(c, kpow=kpow)),
    }[layout_name]


LAYOUTS = ("LIGHTCONE", "LIGHTCONE_VJP", "AP", "DISTANCE", "CHI2A", "GROWTH", "POWER", "TRANS")


@pytest.mark.parametrize("with_kpow", [False, True])
@pytest.mark.parametrize("name", LAYOUTS)
def test_layout_and_inverse(T, name, with_kpow):
    c, fid, kpow = _cosmo(), _cosmo(Omega_c=0.22), _kpow() if with_kpow else None
    layout = getattr(T, name)
    want = _expected(name, c, fid, kpow)
    tab = T.on_device(c, layout, "cpu", fid=fid, kpow=kpow)
    assert tab.t.dtype.is_floating_point and tab.t.element_size() == 8 and tab.t.is_contiguous()
    assert np.array_equal(tab.t.numpy(), np.concatenate(want))
    assert [tab.n[k] for k in layout] == [len(w) for w in want]
    host = T.host_tables(c, layout, fid=fid, kpow=kpow)
    for k, w in zip(layout, want):
        assert np.array_equal(tab.v[k].numpy(), w) and np.array_equal(host[k], w)
    # the inverse map: a cotangent over the arrays that move, in the layout's order
    moving = [k for k in layout if k not in T.FIXED]
    vec = np.arange(sum(tab.n[k] for k in moving), dtype=np.float64) + 0.5
    bars = tab.bars(vec)
    assert list(bars) == moving and np.array_equal(np.concatenate([bars[k] for k in moving]), vec)
    assert all(len(bars[k]) == tab.n[k] for k in moving)


def test_moving_arrays_are_the_kernels_cotangents(T):
    """mcpm_lightcone_tables_vjp_f32 writes chi, g, g2, f, f2; the observation side and mcpm_kaiser_sky_tables_vjp_f32 chi, g, f; the
    Alcock-Paczynski look-up at fixed a_obs chi alone; the PNG kernels trans."""
    moving = lambda layout: tuple(k for k in layout if k not in T.FIXED)
    assert moving(T.LIGHTCONE_VJP) == ("chi", "g", "g2", "f", "f2") and moving(T.LIGHTCONE) == ("chi", "g", "f")
    assert moving(T.AP) == ("chi",) and moving(T.TRANS) == ("trans",)


# ---- keying ---------------------------------------------------------------------------------------------------------------------
BACKGROUND = ("Omega_c", "Omega_b", "Omega_k", "w0", "wa")
READS = {"LIGHTCONE": BACKGROUND, "LIGHTCONE_VJP": BACKGROUND, "AP": BACKGROUND, "DISTANCE": BACKGROUND, "CHI2A": BACKGROUND,
         "GROWTH": BACKGROUND, "POWER": ("Omega_c", "Omega_b", "h", "n_s"), "TRANS": BACKGROUND + ("h", "n_s")}
IGNORES = {"LIGHTCONE": ("sigma8", "h", "n_s"), "AP": ("sigma8", "h", "n_s"), "GROWTH": ("sigma8", "h", "n_s"),
           "POWER": ("sigma8", "Omega_k", "w0", "wa"), "TRANS": ("sigma8",)}


def _moved(name):
    c = _cosmo()
    return _cosmo(**{name: getattr(c, name) * 1.01 + 0.003})


def test_equal_values_in_another_object_hit(T):
    fid = _cosmo(Omega_c=0.22)
    for name in LAYOUTS:
        a = T.on_device(_cosmo(), getattr(T, name), "cpu", fid=fid)
        assert T.on_device(_cosmo(), getattr(T, name), "cpu", fid=_cosmo(Omega_c=0.22)) is a


@pytest.mark.parametrize("name,attr", [(n, a) for n in LAYOUTS for a in READS[n]])
def test_an_attribute_the_table_reads_misses(T, name, attr):
    fid, layout = _cosmo(Omega_c=0.22), getattr(T, name)
    a = T.on_device(_cosmo(), layout, "cpu", fid=fid)
    b = T.on_device(_moved(attr), layout, "cpu", fid=fid)
    assert b is not a and not np.array_equal(a.t.numpy(), b.t.numpy())


@pytest.mark.parametrize("attr", BACKGROUND)
def test_the_fiducial_cosmology_is_part_of_the_key(T, attr):
    a = T.on_device(_cosmo(), T.AP, "cpu", fid=_cosmo())
    b = T.on_device(_cosmo(), T.AP, "cpu", fid=_moved(attr))
    assert b is not a and not np.array_equal(a.v["chi_fid"].numpy(), b.v["chi_fid"].numpy()) and np.array_equal(a.v["chi"].numpy(), b.v["chi"].numpy())


@pytest.mark.parametrize("name,attr", [(n, a) for n in IGNORES for a in IGNORES[n]])
def test_an_attribute_the_table_does_not_read_hits(T, name, attr):
    fid, layout = _cosmo(Omega_c=0.22), getattr(T, name)
    assert T.on_device(_moved(attr), layout, "cpu", fid=fid) is T.on_device(_cosmo(), layout, "cpu", fid=fid)


def test_a_given_power_table_replaces_the_cosmology_in_the_key(T):
    kpow = _kpow()
    assert T.on_device(_moved("h"), T.POWER, "cpu", kpow=kpow) is T.on_device(_cosmo(), T.POWER, "cpu", kpow=kpow)
    assert T.on_device(_moved("w0"), T.TRANS, "cpu", kpow=kpow) is not T.on_device(_cosmo(), T.TRANS, "cpu", kpow=kpow)


def test_table_sizes_and_layout_and_device_are_part_of_the_key(T, monkeypatch):
    from montecosmo_amd import nbody
    c = _cosmo()
    a = T.on_device(c, T.CHI2A, "cpu")
    assert T.on_device(c, T.CHI2A, "meta") is not a and T.on_device(c, T.DISTANCE, "cpu") is not a
    for setting in ("growth_steps", "dist_steps", "growth_log10_amin", "dist_log10_amin"):
        with monkeypatch.context() as m:
            m.setattr(nbody, setting, getattr(nbody, setting) + 1)
            assert T.on_device(c, T.CHI2A, "cpu") is not a
    assert T.on_device(c, T.CHI2A, "cpu") is a


@pytest.mark.parametrize("name", ["POWER", "TRANS"])
def test_kpow_counts_by_identity(T, name):
    c, layout = _cosmo(), getattr(T, name)
    k1, k2 = _kpow(), _kpow()
    a = T.on_device(c, layout, "cpu", kpow=k1)
    assert T.on_device(c, layout, "cpu", kpow=k1) is a and T.on_device(c, layout, "cpu", kpow=(k1[0], k1[1])) is a
    assert T.on_device(c, layout, "cpu", kpow=k2) is not a      # equal contents, distinct arrays
    assert T.on_device(c, layout, "cpu", kpow=None) is not a


def test_a_freed_kpow_never_hands_its_table_to_a_new_one(T):
    """The entry keeps the arrays, so their ids cannot be recycled while it is in the store; once it is evicted they can, and nothing is left
    to answer for them."""
    c = _cosmo()
    for i in range(200):      # only the store holds the pairs before this one: a pair it let go of would lend its address to the next
        new = (np.logspace(-3, 1, 64), np.full(64, float(i)))
        tab = T.on_device(c, T.POWER, "cpu", kpow=new)
        assert np.array_equal(tab.v["pows"].numpy(), new[1]) and tab.keep[1] is new[1]
        del new, tab


# ---- eviction, uploads ----------------------------------------------------------------------------------------------------------------
def test_eviction_drops_the_oldest_entry_only(T):
    cosmos = [_cosmo(Omega_c=0.2 + 0.001 * i) for i in range(T.BOUND + 1)]
    held = [T.on_device(c, T.CHI2A, "cpu") for c in cosmos[:T.BOUND]]
    assert len(T._STORE) == T.BOUND
    first = held[0].t.clone()
    T.on_device(cosmos[-1], T.CHI2A, "cpu")
    assert len(T._STORE) == T.BOUND
    assert all(T.on_device(c, T.CHI2A, "cpu") is h for c, h in zip(cosmos[1:T.BOUND], held[1:]))      # still there
    assert np.array_equal(held[0].t.numpy(), first.numpy())      # a caller's table outlives its entry, unchanged
    assert T.on_device(cosmos[0], T.CHI2A, "cpu") is not held[0]      # and the entry is rebuilt, equal
    assert np.array_equal(T.on_device(cosmos[0], T.CHI2A, "cpu").t.numpy(), first.numpy())


def _count_uploads(T, monkeypatch):
    calls, real = [], T.upload
    monkeypatch.setattr(T, "upload", lambda array, device: calls.append(len(array)) or real(array, device))
    return calls


def _lightcone_gradient_requests(T, c, fid):
    """What one gradient asks the store for on the light cone with png_type, ap_auto=True and no lin_kpow, cosmo_vjp's pair included."""
    for layout in (T.POWER, T.CHI2A, T.GROWTH, T.TRANS, T.LIGHTCONE, T.AP,      # evolve
                   T.GROWTH, T.TRANS, T.POWER, T.LIGHTCONE_VJP):                 # evolve_vjp, lightcone_table_bars
        T.on_device(c, layout, "cpu", fid=fid)
    for pm in T.fd_pair(c, "Omega_m", 1e-5)[1]:                                  # the Eisenstein-Hu term of cosmo_vjp
        T.on_device(pm, T.POWER, "cpu")


def test_one_gradient_fits_the_store_and_a_second_uploads_nothing(T, monkeypatch):
    calls = _count_uploads(T, monkeypatch)
    c, fid = _cosmo(), _cosmo(Omega_c=0.22)
    _lightcone_gradient_requests(T, c, fid)
    assert len(T._STORE) == len(calls) == 9 <= T.BOUND
    _lightcone_gradient_requests(T, _cosmo(), _cosmo(Omega_c=0.22))
    assert len(calls) == 9 and len(T._STORE) == 9


# ---- the central difference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rel_eps", [("Omega_m", 1e-5), ("Omega_b", 1e-4), ("w0", 1e-5), ("wa", 1e-3), ("Omega_k", 1e-5)])
def test_fd_pair(T, name, rel_eps):
    from montecosmo_amd import nbody
    c = _cosmo(wa=0.0, Omega_k=0.001) if name in ("wa", "Omega_k") else _cosmo()
    nbody._dist_cache(c)
    before = {k: getattr(c, k) for k in ("Omega_c", "Omega_b", "h", "n_s", "sigma8", "Omega_k", "w0", "wa")}
    h, (p, m) = T.fd_pair(c, name, rel_eps)
    attr = "Omega_c" if name == "Omega_m" else name
    assert h == rel_eps * max(abs(before[attr]), 1e-2)
    assert getattr(p, attr) == before[attr] + h and getattr(m, attr) == before[attr] - h
    for k, v in before.items():
        assert getattr(c, k) == v and (k == attr or getattr(p, k) == getattr(m, k) == v)
    if name == "Omega_m":
        assert p.Omega_b == m.Omega_b == c.Omega_b and p.Omega_m == c.Omega_b + (before["Omega_c"] + h)
    assert p._workspace == {} and m._workspace == {} and len(c._workspace) == 1
    assert p._workspace is not c._workspace and m._workspace is not c._workspace and p._workspace is not m._workspace
