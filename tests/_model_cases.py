"""The feature mixes at which the HIP log density and its gradient are held to tests/_model_f64.py: the factors and their levels, the
constructors' own constraints, the case table, and the host-side set-up of a case (configuration, latents, sample, observation).  Nothing
here imports the library; tests/test_model_f64_host.py checks the table's coverage and the reference's own derivatives,
tests/test_gpu_model_combinations.py runs the table on the device."""
import itertools

import numpy as np

import _model_f64 as M
import _lik_phi_f64 as P
import _png_f64 as pf
from oracle import background as obg

FACTORS = {
    "evo": ("lpt", "lpt_lc", "nbody", "kaiser"),      # lpt at scalar a_obs; lpt on the light cone; nbody (3 steps, scalar a_obs); kaiser on the curved light cone
    "bias_type": ("lagrangian", "eulerian"),
    "png_type": (None, "fNL", "bias"),
    "ap_auto": (None, True, False),
    "lik_type": ("quad_gauss", "shash", "two_quad_gauss", "poisson", "fourier_gauss"),
    "survey": ("none", "survey", "ngbars"),           # survey: selection mesh + mask + two shells; ngbars: sampled per-shell mean densities
    "precond": ("real", "fourier", "kaiser"),
    "s_ep": (False, True),                            # absent; sampled
    "temp": (1., 2.5),
}
DEFAULT = dict(evo="lpt", bias_type="lagrangian", png_type=None, ap_auto=None, lik_type="quad_gauss", survey="none", precond="fourier",
               s_ep=False, temp=1.)


def valid(c):
    """The constructors' own constraints (FieldLevelForward, FieldLevelLogDensity)."""
    if c["evo"] == "kaiser" and (c["ap_auto"] is not None or c["s_ep"]):
        return False      # kaiser takes no ap_auto and no sampled s_ep (it ignores bias_type; nbody has no light cone: no such level)
    if c["lik_type"] == "fourier_gauss" and c["survey"] == "survey":
        return False      # no mask and no selection mesh
    if c["s_ep"] and (c["png_type"] is None or c["lik_type"] not in M.PHI_LIKS):
        return False
    return True


def valid_pairs():
    """Every pair of levels of two different factors that some valid combination contains."""
    names = list(FACTORS)
    pairs = set()
    for levels in itertools.product(*FACTORS.values()):
        c = dict(zip(names, levels))
        if valid(c):
            pairs.update(pairs_of(c))
    return pairs


def pairs_of(c):
    names = list(FACTORS)
    return {((a, c[a]), (b, c[b])) for i, a in enumerate(names) for b in names[i + 1:]}


def n_features(c):
    return sum(c[k] != DEFAULT[k] for k in FACTORS)


def _case(evo, bias_type, png_type, ap_auto, lik_type, survey, precond, s_ep, temp, seed=41, flat=None, h=None):
    """`flat`: the sky (default: flat at scalar a_obs under lpt, where alpha_ap is read; curved otherwise).  `h`: steps in sample space of
    the central differences, by latent, where the default 1e-4 is not small enough (see `steps`)."""
    c = dict(evo=evo, bias_type=bias_type, png_type=png_type, ap_auto=ap_auto, lik_type=lik_type, survey=survey, precond=precond, s_ep=s_ep,
             temp=temp, seed=seed, flat=(evo == "lpt") if flat is None else flat, h=dict(h or {}))
    assert valid(c), c
    return c


# One case per (evolution, likelihood): each of these 20 pairs needs a case of its own, so no pairwise-covering table is shorter.  The other
# factors are laid over that grid so that every valid pair of levels occurs (test_model_f64_host.py enumerates them).
CASES = [
    _case("lpt", "lagrangian", "fNL", True, "quad_gauss", "survey", "fourier", True, 1.0),
    _case("lpt", "lagrangian", "bias", True, "shash", "ngbars", "real", True, 2.5),
    _case("lpt", "eulerian", "bias", False, "two_quad_gauss", "none", "kaiser", True, 1.0),
    _case("lpt", "eulerian", "bias", True, "poisson", "none", "kaiser", False, 1.0),
    _case("lpt", "eulerian", None, None, "fourier_gauss", "none", "real", False, 2.5),
    _case("lpt_lc", "eulerian", None, None, "quad_gauss", "ngbars", "real", False, 1.0),
    _case("lpt_lc", "eulerian", "fNL", False, "shash", "survey", "fourier", False, 1.0),
    _case("lpt_lc", "eulerian", "bias", True, "two_quad_gauss", "survey", "kaiser", True, 2.5),      # required: the most cotangent paths under lpt
    _case("lpt_lc", "eulerian", None, True, "poisson", "ngbars", "fourier", False, 1.0),
    _case("lpt_lc", "lagrangian", "fNL", False, "fourier_gauss", "none", "real", False, 2.5),
    _case("nbody", "eulerian", "bias", False, "quad_gauss", "none", "kaiser", False, 2.5),
    _case("nbody", "lagrangian", "fNL", False, "shash", "ngbars", "kaiser", True, 2.5, flat=True),   # required; flat sky: alpha_ap is read
    _case("nbody", "eulerian", "fNL", None, "two_quad_gauss", "survey", "real", True, 2.5, seed=43),     # (41: a kink of the log density 3e-6 away along the field direction)
    _case("nbody", "lagrangian", None, False, "poisson", "survey", "fourier", False, 1.0, h=dict(Omega_m=1e-4)),     # (d/d Omega_m_ is 1e-3 here:
    _case("nbody", "lagrangian", "bias", True, "fourier_gauss", "ngbars", "kaiser", False, 2.5),
    _case("kaiser", "eulerian", None, None, "quad_gauss", "survey", "kaiser", False, 2.5, h=dict(Omega_m=1e-4)),    # the curvature shows at 1e-3)
    _case("kaiser", "lagrangian", None, None, "shash", "none", "fourier", False, 2.5),
    _case("kaiser", "lagrangian", None, None, "two_quad_gauss", "ngbars", "fourier", False, 2.5),
    _case("kaiser", "eulerian", "fNL", None, "poisson", "survey", "real", False, 2.5, seed=46),      # (a seed at which every mean count is positive)
    _case("kaiser", "eulerian", "bias", None, "fourier_gauss", "ngbars", "fourier", False, 1.0),
]


def case_id(c):
    return "-".join(str(c[k]) for k in FACTORS)


_KPOW = None


def kpow():
    global _KPOW
    if _KPOW is None:
        ks = np.logspace(-3, 1, 128)
        _KPOW = (ks, 3.0e4 * (ks / 0.02) / (1 + (ks / 0.02) ** 2.6))
    return _KPOW


FINAL, CELL = (8, 8, 8), 40.
A_OBS = {"lpt": 0.65, "lpt_lc": None, "nbody": 0.7, "kaiser": None}
OM_FID = 0.27      # Omega_m of the cosmology the catalogue was gridded with (ap_auto = True); the sampled one is near 0.31
S_EP_FID = 3e3     # phi ~ 2e-5 on this mesh: s_ep phi reaches 0.1 beside s_e = 1
TN = lambda loc, sf, scale=0.1: dict(loc=loc, scale=scale, loc_fid=loc, scale_fid=sf, low=0., high=np.inf)
N = lambda loc, sf, scale=1e2: dict(loc=loc, scale=scale, loc_fid=loc, scale_fid=sf)


def forward_kwargs(c):
    """Keyword arguments of FieldLevelForward (without cosmo_fid, which is the library's or the oracle's own object)."""
    return dict(final_shape=FINAL, cell_length=CELL, box_center=(60., -40., 1400.), box_rotvec=(0.1, 0.2, -0.1),
                evolution=c["evo"].split("_")[0], nbody_n_steps=3, lpt_order=2, init_oversamp=1.5, evol_oversamp=2., ptcl_oversamp=2.,
                paint_oversamp=2., a_obs=A_OBS[c["evo"]], curved_sky=not c["flat"], lin_kpow=kpow(), nbody_a_start=0.1,
                png_type=c["png_type"], ap_auto=c["ap_auto"], bias_type=c["bias_type"])


def config(c):
    """What FieldLevelForward.config() returns for `forward_kwargs(c)` (the device test compares the two), with the entries the oracle's
    log density reads besides."""
    kw = forward_kwargs(c)
    cfg = dict(init_shape=(12, 12, 12), evol_shape=(16, 16, 16), ptcl_shape=(16, 16, 16), paint_shape=(16, 16, 16),
               box_size=np.multiply(FINAL, CELL), box_center=np.asarray(kw["box_center"]), box_rotvec=np.asarray(kw["box_rotvec"]),
               a_obs=kw["a_obs"], curved_sky=kw["curved_sky"], evolution=kw["evolution"], nbody_a_start=0.1, nbody_n_steps=3, lpt_order=2,
               paint_order=2, paint_deconv=True, interlace_order=2, lin_kpow=kpow(), bias_type=c["bias_type"])
    return dict(cfg, final_shape=FINAL, cell_length=CELL, precond=c["precond"])


class _Cosmology(obg.Cosmology):
    """The oracle's cosmology with look-up tables that outlive the `_workspace = {}` of evolve and are shared by every object of equal
    parameters: the tables are functions of those parameters alone, so the numbers are the same and most evaluations of a case's
    central differences, which leave the cosmology where it is, solve no growth or distance equation again."""
    _TABLES = {}

    @property
    def _workspace(self):
        if len(self._TABLES) > 64:
            self._TABLES.clear()
        return self._TABLES.setdefault((self.Omega_c, self.Omega_b, self.h, self.n_s, self.Omega_k, self.w0, self.wa), {})

    @_workspace.setter
    def _workspace(self, value):
        pass


def _planck(Omega_m):
    p = obg.Planck18(Omega_c=Omega_m - 0.0490)
    return _Cosmology(Omega_c=p.Omega_c, Omega_b=p.Omega_b, h=p.h, n_s=p.n_s, sigma8=p.sigma8, Omega_k=p.Omega_k, w0=p.w0, wa=p.wa)


def make_cosmo(base):
    c = _planck(base["Omega_m"])
    c.sigma8 = base["sigma8"]
    c.png_params = {k: base.get(k, 0.) for k in pf.PNG_KEYS}
    return c


def cosmo_fid_oracle():
    return _planck(OM_FID)


def steps(c, lat):
    """Step of the central difference of each latent and of the white-mesh direction, in sample space; tests/test_model_f64_host.py holds
    every one of them to its own half.  Two things bound a step.  From below: the oracle's prior of a truncated latent differentiates
    std2trunc by a difference of its own (1e-6), which leaves rounding of 1e-16 value / (scale_fid 1e-6) in the log density -- 4e-9 for
    sigma8, 2e-9 for Omega_m, 5e-9 for ngbars and the alphas -- so those take 1e-3 where nothing else forbids it.  From above: Alcock-Paczynski dilates the
    whole particle set -- 52 cells per unit alpha, 26 per unit Omega_m (ap_auto = True) -- under a paint that is piecewise linear in the
    positions, so those differences are the derivative only for steps that move no noticeable share of the particles across a cell
    boundary (tests/test_gpu_ap_model.py): 1e-5.  alpha_ap is not read on the curved sky: only its smooth prior moves, 1e-2."""
    h = {k: 1e-4 for k in lat}
    h.update(white_mesh=3e-5, sigma8=1e-3, Omega_m=1e-3)
    if "ngbars" in lat:
        h.update(ngbars=1e-3)
    if c["ap_auto"] is False:
        h.update(alpha_iso=1e-5, alpha_ap=1e-5 if c["flat"] else 1e-2)
    if c["ap_auto"] is True:
        h.update(Omega_m=1e-5)
    h.update(c["h"])
    return h


_BUILT = {}


def build(c):
    """Host set-up of a case, computed once: cfg, latents, fixed, sample, obs (drawn from the reference's own likelihood at a nearby
    truth), the keyword arguments of both log densities, and `ref(sample, info=None)`, the float64 log density."""
    key = case_id(c)
    if key in _BUILT:
        return _BUILT[key]
    rng = np.random.default_rng(c["seed"])
    cfg = config(c)
    lik, png_type = c["lik_type"], c["png_type"]
    lat = {"Omega_m": dict(loc=0.3111, scale=0.1, loc_fid=0.3111, scale_fid=1e-2, low=0.05, high=1.), "sigma8": TN(0.8102, 1e-2),
           "b1": N(1., 1e-2)}
    fixed = dict(b2=0.2, bs2=-0.15, bn2=20., bnpar=5., b3=0.1, bds2=0.1, bs3=-0.05, ngbars=1e-3)
    if lik in M.PHI_LIKS:
        lat["s_ed"] = N(0.3, 1e-2, 1e1)
        fixed.update(s_e=1.0, s_e2=0.03)
    elif lik == "fourier_gauss":
        lat["s_k2e"] = N(10., 1.)
        fixed.update(s_e=1.0, s_kmu2e=10.)
    if png_type is not None:
        lat["fNL"] = dict(loc=0., scale=1e3, loc_fid=200., scale_fid=50.)
        fixed.update(fNL_bpd2=-20., fNL_bps2=30., fNL_bn2p=2.0e3)
        if png_type == "bias":
            lat["fNL_bp"] = N(3., 0.5)
            fixed.update(fNL_bpd=-1.)
    if c["s_ep"]:
        lat["s_ep"] = dict(loc=0., scale=1e5, loc_fid=S_EP_FID, scale_fid=1e3)
    if c["ap_auto"] is False:
        lat["alpha_iso"], lat["alpha_ap"] = TN(1., 1e-2), TN(1., 1e-2)
    extra = {}
    if c["survey"] == "survey":
        g = np.indices(cfg["paint_shape"]).astype(float)
        extra["selec_mesh"] = 0.7 + 0.3 * np.cos(2 * np.pi * g[0] / 16) * np.sin(2 * np.pi * g[2] / 16) + 0.1 * rng.uniform(size=cfg["paint_shape"])
        extra["mask_mesh"] = rng.uniform(size=FINAL) < 0.8
        fixed["ngbars"] = np.array([1e-3, 1.4e-3])
    elif c["survey"] == "ngbars":
        fixed.pop("ngbars")
        lat["ngbars"] = dict(loc=np.array([1e-3, 1.4e-3]), scale=1e-2, loc_fid=np.array([1e-3, 1.4e-3]), scale_fid=1e-5, low=0., high=np.inf)
        extra["n_rbins"] = 2
    cfg.update(extra)
    sample = {k + "_": (float(rng.normal(0, 1.0)) if k != "ngbars" else rng.normal(0, 1.0, 2)) for k in lat}
    sample["white_mesh_"] = rng.standard_normal(cfg["init_shape"])
    kw = dict(lik_type=lik, png_type=png_type, bias_type=c["bias_type"], ap_auto=c["ap_auto"],
              cosmo_fid=cosmo_fid_oracle() if c["ap_auto"] else None)
    log_density = lambda s, obs, temp=c["temp"], info=None: M.log_density(cfg, lat, fixed, s, obs, make_cosmo, temp=temp, info=info, **kw)
    # the observation: a draw from the likelihood itself (the scales at temp = 1) at a truth whose field is 0.98 of the sample's plus 0.2 of another
    truth = dict(sample, white_mesh_=0.98 * sample["white_mesh_"] + 0.2 * rng.standard_normal(cfg["init_shape"]))
    info = {}
    log_density(truth, np.zeros(FINAL), temp=1., info=info)
    cm, base = info["count"], info["base"]
    if lik == "poisson":
        obs = rng.poisson(np.abs(cm) ** (1. / c["temp"])).astype(np.float64)      # (the tempered rate: the counts the case's own likelihood expects)
    elif lik == "fourier_gauss":
        obs = cm + np.mean(info["selec"]) ** .5 * rng.standard_normal(FINAL)
    else:
        sc = P.scales(cm, info["selec"], info["phi"], base["s_e"], base["s_ed"], base["s_e2"], base.get("s_ep", 0.), 1.)
        e1 = rng.standard_normal(FINAL)
        e2 = rng.standard_normal(FINAL) if lik == "two_quad_gauss" else e1
        obs = cm + sc["b"] * e1 + sc["a"] * (e2 ** 2 - 1.)
    out = dict(case=c, cfg=cfg, lat=lat, fixed=fixed, sample=sample, obs=obs, extra=extra, rng=rng, h=steps(c, lat),
               direction=rng.standard_normal(cfg["init_shape"]), ref=lambda s, info=None: log_density(s, obs, info=info))
    _BUILT[key] = out
    return out


def scalar_names(b):
    """(latent, index or None) of every sampled scalar of a built case."""
    out = []
    for k in b["lat"]:
        out += [(k, 0), (k, 1)] if k == "ngbars" else [(k, None)]
    return out


def shifted(sample, name, idx, dx):
    k = name + "_"
    if idx is None:
        return dict(sample, **{k: sample[k] + dx})
    return dict(sample, **{k: sample[k] + dx * np.eye(len(sample[k]))[idx]})


def central_difference(b, name, idx, h):
    """Of the reference log density along one scalar, or (name 'white_mesh') along the case's white-mesh direction."""
    if name == "white_mesh":
        s, d = b["sample"], b["direction"]
        return (b["ref"](dict(s, white_mesh_=s["white_mesh_"] + h * d)) - b["ref"](dict(s, white_mesh_=s["white_mesh_"] - h * d))) / (2 * h)
    return (b["ref"](shifted(b["sample"], name, idx, h)) - b["ref"](shifted(b["sample"], name, idx, -h))) / (2 * h)
