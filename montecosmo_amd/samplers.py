"""Host sampler loop for the field-level log density (the role of montecosmo/samplers.py:17-269, which drives blackjax
NUTS): a from-scratch multinomial No-U-Turn sampler (Hoffman & Gelman 2014; Betancourt 2017) with dual-averaging
step-size adaptation, operating on one flat tensor (device or host) and a callable returning (log density, gradient).
Third-party algorithm: what is montecosmo's is the call contract `logdensity_fn(position) -> scalar`, kept here as
`logdensity_and_grad(q) -> (float, tensor)`.  Warm-up follows `blackjax.window_adaptation` (samplers.py:44: Stan's windowed
scheme): dual averaging of the step size throughout, and a DIAGONAL mass matrix estimated over doubling slow windows
(`adapt_mass=True`, the default; identity metric otherwise -- the model's sample space is already roughly standardised by
`scale_fid` and the 'kaiser' preconditioning, so the estimate mostly corrects the scalar latents).  MCLMC tunes its step
size to the energy-error target and, in the second half of the warm-up, L from the running variances of the position
(`mclmc_find_L_and_step_size` as the reference calls it, samplers.py:322-331: frac_tune1 = frac_tune2 = 0.5, no
ESS-based third stage)."""
from __future__ import annotations

import math
import time

import torch


class DualAveraging:
    """Nesterov dual averaging of log(step size) towards a target acceptance statistic (Hoffman & Gelman 2014, alg. 5)."""

    def __init__(self, eps0, target=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        self.mu = math.log(10.0 * eps0)
        self.target, self.gamma, self.t0, self.kappa = target, gamma, t0, kappa
        self.hbar, self.log_eps_bar, self.t = 0.0, 0.0, 0
        self.eps = eps0

    def update(self, accept_stat):
        self.t += 1
        eta = 1.0 / (self.t + self.t0)
        self.hbar = (1 - eta) * self.hbar + eta * (self.target - accept_stat)
        log_eps = self.mu - math.sqrt(self.t) / self.gamma * self.hbar
        w = self.t ** (-self.kappa)
        self.log_eps_bar = w * log_eps + (1 - w) * self.log_eps_bar
        self.eps = math.exp(log_eps)
        return self.eps

    def final(self):
        return math.exp(self.log_eps_bar)


class _State:
    __slots__ = ("q", "p", "lp", "g")

    def __init__(self, q, p, lp, g):
        self.q, self.p, self.lp, self.g = q, p, lp, g


def _leapfrog(fn, s, eps, minv=None):
    p = s.p + (0.5 * eps) * s.g
    q = s.q + eps * (p if minv is None else minv * p)
    lp, g = fn(q)
    p = p + (0.5 * eps) * g
    return _State(q, p, lp, g)


def _energy(s, minv=None):
    return -s.lp + 0.5 * float(torch.dot(s.p, s.p) if minv is None else torch.dot(s.p, minv * s.p))


def _logaddexp(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def _build_tree(fn, edge, direction, depth, eps, H0, rng, max_delta=1000.0, minv=None):
    """Recursively doubles from `edge` in `direction`.  Returns (new edge, proposal, log_w, rho, n_leapfrog,
    sum_accept, diverging, turning) where log_w = log sum exp(-H) over the subtree and rho its summed momentum."""
    if depth == 0:
        s = _leapfrog(fn, edge, direction * eps, minv)
        H = _energy(s, minv)
        if not math.isfinite(H):
            H = math.inf
        diverging = (H - H0) > max_delta
        acc = min(1.0, math.exp(min(0.0, H0 - H))) if math.isfinite(H) else 0.0
        return s, s, (-H if math.isfinite(H) else -math.inf), s.p.clone(), 1, acc, diverging, False, s
    e1, prop1, lw1, rho1, n1, a1, div1, turn1, first1 = _build_tree(fn, edge, direction, depth - 1, eps, H0, rng, max_delta, minv)
    if div1 or turn1:
        return e1, prop1, lw1, rho1, n1, a1, div1, turn1, first1
    e2, prop2, lw2, rho2, n2, a2, div2, turn2, _ = _build_tree(fn, e1, direction, depth - 1, eps, H0, rng, max_delta, minv)
    lw = _logaddexp(lw1, lw2)
    prop = prop1
    if not (div2 or turn2) and lw2 > -math.inf:
        if math.log(max(rng.random(), 1e-300)) < lw2 - lw:      # multinomial sampling within the subtree
            prop = prop2
    rho = rho1 + rho2
    # generalised no-U-turn criterion between the two ends of this subtree (p_sharp = M^-1 p)
    p_first, p_last = first1.p, e2.p
    if direction < 0:
        p_first, p_last = p_last, p_first
    rs = rho if minv is None else minv * rho
    turning = turn2 or (float(torch.dot(rs, p_first)) <= 0.0) or (float(torch.dot(rs, p_last)) <= 0.0)
    return e2, prop, lw, rho, n1 + n2, a1 + a2, div2, turning, first1


def nuts_step(fn, q, lp, g, eps, rng, max_tree_depth=10, minv=None):
    """One NUTS transition; `minv`: diagonal inverse mass matrix (None = identity).  Returns (q, lp, g, info)."""
    p0 = torch.randn(q.shape, dtype=q.dtype, device=q.device, generator=rng.torch_gen(q.device))
    if minv is not None:
        p0 = p0 / torch.sqrt(minv)                      # p ~ N(0, M)
    start = _State(q, p0, lp, g)
    H0 = _energy(start, minv)
    left = right = start
    sample = start
    log_w = -H0
    rho = p0.clone()
    n_leap, sum_acc, depth, diverging = 0, 0.0, 0, False
    while depth < max_tree_depth:
        direction = 1 if rng.random() < 0.5 else -1
        edge = right if direction > 0 else left
        new_edge, prop, lw_sub, rho_sub, n, acc, div, turn, _ = _build_tree(fn, edge, direction, depth, eps, H0, rng, minv=minv)
        n_leap += n
        sum_acc += acc
        if div:
            diverging = True
            break
        if turn:
            break
        if lw_sub > -math.inf and math.log(max(rng.random(), 1e-300)) < lw_sub - log_w:   # biased progressive sampling
            sample = prop
        log_w = _logaddexp(log_w, lw_sub)
        rho = rho + rho_sub
        if direction > 0:
            right = new_edge
        else:
            left = new_edge
        depth += 1
        rs = rho if minv is None else minv * rho
        if float(torch.dot(rs, left.p)) <= 0.0 or float(torch.dot(rs, right.p)) <= 0.0:
            break
    info = {"n_leapfrog": n_leap, "accept_stat": sum_acc / max(n_leap, 1), "depth": depth, "diverging": diverging,
            "energy": H0}
    return sample.q, sample.lp, sample.g, info


class _Rng:
    def __init__(self, seed):
        import random
        self._r = random.Random(seed)
        self._seed = seed
        self._gens = {}

    def random(self):
        return self._r.random()

    def torch_gen(self, device):
        key = str(device)
        if key not in self._gens:
            g = torch.Generator(device=device)
            g.manual_seed(self._seed + 12345)
            self._gens[key] = g
        return self._gens[key]

    def get_state(self):
        """Everything needed to continue the streams exactly (a chain resumed from a saved state repeats the draws an
        uninterrupted chain would have made)."""
        return {"seed": self._seed, "py": self._r.getstate(), "gens": {k: g.get_state() for k, g in self._gens.items()}}

    @classmethod
    def from_state(cls, st):
        r = cls(st["seed"])
        r._r.setstate(st["py"])
        for k, gs in st["gens"].items():
            r.torch_gen(torch.device(k)).set_state(gs)
        return r


def find_reasonable_step_size(fn, q, lp, g, rng, eps=1.0, minv=None):
    """Heuristic of Hoffman & Gelman 2014, alg. 4: double / halve until the one-step acceptance crosses 1/2."""
    p = torch.randn(q.shape, dtype=q.dtype, device=q.device, generator=rng.torch_gen(q.device))
    if minv is not None:
        p = p / torch.sqrt(minv)
    s0 = _State(q, p, lp, g)
    H0 = _energy(s0, minv)
    s1 = _leapfrog(fn, s0, eps, minv)
    dH = H0 - _energy(s1, minv)
    direction = 1.0 if (math.isfinite(dH) and dH > math.log(0.5)) else -1.0
    for _ in range(50):
        eps *= 2.0 ** direction
        s1 = _leapfrog(fn, s0, eps, minv)
        dH = H0 - _energy(s1, minv)
        ok = math.isfinite(dH) and dH > math.log(0.5)
        if (direction > 0 and not ok) or (direction < 0 and ok):
            break
    return eps


def warmup_windows(n_warmup, init_buffer=75, term_buffer=50, base_window=25):
    """Stan's warm-up schedule (what `blackjax.window_adaptation` builds): [fast initial buffer | slow windows, each twice the
    last, the final one stretched to the terminal buffer | fast terminal buffer].  Returns the list of (start, end) of the slow
    windows (the mass matrix is re-estimated at every `end`); short warm-ups use the 15 % / 75 % / 10 % split."""
    if n_warmup < 20:
        return []
    if init_buffer + base_window + term_buffer > n_warmup:
        init_buffer, term_buffer = int(0.15 * n_warmup), int(0.10 * n_warmup)
        base_window = n_warmup - init_buffer - term_buffer
    wins, start, size, slow_end = [], init_buffer, base_window, n_warmup - term_buffer
    while start < slow_end:
        end = start + size
        if end + 2 * size > slow_end:          # the next window would not fit: this one runs to the terminal buffer
            end = slow_end
        wins.append((start, end))
        start, size = end, 2 * size
    return wins


class _Welford:
    """Running mean / variance of the chain's positions on their own device (two vectors, whatever the dimension)."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, None, None

    def add(self, q):
        q = q.double()
        if self.mean is None:
            self.mean, self.m2 = torch.zeros_like(q), torch.zeros_like(q)
        self.n += 1
        d = q - self.mean
        self.mean += d / self.n
        self.m2 += d * (q - self.mean)

    def inverse_mass(self, dtype):
        """Stan's regularised variance estimate: (n / (n + 5)) var + 1e-3 (5 / (n + 5))."""
        var = self.m2 / max(self.n - 1, 1)
        return ((self.n / (self.n + 5.0)) * var + 1e-3 * (5.0 / (self.n + 5.0))).to(dtype)


def nuts_sample(logdensity_and_grad, q0, n_warmup=200, n_samples=200, max_tree_depth=10, target_accept=0.8, seed=0,
                step_size=None, callback=None, keep=None, state=None, adapt_mass=True, inverse_mass=None):
    """Runs warm-up (step-size adaptation by dual averaging) then sampling.  `logdensity_and_grad(q) -> (float, tensor)`.
    `keep(q)` maps a state to what is stored per draw (default: the state itself; pass a reducer for 10^7-dimensional
    states).  Returns dict(samples=[...], step_size, infos=[...], seconds, last_state).  `state` (a previous call's
    `last_state`, see `save_run` / `load_state`) continues that chain: position, step size and random streams are taken
    from it (q0, seed and step_size are ignored; pass n_warmup=0 to keep the adapted step size, as the reference does
    with `post_warmup_state`, samplers.py:618-660)."""
    if state is not None:
        rng = _Rng.from_state(state["rng"])
        q = state["q"].clone().to(q0.device if q0 is not None else state["q"].device)
        step_size = state["step_size"]
    else:
        rng = _Rng(seed)
        q = q0.clone()
    minv = inverse_mass
    if state is not None and state.get("inverse_mass") is not None:
        minv = state["inverse_mass"].to(q.device)
    lp, g = logdensity_and_grad(q)
    eps = step_size if step_size is not None else find_reasonable_step_size(logdensity_and_grad, q, lp, g, rng, minv=minv)
    da = DualAveraging(eps, target=target_accept)
    wins = warmup_windows(n_warmup) if adapt_mass else []
    win_end = {e: s_ for s_, e in wins}
    wf = _Welford()
    infos, samples = [], []
    t0 = time.perf_counter()
    for it in range(n_warmup + n_samples):
        warm = it < n_warmup
        q, lp, g, info = nuts_step(logdensity_and_grad, q, lp, g, eps, rng, max_tree_depth, minv)
        if warm:
            eps = da.update(info["accept_stat"])
            if wins and wins[0][0] <= it < wins[-1][1]:
                wf.add(q)
            if (it + 1) in win_end and wf.n > 1:
                # end of a slow window: new metric from this window's draws, step size re-initialised and its averaging
                # restarted (window_adaptation does the same)
                minv = wf.inverse_mass(q.dtype)
                wf = _Welford()
                eps = find_reasonable_step_size(logdensity_and_grad, q, lp, g, rng, eps=da.final(), minv=minv)
                da = DualAveraging(eps, target=target_accept)
            if it == n_warmup - 1:
                eps = da.final()
        else:
            samples.append(keep(q) if keep is not None else q.clone())
        info.update(step_size=eps, warmup=warm, logdensity=lp)
        infos.append(info)
        if callback is not None:
            callback(it, info)
    return {"samples": samples, "step_size": eps, "inverse_mass": minv, "infos": infos, "seconds": time.perf_counter() - t0,
            "last_state": {"sampler": "nuts", "q": q.clone(), "step_size": eps, "rng": rng.get_state(),
                           "inverse_mass": None if minv is None else minv.clone()}}


# ---- chains on disk (montecosmo/samplers.py:596-660: one .npz of draws per run + the last state, overwritten) ----
def save_run(result, i_run, path, extra_fields=("n_evals", "accept_stat", "step_size", "logdensity", "diverging")):
    """Writes `path_{i_run}.npz` (the kept draws stacked as 'samples' + the requested per-transition fields; n_evals is
    the number of gradient evaluations, the reference's renamed `num_steps`) and overwrites `path_last_state.pt`."""
    import numpy as np
    infos = result["infos"]
    out = {}
    draws = result["samples"]
    if len(draws):
        out["samples"] = np.stack([np.asarray(d.detach().cpu()) if isinstance(d, torch.Tensor) else np.asarray(d) for d in draws])
    for f in extra_fields:
        key = "n_leapfrog" if (f == "n_evals" and infos and "n_evals" not in infos[0]) else f
        if infos and key in infos[0]:
            out[f] = np.asarray([i[key] for i in infos])
    out["warmup"] = np.asarray([bool(i["warmup"]) for i in infos])
    np.savez(f"{path}_{i_run}.npz", **out)
    st = dict(result["last_state"])
    st["q"] = st["q"].detach().cpu()
    if "u" in st:
        st["u"] = st["u"].detach().cpu()
    if st.get("inverse_mass") is not None:
        st["inverse_mass"] = st["inverse_mass"].detach().cpu()
    torch.save(st, f"{path}_last_state.pt")


def load_state(path, device=None):
    """The state `save_run` left at `path_last_state.pt`, on `device`."""
    st = torch.load(f"{path}_last_state.pt", weights_only=False)
    if device is not None:
        st["q"] = st["q"].to(device)
        if "u" in st:
            st["u"] = st["u"].to(device)
    return st


def sample_and_save(sampler, logdensity_and_grad, q0, path, start=0, end=1, n_warmup=200, n_samples=200, resume=False, **kw):
    """Run `start` = warm-up (+ its draws), runs start+1..end = `n_samples` draws each, every run saved with `save_run`
    (samplers.py:618-660).  `sampler` is nuts_sample or mclmc_sample.  resume=True continues from `path_last_state.pt`
    without warm-up."""
    import os
    state = None
    if resume and os.path.exists(f"{path}_last_state.pt"):
        state = load_state(path, q0.device if q0 is not None else None)
    res = None
    for i_run in range(start, end + 1):
        warm = n_warmup if (state is None) else 0
        res = sampler(logdensity_and_grad, q0, n_warmup=warm, n_samples=n_samples, state=state, **kw)
        save_run(res, i_run, path)
        state = res["last_state"]
    return res


# ---- packing the model's parameter dict into one flat vector -----------------------------------------------------
class FlatLogDensity:
    """Adapts `FieldLevelLogDensity` (dict of scalars + 'white_mesh_') to the flat-vector contract of `nuts_sample`:
    q = [scalars in ld.names() order ..., white_mesh_.ravel()] as one float32 device tensor."""

    def __init__(self, ld):
        self.ld = ld
        self.scalars = [n for n in ld.names() if n != "white_mesh_"]
        # 'ngbars_' is one value per radial shell (model.py:1099-1103); every other scalar latent is one number
        self.sizes = [getattr(ld, "n_rbins", 1) if n == "ngbars_" else 1 for n in self.scalars]
        self.ns = int(sum(self.sizes))
        self.shape = tuple(ld.fwd.init_shape)
        self.n_eval = 0

    def pack(self, sample):
        from . import nbody
        import numpy as np
        w = nbody._f32(sample["white_mesh_"], self.shape).reshape(-1)
        vals = np.concatenate([np.atleast_1d(np.asarray(sample[n], dtype=np.float64)).reshape(-1) for n in self.scalars]) \
            if self.scalars else np.zeros(0)
        return torch.cat([torch.tensor(vals, dtype=torch.float32, device=w.device), w])

    def layout(self):
        """name -> (start, stop, shape) of every latent in the flat vector (what `unpack` slices): chains.Chains.from_flat takes it."""
        out, k = {}, 0
        for n, sz in zip(self.scalars, self.sizes):
            out[n] = (k, k + sz, (sz,) if n == "ngbars_" else ())
            k += sz
        out["white_mesh_"] = (k, k + int(math.prod(self.shape)), self.shape)
        return out

    def unpack(self, q):
        vals = q[:self.ns].tolist()
        out, k = {}, 0
        for n, sz in zip(self.scalars, self.sizes):
            out[n] = vals[k] if n != "ngbars_" else vals[k:k + sz]
            k += sz
        out["white_mesh_"] = q[self.ns:].reshape(self.shape)
        return out

    def __call__(self, q):
        import numpy as np
        self.n_eval += 1
        lp, grad = self.ld.logdensity_and_grad(self.unpack(q))
        if math.isnan(lp):      # never a legitimate value: a silent -inf would freeze the chain at its current state
            raise FloatingPointError("log density is NaN at this state (non-finite inputs to the likelihood?)")
        if not math.isfinite(lp):      # outside the support (QuadGaussian's is bounded, utils.py:476-477): rejected, and counted
            self.n_nonfinite = getattr(self, "n_nonfinite", 0) + 1
            return -math.inf, torch.zeros_like(q)
        gs = np.concatenate([np.atleast_1d(np.asarray(grad[n], dtype=np.float64)).reshape(-1) for n in self.scalars]) \
            if self.scalars else np.zeros(0)
        g = torch.cat([torch.tensor(gs, dtype=torch.float32, device=q.device), grad["white_mesh_"].reshape(-1)])
        return lp, g


# ------------------------------------------------------------------------------------------------------------------
# MCLMC: microcanonical Langevin Monte Carlo (Robnik, De Luca, Silverstein & Seljak 2023), the sampler the reference's
# production drivers run through blackjax (montecosmo/samplers.py:273-398: isokinetic McLachlan integrator, step size
# tuned to an energy-error variance per dimension of 5e-4, L initialised at sqrt(d)).  From scratch, identity metric.
_MCLACHLAN = 0.1931833275037836


def _mclmc_B(u, g, eps, d):
    """Isokinetic velocity update for the gradient g of the LOG density (force direction e = g / |g|).  Returns the new
    unit velocity and the kinetic energy change (d - 1) log(cosh delta + e.u sinh delta)."""
    gn = float(torch.linalg.vector_norm(g))
    if gn == 0.0:
        return u, 0.0
    e = g / gn
    delta = eps * gn / (d - 1)
    ue = float(torch.dot(u, e))
    if delta > 30.0:       # sinh / cosh overflow: the update saturates at u -> e
        return e.clone(), (d - 1) * (delta + math.log(0.5 * (1.0 + ue) + 1e-300))
    sh, ch = math.sinh(delta), math.cosh(delta)
    un = (u + e * (sh + ue * (ch - 1.0))) / (ch + ue * sh)
    return un / torch.linalg.vector_norm(un), (d - 1) * math.log(ch + ue * sh)


def mclmc_step(fn, q, lp, g, u, eps, L, rng):
    """One MCLMC transition (McLachlan minimal-norm splitting + partial velocity refreshment).
    Returns (q, lp, g, u, energy_change)."""
    d = q.numel()
    lam = _MCLACHLAN
    u, k1 = _mclmc_B(u, g, lam * eps, d)
    q = q + (0.5 * eps) * u
    lp1, g1 = fn(q)
    u, k2 = _mclmc_B(u, g1, (1 - 2 * lam) * eps, d)
    q = q + (0.5 * eps) * u
    lp2, g2 = fn(q)
    u, k3 = _mclmc_B(u, g2, lam * eps, d)
    dE = (k1 + k2 + k3) - (lp2 - lp)           # kinetic + potential (V = -log p) change
    nu = math.sqrt((math.exp(2.0 * eps / L) - 1.0) / d)
    z = torch.randn(q.shape, dtype=q.dtype, device=q.device, generator=rng.torch_gen(q.device))
    u = u + nu * z
    u = u / torch.linalg.vector_norm(u)
    return q, lp2, g2, u, dE


def mclmc_sample(logdensity_and_grad, q0, n_warmup=200, n_samples=200, desired_energy_var=5e-4, L=None, step_size=None,
                 seed=0, callback=None, keep=None, state=None, tune_L=True):
    """Warm-up (the two stages of `blackjax.mclmc_find_L_and_step_size` the reference runs, samplers.py:322-331, each half of
    `n_warmup`): throughout, the step size is driven to an energy-error variance per dimension of `desired_energy_var`
    (E[dE^2] / d = C eps^6 for this second-order splitting: C is a down-weighted running average, eps = C^(-1/6)); in the
    second half the same weights also average x and x^2, and at its end L = sqrt(sum_i Var(x_i)) (the size of the typical set;
    `tune_L=False` or an explicit `L` keep L, default sqrt(d), samplers.py:285-287).  Then `n_samples` transitions are
    recorded.  Two gradient evaluations per transition."""
    if state is not None:      # continue a chain: position, direction, step size, L and random streams (see nuts_sample)
        rng = _Rng.from_state(state["rng"])
        dev = q0.device if q0 is not None else state["q"].device
        q, step_size, L = state["q"].clone().to(dev), state["step_size"], state["L"]
    else:
        rng = _Rng(seed)
        q = q0.clone()
    d = q.numel()
    lp, g = logdensity_and_grad(q)
    tune_L = bool(tune_L) and L is None and state is None
    L = float(L) if L is not None else math.sqrt(d)
    eps = float(step_size) if step_size is not None else math.sqrt(d) / 1e4 * 10.0
    n_tune1 = n_warmup // 2                      # stage 1: step size only; stage 2: step size + position variances
    x_avg = x2_avg = None
    wx_sum = 0.0
    if state is not None:
        u = state["u"].clone().to(q.device)
    else:
        u = torch.randn(q.shape, dtype=q.dtype, device=q.device, generator=rng.torch_gen(q.device))
        u = u / torch.linalg.vector_norm(u)
    infos, samples = [], []
    # step-size predictor (the scheme of blackjax's mclmc adaptation): the energy-error variance per dimension scales as
    # xi = C eps^6; C is tracked as a weighted running average (outliers down-weighted in log space) and
    # eps = C^(-1/6) puts xi at the target
    neff, sigma_xi = 150.0, 1.5
    gamma = (neff - 1.0) / (neff + 1.0)
    c_avg, w_sum = 0.0, 0.0
    t0 = time.perf_counter()
    for it in range(n_warmup + n_samples):
        warm = it < n_warmup
        qn, lpn, gn, un, dE = mclmc_step(logdensity_and_grad, q, lp, g, u, eps, L, rng)
        bad = not (math.isfinite(dE) and math.isfinite(lpn))
        if bad:                  # reject a blown-up step, shrink the step
            eps *= 0.5
            dE = float("nan")
        else:
            q, lp, g, u = qn, lpn, gn, un
        if warm and not bad:
            xi = dE * dE / (d * desired_energy_var) + 1e-8
            w = math.exp(-0.5 * (math.log(xi) / (6.0 * sigma_xi)) ** 2)
            c_avg = gamma * c_avg + w * xi / eps ** 6
            w_sum = gamma * w_sum + w
            eps = (c_avg / w_sum) ** (-1.0 / 6.0)
            if tune_L and it >= n_tune1:
                qd = q.double()
                if x_avg is None:
                    x_avg, x2_avg = torch.zeros_like(qd), torch.zeros_like(qd)
                x_avg = gamma * x_avg + w * qd
                x2_avg = gamma * x2_avg + w * qd * qd
                wx_sum = gamma * wx_sum + w
        if tune_L and it == n_warmup - 1 and x_avg is not None and wx_sum > 0:
            var = x2_avg / wx_sum - (x_avg / wx_sum) ** 2
            Lnew = math.sqrt(max(float(var.clamp_min(0).sum()), 0.0))
            if math.isfinite(Lnew) and Lnew > 0:
                L = Lnew
        if not warm:
            samples.append(keep(q) if keep is not None else q.clone())
        info = {"energy_change": dE, "mse_per_dim": dE * dE / d if not bad else float("nan"), "step_size": eps, "L": L,
                "warmup": warm, "logdensity": lp, "n_evals": 2}
        infos.append(info)
        if callback is not None:
            callback(it, info)
    return {"samples": samples, "step_size": eps, "L": L, "infos": infos, "seconds": time.perf_counter() - t0,
            "last_state": {"sampler": "mclmc", "q": q.clone(), "u": u.clone(), "step_size": eps, "L": L, "rng": rng.get_state()}}


# ------------------------------------------------------------------------------------------------------------------
# Preconditioned MCLMC and MAMS (montecosmo/samplers.py:285-583: mclmc_warmup / mclmc_run / mams_warmup / mams_run, which
# drive blackjax) on one integrator object.  The diagonal metric enters as s = sqrt(inverse_mass): the force is s g, the
# drift s u.  Two back ends, one interface: 'hip' runs the fused kernels of csrc/mclmc.hip on float32 device vectors (two
# passes per velocity update, the sums and the energy stay on the device until the end of the transition), 'torch' runs
# the same formulas through torch ops on any dtype and device.
class _TorchIntegrator:
    backend = "torch"

    def __init__(self, q, inverse_mass=None):
        self.d, self.dtype, self.device = q.numel(), q.dtype, q.device
        self.dK = 0.0
        self.set_inverse_mass(inverse_mass)

    def set_inverse_mass(self, inverse_mass):
        self.s = None if inverse_mass is None else torch.sqrt(inverse_mass.to(device=self.device, dtype=torch.float64)).to(self.dtype)

    def kick_drift(self, u, q, g, eps_kick, eps_drift):
        """In place: u <- B(eps_kick) u for the gradient g, then q += eps_drift s u' (q may be None).  Adds the kinetic
        energy change to the running sum `read_dK` returns.  u need not be normalised."""
        gt = g.double() if self.s is None else self.s.double() * g.double()
        ud = u.double()
        gg, ug, uu = float(torch.dot(gt, gt)), float(torch.dot(ud, gt)), float(torch.dot(ud, ud))
        n = math.sqrt(uu)
        if gg > 0.0:
            gam = math.sqrt(gg)
            c = ug / (gam * n)
            delta = eps_kick * gam / (self.d - 1)
            z = math.exp(-delta)
            D = max((1.0 + c) + (1.0 - c) * z * z, 1e-300)
            ca, cb = (1.0 - z) * (1.0 + z + c * (1.0 - z)) / (gam * D), 2.0 * z / (n * D)
            self.dK += (self.d - 1) * (delta - math.log(2.0) + math.log(D))
            u.copy_(ca * gt + cb * ud)
        else:
            u.copy_(ud / n)
        if q is not None:
            su = u.double() if self.s is None else self.s.double() * u.double()
            q.copy_(q.double() + eps_drift * su)

    def refresh(self, u, nu, rng):
        """Partial refresh u += nu z (left un-normalised: the next kick divides by the norm it measures)."""
        u.add_(torch.randn(u.shape, dtype=u.dtype, device=u.device, generator=rng.torch_gen(u.device)), alpha=nu)

    def new_moments(self):
        return (torch.zeros(self.d, dtype=torch.float64, device=self.device), torch.zeros(self.d, dtype=torch.float64, device=self.device))

    def moments(self, q, gamma, w, xavg, x2avg):
        """In place: xavg = gamma xavg + w q, x2avg = gamma x2avg + w q^2 (float64)."""
        qd = q.double()
        xavg.mul_(gamma).add_(w * qd)
        x2avg.mul_(gamma).add_(w * (qd * qd))

    def zero_dK(self):
        self.dK = 0.0

    def read_dK(self):
        """The kinetic energy change summed since `zero_dK`."""
        return self.dK


class _HipIntegrator(_TorchIntegrator):
    backend = "hip"

    def __init__(self, q, inverse_mass=None):
        from . import nbody
        if not (q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.dim() == 1):
            raise ValueError("backend='hip' serves flat contiguous float32 device tensors")
        self.plan = nbody.get_plan((8, 8, 8))      # shape-free passes: the plan lends its stream and reduction scratch
        self.stats = torch.zeros(4, dtype=torch.float64, device=q.device)
        super().__init__(q, inverse_mass)

    def set_inverse_mass(self, inverse_mass):
        super().set_inverse_mass(inverse_mass)
        if self.s is not None:
            self.s = self.s.contiguous()

    def kick_drift(self, u, q, g, eps_kick, eps_drift):
        self.plan.call("mcpm_mclmc_kick_drift_f32", u, q, g if g.is_contiguous() else g.contiguous(), self.s, self.d, float(eps_kick),
                       float(eps_drift), self.stats)

    def moments(self, q, gamma, w, xavg, x2avg):
        self.plan.call("mcpm_mclmc_moments_f64", q, self.d, float(gamma), float(w), xavg, x2avg)

    def zero_dK(self):
        self.stats[3:].zero_()

    def read_dK(self):
        return float(self.stats[3])      # the transition's one read-back: 8 bytes


def hip_backend_applies(q):
    """Whether backend='auto' takes the HIP kernels for this state vector (float32, contiguous, on the device)."""
    return bool(q.is_cuda and q.dtype == torch.float32 and q.is_contiguous() and q.dim() == 1 and q.numel() >= 2)


def make_integrator(q, inverse_mass=None, backend="auto"):
    """The integrator object of the samplers below for states like `q`: backend 'hip', 'torch' or 'auto' ('hip' where it
    applies).  Interface: kick_drift, refresh, moments, zero_dK / read_dK."""
    if backend == "auto":
        backend = "hip" if hip_backend_applies(q) else "torch"
    if backend == "hip":
        return _HipIntegrator(q, inverse_mass)
    if backend == "torch":
        return _TorchIntegrator(q, inverse_mass)
    raise ValueError(f"backend must be 'auto', 'hip' or 'torch', not {backend!r}")


def mclachlan_step(integ, fn, q, u, lp, g, eps):
    """One McLachlan minimal-norm step B(lam eps) A(eps/2) B((1-2 lam) eps) A(eps/2) B(lam eps) under the integrator's
    metric, IN PLACE on q and u; (lp, g) belong to the incoming q.  Returns (lp', g', energy change)."""
    lam = _MCLACHLAN
    integ.zero_dK()
    integ.kick_drift(u, q, g, lam * eps, 0.5 * eps)
    lp1, g1 = fn(q)
    integ.kick_drift(u, q, g1, (1 - 2 * lam) * eps, 0.5 * eps)
    lp2, g2 = fn(q)
    integ.kick_drift(u, None, g2, lam * eps, 0.0)
    if not math.isfinite(lp1):
        return lp2, g2, float("nan")
    return lp2, g2, integ.read_dK() - (lp2 - lp)


def _unit_normal(q, rng):
    u = torch.randn(q.shape, dtype=q.dtype, device=q.device, generator=rng.torch_gen(q.device))
    return u / torch.linalg.vector_norm(u)


def _mclmc_transition(integ, fn, st, eps, L, rng):
    """One MCLMC transition on the chain state `st` (dict q, u, lp, g): a McLachlan step, then the partial refresh
    u += nu z.  A blown-up step is rejected (st unchanged).  Returns the energy change (nan when rejected)."""
    q, u = st["q"].clone(), st["u"].clone()
    lp, g, dE = mclachlan_step(integ, fn, q, u, st["lp"], st["g"], eps)
    if not (math.isfinite(dE) and math.isfinite(lp)):
        return float("nan")
    nu = math.sqrt((math.exp(2.0 * eps / L) - 1.0) / q.numel())
    integ.refresh(u, nu, rng)
    st.update(q=q, u=u, lp=lp, g=g)
    return dE


def _mams_transition(integ, fn, st, eps, L, rng):
    """One MAMS transition: fresh u on the sphere, n = max(1, ceil(U (2 L / eps - 1))) McLachlan steps without refresh,
    accepted with probability min(1, exp(-dE)).  A rejection leaves q, lp and g as they are.  Returns
    (acceptance probability, n)."""
    u = _unit_normal(st["q"], rng)
    n = max(1, math.ceil(rng.random() * (2.0 * L / eps - 1.0)))
    q, lp, g, dE = st["q"].clone(), st["lp"], st["g"], 0.0
    for _ in range(n):
        lp, g, de = mclachlan_step(integ, fn, q, u, lp, g, eps)
        dE += de
        if not math.isfinite(dE):
            break
    acc = min(1.0, math.exp(min(0.0, -dE))) if (math.isfinite(dE) and math.isfinite(lp)) else 0.0
    if rng.random() < acc:
        st.update(q=q, lp=lp, g=g)
    st["u"] = u
    return acc, n


def _unit(u):
    return u / torch.linalg.vector_norm(u)


def _config(config, d, eps0):
    config = dict(config or {})
    L = float(config["L"]) if config.get("L") is not None else math.sqrt(d)
    eps = float(config["step_size"]) if config.get("step_size") is not None else eps0
    return L, eps, config.get("inverse_mass")


def _variance(xavg, x2avg, wsum):
    return (x2avg / wsum - (xavg / wsum) ** 2).clamp_min(0.0)


def _start(fn, q0, rng):
    q = q0.clone()
    lp, g = fn(q)
    return {"q": q, "u": _unit_normal(q, rng), "lp": lp, "g": g}


def _state_out(sampler, st, eps, L, inverse_mass, rng):
    # 'u' is stored normalised; the chain itself carries the refreshed, un-normalised direction into its next kick, and 'u_raw' (on the
    # host, as `save_run` leaves the rest) is that vector, from which a continued chain repeats the uninterrupted one bit for bit
    return {"sampler": sampler, "q": st["q"].clone(), "u": _unit(st["u"]), "u_raw": st["u"].detach().cpu(), "step_size": eps, "L": L,
            "rng": rng.get_state(), "inverse_mass": None if inverse_mass is None else inverse_mass.clone()}


def mclmc_warmup(logdensity_and_grad, q0, n_steps, config=None, desired_energy_var=5e-4, diagonal_preconditioning=False, seed=0,
                 backend="auto"):
    """Tunes MCLMC (`blackjax.mclmc_find_L_and_step_size` as the reference calls it, samplers.py:318-337: frac_tune1 =
    frac_tune2 = 0.5, no ESS stage).  `config`: dict(L, step_size, inverse_mass) to start from (defaults: sqrt(d),
    sqrt(d) / 1000, identity).  `n_steps` is the total number of transitions spent.  First half: the step size is driven to
    an energy-error variance per dimension of `desired_energy_var` (the predictor of `mclmc_sample`); second half: the same,
    and the running moments of the position.  At the end, without preconditioning, L = sqrt(sum var).  With it,
    inverse_mass = var, L = sqrt(d), and a third stage (one third of the second's length) re-tunes the step size under the
    new metric with fresh averages.  Returns (state, config); `state` goes to `mclmc_run`."""
    rng = _Rng(seed)
    d = q0.numel()
    L, eps, inverse_mass = _config(config, d, math.sqrt(d) / 1e4 * 10.0)
    integ = make_integrator(q0, inverse_mass, backend)
    st = _start(logdensity_and_grad, q0, rng)
    n_steps = int(n_steps)
    if diagonal_preconditioning:      # n1 + n2 + n2 // 3 = n_steps, n1 = n2 up to rounding (the reference's num_steps formula)
        n2 = int(round(n_steps / (2.0 + 1.0 / 3.0)))
        n3 = n2 // 3
        n1 = max(n_steps - n2 - n3, 0)
    else:
        n1 = n_steps // 2
        n2, n3 = n_steps - n1, 0
    neff, sigma_xi = 150.0, 1.5
    gamma = (neff - 1.0) / (neff + 1.0)
    c_avg = w_sum = wx_sum = 0.0
    xavg = x2avg = None
    for it in range(n_steps):
        if it == n1 + n2 and n3 > 0:
            c_avg = w_sum = 0.0      # third stage: fresh step-size averages under the new metric
        dE = _mclmc_transition(integ, logdensity_and_grad, st, eps, L, rng)
        if not math.isfinite(dE):
            eps *= 0.5
            continue
        xi = dE * dE / (d * desired_energy_var) + 1e-8
        w = math.exp(-0.5 * (math.log(xi) / (6.0 * sigma_xi)) ** 2)
        c_avg = gamma * c_avg + w * xi / eps ** 6
        w_sum = gamma * w_sum + w
        eps = (c_avg / w_sum) ** (-1.0 / 6.0)
        if n1 <= it < n1 + n2:
            if xavg is None:
                xavg, x2avg = integ.new_moments()
            integ.moments(st["q"], gamma, w, xavg, x2avg)
            wx_sum = gamma * wx_sum + w
        if it == n1 + n2 - 1 and xavg is not None and wx_sum > 0:
            var = _variance(xavg, x2avg, wx_sum)
            if diagonal_preconditioning:
                inverse_mass = var.clamp_min(1e-30).to(q0.dtype)
                integ.set_inverse_mass(inverse_mass)
                L = math.sqrt(d)
            else:
                Lnew = math.sqrt(float(var.sum()))
                if math.isfinite(Lnew) and Lnew > 0:
                    L = Lnew
    config = {"L": L, "step_size": eps, "inverse_mass": inverse_mass}
    return _state_out("mclmc", st, eps, L, inverse_mass, rng), config


def _run(kind, transition, logdensity_and_grad, state, config, n_samples, thinning, seed, keep, callback, backend):
    rng = _Rng(seed) if seed is not None else _Rng.from_state(state["rng"])
    q = state["q"].clone()
    d = q.numel()
    config = config if config is not None else state
    L, eps = float(config["L"]), float(config["step_size"])
    inverse_mass = config.get("inverse_mass")
    if inverse_mass is not None:
        inverse_mass = inverse_mass.to(q.device)
    integ = make_integrator(q, inverse_mass, backend)
    lp, g = logdensity_and_grad(q)
    st = {"q": q, "u": state["u_raw" if "u_raw" in state else "u"].clone().to(q.device), "lp": lp, "g": g}
    thinning = int(thinning)
    samples, infos = [], []
    t0 = time.perf_counter()
    for it in range(int(n_samples)):
        info = transition(integ, logdensity_and_grad, st, eps, L, rng, thinning, d)
        samples.append(keep(st["q"]) if keep is not None else st["q"].clone())
        info.update(step_size=eps, L=L, warmup=False, logdensity=st["lp"])
        infos.append(info)
        if callback is not None:
            callback(it, info)
    return {"samples": samples, "step_size": eps, "L": L, "inverse_mass": inverse_mass, "infos": infos, "seconds": time.perf_counter() - t0,
            "backend": integ.backend, "last_state": _state_out(kind, st, eps, L, inverse_mass, rng)}


def _mclmc_thinned(integ, fn, st, eps, L, rng, thinning, d):
    s2 = 0.0
    for _ in range(thinning):
        dE = _mclmc_transition(integ, fn, st, eps, L, rng)
        s2 += dE * dE
    rms = math.sqrt(s2 / thinning) if math.isfinite(s2) else float("nan")
    return {"energy_change": rms, "mse_per_dim": rms * rms / d, "n_evals": 2 * thinning}


def _mams_thinned(integ, fn, st, eps, L, rng, thinning, d):
    acc, n = 0.0, 0
    for _ in range(thinning):
        a, k = _mams_transition(integ, fn, st, eps, L, rng)
        acc, n = acc + a, n + k
    return {"acceptance_rate": acc / thinning, "accept_stat": acc / thinning, "n_steps": n, "n_evals": 2 * n}


def mclmc_run(logdensity_and_grad, state, config=None, n_samples=200, thinning=1, seed=None, keep=None, callback=None, backend="auto"):
    """`n_samples` kept states of MCLMC from `state` (of `mclmc_warmup`, or a previous run's `last_state`) under `config`
    (dict(L, step_size, inverse_mass); None: the values `state` carries), every `thinning`-th transition kept.  Per kept
    state `energy_change` is the RMS of the skipped steps' energy changes, `mse_per_dim` its square over d and `n_evals` =
    2 thinning (samplers.py:379-400).  seed=None continues the random streams of `state` (a chain continued from a saved
    state repeats the uninterrupted one bit for bit); a seed starts fresh ones.  The result has `mclmc_sample`'s shape;
    `last_state` also carries `inverse_mass`."""
    return _run("mclmc", _mclmc_thinned, logdensity_and_grad, state, config, n_samples, thinning, seed, keep, callback, backend)


def mams_warmup(logdensity_and_grad, q0, n_steps, config=None, target_acc_rate=0.65, diagonal_preconditioning=False, seed=0,
                backend="auto"):
    """Tunes MAMS, the Metropolis-adjusted microcanonical sampler (samplers.py:432-497).  Schedule of `mclmc_warmup` (two
    halves, plus a third of the second under a new metric), with the step size tuned by dual averaging of the acceptance
    probability to `target_acc_rate` (samplers.py:481) and plain running moments in the second stage: L = sqrt(sum var), or
    inverse_mass = var and L = sqrt(d).  Defaults: L = sqrt(d), step size sqrt(d) / 64 (samplers.py:447).
    The number of steps of a trajectory is n = max(1, ceil(U (2 L / eps - 1))), mean L / eps; blackjax's `rescale`
    interpolates for non-integer arguments, which this does not.  Only L_proposal_factor = inf (no refresh inside a
    trajectory) is built.  Returns (state, config)."""
    rng = _Rng(seed)
    d = q0.numel()
    L, eps, inverse_mass = _config(config, d, math.sqrt(d) / 64.0)
    integ = make_integrator(q0, inverse_mass, backend)
    st = _start(logdensity_and_grad, q0, rng)
    n_steps = int(n_steps)
    if diagonal_preconditioning:
        n2 = int(round(n_steps / (2.0 + 1.0 / 3.0)))
        n3 = n2 // 3
        n1 = max(n_steps - n2 - n3, 0)
    else:
        n1 = n_steps // 2
        n2, n3 = n_steps - n1, 0
    da = DualAveraging(eps, target=target_acc_rate)
    xavg = x2avg = None
    cnt = 0
    for it in range(n_steps):
        if it == n1 + n2 and n3 > 0:
            da = DualAveraging(eps, target=target_acc_rate)
        acc, _ = _mams_transition(integ, logdensity_and_grad, st, eps, L, rng)
        eps = da.update(acc)
        if n1 <= it < n1 + n2:
            if xavg is None:
                xavg, x2avg = integ.new_moments()
            integ.moments(st["q"], 1.0, 1.0, xavg, x2avg)
            cnt += 1
        if it == n1 + n2 - 1 and cnt > 1:
            eps = da.final()
            var = _variance(xavg, x2avg, float(cnt))
            if diagonal_preconditioning:
                inverse_mass = var.clamp_min(1e-30).to(q0.dtype)
                integ.set_inverse_mass(inverse_mass)
                L = math.sqrt(d)
            else:
                Lnew = math.sqrt(float(var.sum()))
                if math.isfinite(Lnew) and Lnew > 0:
                    L = Lnew
    if n_steps > 0:
        eps = da.final()
    config = {"L": L, "step_size": eps, "inverse_mass": inverse_mass}
    return _state_out("mams", st, eps, L, inverse_mass, rng), config


def mams_run(logdensity_and_grad, state, config=None, n_samples=200, thinning=1, seed=None, keep=None, callback=None, backend="auto"):
    """`n_samples` kept states of MAMS (see `mams_warmup` for the transition).  `infos` carry `acceptance_rate`, `n_steps`
    and `n_evals` = 2 n_steps; thinning averages the first and sums the other two (samplers.py:543-551).  Otherwise as
    `mclmc_run`."""
    return _run("mams", _mams_thinned, logdensity_and_grad, state, config, n_samples, thinning, seed, keep, callback, backend)


def collapse_configs(configs, eval_per_ess=1e3):
    """The chains' configs collapsed to one shared config (montecosmo/script.py:141-144): the median step size,
    L = 0.4 eval_per_ess / 2 step_size, the element-wise median inverse mass (None when no chain has one)."""
    def median(x):      # over the chain axis, the mean of the middle two for an even count (torch.quantile caps its input's size)
        x, n = torch.sort(x.double(), dim=0).values, x.shape[0]
        return x[n // 2] if n % 2 else 0.5 * (x[n // 2 - 1] + x[n // 2])
    eps = float(median(torch.tensor([float(c["step_size"]) for c in configs], dtype=torch.float64)))
    ims = [c.get("inverse_mass") for c in configs]
    inverse_mass = None
    if any(m is not None for m in ims):
        ref = next(m for m in ims if m is not None)
        inverse_mass = median(torch.stack([torch.ones_like(ref) if m is None else m.to(ref.device) for m in ims])).to(ref.dtype)
    return {"L": 0.4 * eval_per_ess / 2.0 * eps, "step_size": eps, "inverse_mass": inverse_mass}


def chain_sampler(kind="mclmc", **warmup_kw):
    """Adapter for `sample_and_save`: a callable with the signature of `mclmc_sample` that warms up (`mclmc_warmup` /
    `mams_warmup` with `warmup_kw`) unless it is handed a state, then runs `mclmc_run` / `mams_run`.  Keywords thinning, seed,
    keep, callback and backend pass through `sample_and_save`."""
    warmup, run = {"mclmc": (mclmc_warmup, mclmc_run), "mams": (mams_warmup, mams_run)}[kind]

    def sampler(logdensity_and_grad, q0, n_warmup=200, n_samples=200, state=None, seed=0, backend="auto", **kw):
        config = None
        if state is None:
            state, config = warmup(logdensity_and_grad, q0, n_warmup, seed=seed, backend=backend, **warmup_kw)
        elif q0 is not None:
            state = dict(state, q=state["q"].to(q0.device), u=state["u"].to(q0.device))
        return run(logdensity_and_grad, state, config, n_samples, backend=backend, **kw)
    return sampler


# ------------------------------------------------------------------------------------------------------------------
# MAP optimisation (montecosmo/samplers.py:671-696: `optimize`, Adam from jax.example_libraries.optimizers with the learning
# rate lr0 / sqrt(1 + i)).  jax is not installed where this was written: the update below is restated from knowledge of that
# library (adam(step_size, b1=0.9, b2=0.999, eps=1e-8): m and v start at zero, both are bias-corrected, eps is added to the
# root), as is done for numpyro and jax_cosmo elsewhere in the package.
def _adam_torch(q, m, v, g, lr, b1, b2, eps, c1, c2):
    """One Adam epoch in place through torch ops: the formulas of csrc/lapprox.hip in float64, rounded once to the dtype of q."""
    gu = -g.double()
    md = (1.0 - b1) * gu + b1 * m.double()
    vd = (1.0 - b2) * (gu * gu) + b2 * v.double()
    q.copy_(q.double() - (lr * (md * c1)) / (torch.sqrt(vd * c2) + eps))
    m.copy_(md)
    v.copy_(vd)


def optimize(logdensity_and_grad, start, lr0=0.1, n_epochs=100, b1=0.9, b2=0.999, eps=1e-8, backend="auto", callback=None):
    """Climbs the log density from `start` by Adam, the reference's `optimize(potential, start, lr0, n_epochs)` on the flat
    contract `logdensity_and_grad(q) -> (lp, g)`.  With U = -log p, g_U = -g and epoch i = 0, 1, ...:

        m = (1 - b1) g_U + b1 m,   v = (1 - b2) g_U^2 + b2 v,
        q -= lr0 / sqrt(1 + i) * [m / (1 - b1^(i+1))] / (sqrt(v / (1 - b2^(i+1))) + eps)

    which is jax.example_libraries.optimizers.adam under the schedule lr0 / sqrt(1 + i), restated from knowledge of that
    library (jax is not a dependency).  Returns (q, pots): pots[i] is the potential at the point epoch i STARTS from, as in the
    reference, and q the state after the last update.  A non-finite log density (FlatLogDensity returns -inf outside the support)
    stops the loop: the last point whose potential was finite is returned, with pots up to there.  A NaN raises.

    backend 'hip' runs one fused pass per epoch (mcpm_adam_step_f32) on a flat contiguous float32 device vector, 'torch' the same
    formulas through torch ops on any dtype and device, 'auto' takes 'hip' where it applies.  Nothing is random: two runs from one
    start are bitwise equal.  callback(i, {'potential', 'lr'}) is called once per epoch."""
    if backend == "auto":
        backend = "hip" if hip_backend_applies(start) else "torch"
    if backend not in ("hip", "torch"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'torch', not {backend!r}")
    q = start.clone()
    if backend == "hip":
        from . import nbody
        if not hip_backend_applies(q):
            raise ValueError("backend='hip' serves flat contiguous float32 device tensors")
        plan = nbody.get_plan((8, 8, 8))      # shape-free pass: the plan lends its stream
    m, v, last = torch.zeros_like(q), torch.zeros_like(q), q.clone()
    pots = []
    for i in range(int(n_epochs)):
        lp, g = logdensity_and_grad(q)
        lp = float(lp)
        if math.isnan(lp):
            raise FloatingPointError(f"log density is NaN at epoch {i}")
        if not math.isfinite(lp):      # the last update left the support
            return last, pots
        pots.append(-lp)
        last.copy_(q)
        lr = lr0 / math.sqrt(1.0 + i)
        c1, c2 = 1.0 / (1.0 - b1 ** (i + 1)), 1.0 / (1.0 - b2 ** (i + 1))
        if backend == "hip":
            plan.call("mcpm_adam_step_f32", q, m, v, g if g.is_contiguous() else g.contiguous(), q.numel(), lr, float(b1), float(b2),
                      float(eps), c1, c2)
        else:
            _adam_torch(q, m, v, g, lr, b1, b2, eps, c1, c2)
        if callback is not None:
            callback(i, {"potential": -lp, "lr": lr})
    return q, pots
