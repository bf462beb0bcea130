"""
Device-resident nested sampler with a results interface shaped like nautilus's (``run``, ``posterior``, ``log_z``).

The reference runs half of its scripts under nautilus and publishes their log-evidence (``sampler.log_z``).  This is NOT
nautilus's algorithm (no neural-network boundaries, no importance-sampling shells): it is classic nested sampling
(Skilling 2006) with batch deletion and constrained differential-evolution walks.  Its log Z agrees with the truth within
its own stated error; it does not reproduce nautilus's numbers bit for bit.

Algorithm, as built.  n = n_live, d = ndim, k = n_batch.  Points live in the unit cube; theta = T(u) is the prior transform,
lo + u (hi - lo) for a uniform dimension, loc + scale * Phi^-1(u) for a normal one.

* Start.  u uniform on (0, 1)^d for all n points from the counter-based generator keyed on (seed, iteration 0, step 0) with
  stream = dimension and counter = point index (cf_ns_prior_draw).  log L is evaluated; a non-finite value becomes -inf and is
  counted (``n_nonfinite_start``).
* Iteration t = 1, 2, ...
  1. The live points are ordered by (log L ascending, index ascending) (a stable torch.sort); L* is the k-th lowest value.
  2. Every point with log L <= L* dies (ties die together, so m >= k points die).  The survivors S are the rest, in index
     order.  |S| < 2 raises (a likelihood plateau).
  3. Bookkeeping in the sorted order: death j (0-based) of the iteration happens with n - j points live; it gets
     ln w = log L + ln X + ln(1 - exp(-1 / (n - j))) with ln X before the death, then ln X -= 1 / (n - j).  A -inf point
     gets ln w = -inf.
  4. Walker i of the m dead slots (slots in index order) starts at S[floor(U * |S|)] (cf_ns_walk_start, step 0, stream 0).
  5. n_walk steps s = 1 .. n_walk of a DE walk against the frozen survivor snapshot (cf_ns_propose, cf_ns_accept):
     u' = u + gamma (u_a - u_b) + sigma N(0, 1) per dimension, a != b uniform on S (streams 0, 1; the normal of dimension
     k from streams 2 + 2k, 3 + 2k).  gamma = 2.38 / sqrt(2 d) (the DE move's scale), sigma = 1e-6 (a jitter that makes the
     walk irreducible; it is far below any posterior width in the cube).  The walker moves iff u' lies in the open cube and
     log L(T(u')) is finite and > L*.  The proposal is symmetric for a fixed snapshot and the target is uniform on
     {L > L*}, so this indicator is the Metropolis test.  An out-of-cube proposal is not evaluated at u': the likelihood
     sees the walker's current theta and the proposal is rejected.
  6. Each walker's final state fills its dead slot.
* Termination.  Before every iteration ln Z_live = ln X + logsumexp(log L_live) - ln n; the run stops when
  Z_live / (Z_dead + Z_live) < f_live (nautilus's default 0.01), or at the iteration cap.  The live points count with
  ln w = log L + ln X - ln n.
* Results.  All sums run in one fixed order: the dead points in death order, then the live points in index order.
  log_z = logsumexp(ln w), H = sum p_i log L_i - log_z (p_i = exp(ln w_i - log_z)), log_z_err = sqrt(H / n),
  n_eff = (sum p)^2 / sum p^2 (Kish).

Defaults: k = n // 2 and n_walk = 20 d (the calibration test runs 10 seeds of a 3-D Gaussian at n = 500 with them: the
scatter of log Z matches log_z_err and there is no bias).  Deleting half the live set per iteration shrinks ln X by
~ln 2 with variance ~1 / n per iteration; the scatter of log Z is then ~1.2 sqrt(H / n), a little above the classic error
sqrt(H / n) that log_z_err reports (the CPU shrinkage test measures the ratio).

Random numbers: the ensemble's counter-based generator (ensemble._mix_int, the kernels' ens_uniform / ens_normal), keyed by
``ns_key(seed, iteration, step)``; stream s has key + s and the counter is the row (point or walker) index.  The key passes
seed, iteration and step through their own hash rounds behind a domain tag of its own, so no key meets an ensemble key.
The same seed gives the same bits on every run.

Device work per iteration: one sort, the index_select / index_copy_ of the dead and surviving rows, one host read of the
sorted log L (the bookkeeping and the termination test run on the host in float64 numpy), and per walk step one propose
launch, one likelihood call and one accept launch on torch's current stream, with no host round trip.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Sequence, Tuple

import numpy as np

from ._args import stream_of
from .ensemble import _U64, _mix_int, uniform01_scalar

# ---- random-stream keys ----------------------------------------------------------------------------------------------
_NS_TAG = 0x4E45535445445331  # "NESTEDS1": the nested sampler's domain tag (the ensemble's constant is 0x5851F42D4C957F2D)
_GOLDEN = 0x9E3779B97F4A7C15


def ns_key(seed: int, iteration: int, step: int) -> int:
    """Unsigned 64-bit key of stream 0 for (seed, iteration, walk step); stream s has key + s.  Iteration 0 step 0 is the
    prior draw, step 0 of an iteration the walk start, steps 1 .. n_walk the walk."""
    base = _mix_int(_mix_int((seed * _GOLDEN + _NS_TAG) & _U64) ^ (iteration & _U64))
    return _mix_int(base ^ (step & _U64))


def uniform_open_scalar(key: int, counter: int) -> float:
    """The prior draw's uniform in (0, 1): the ensemble's 53 bits with the lowest one set (cf_ns_prior_draw)."""
    x = _mix_int(((counter & _U64) * _GOLDEN + key) & _U64)
    x = _mix_int((x + _GOLDEN) & _U64)
    return ((x >> 11) | 1) * (1.0 / 9007199254740992.0)


__all__ = ["Prior", "DeviceNestedSampler", "ns_key", "uniform_open_scalar", "uniform01_scalar", "kill", "live_log_weights",
           "live_fraction", "summarize", "logsumexp"]


# ---- prior -----------------------------------------------------------------------------------------------------------
class Prior:
    """nautilus's ``Prior`` for the two kinds the reference uses: ``add_parameter(key, dist=(lo, hi))`` (uniform) and
    ``add_parameter(key, dist=scipy.stats.norm(loc, scale))`` (a frozen normal)."""

    def __init__(self):
        self.keys = []
        self._kind, self._a, self._b = [], [], []

    def add_parameter(self, key=None, dist=(0.0, 1.0)):
        from . import _lib as L

        key = f"x_{len(self.keys)}" if key is None else key
        if key in self.keys:
            raise ValueError(f"parameter {key!r} is already in the prior")
        if len(self.keys) >= L.CF_NS_MAX_NDIM:
            raise ValueError(f"the device sampler takes at most {L.CF_NS_MAX_NDIM} parameters")
        if isinstance(dist, tuple) and len(dist) == 2 and all(isinstance(v, (int, float, np.integer, np.floating)) for v in dist):
            lo, hi = float(dist[0]), float(dist[1])
            if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
                raise ValueError(f"parameter {key!r}: a uniform prior needs finite lo < hi, got {dist}")
            kind, a, b = L.CF_NS_UNIFORM, lo, hi
        elif getattr(getattr(dist, "dist", None), "name", None) == "norm" and hasattr(dist, "kwds"):
            args, kwds = tuple(dist.args), dict(dist.kwds)
            loc = float(kwds.get("loc", args[0] if len(args) > 0 else 0.0))
            scale = float(kwds.get("scale", args[1] if len(args) > 1 else 1.0))
            if not (math.isfinite(loc) and math.isfinite(scale) and scale > 0):
                raise ValueError(f"parameter {key!r}: a normal prior needs a finite loc and scale > 0")
            kind, a, b = L.CF_NS_NORMAL, loc, scale
        else:
            raise ValueError(f"parameter {key!r}: dist must be a (lo, hi) tuple or a frozen scipy.stats.norm, got {dist!r}")
        self.keys.append(key)
        self._kind.append(kind)
        self._a.append(a)
        self._b.append(b)

    def dimensionality(self) -> int:
        return len(self.keys)

    def unit_to_physical(self, u) -> np.ndarray:
        """T(u) on the host (numpy / scipy.special.ndtri): the restatement of cf_ns_transform."""
        from scipy.special import ndtri

        u = np.asarray(u, dtype=np.float64)
        out = np.empty_like(u)
        for k, (kind, a, b) in enumerate(zip(self._kind, self._a, self._b)):
            out[..., k] = a + b * ndtri(u[..., k]) if kind == 1 else a + u[..., k] * (b - a)
        return out

    def c_struct(self):
        from . import _lib as L

        if not self.keys:
            raise ValueError("the prior has no parameters")
        p = L.cf_ns_prior()
        p.ndim = len(self.keys)
        for k in range(p.ndim):
            p.kind[k], p.a[k], p.b[k] = self._kind[k], self._a[k], self._b[k]
        return p


# ---- bookkeeping (pure float64 numpy: the CPU tests drive it without a GPU) ------------------------------------------
def logsumexp(x) -> float:
    """log(sum(exp(x))) over x in the given order (numpy's sum of the shifted terms); -inf for an empty or all -inf x."""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return -math.inf
    mx = float(np.max(x))
    if mx == -math.inf:
        return -math.inf
    return mx + math.log(float(np.sum(np.exp(x - mx))))


def kill(dead_log_l, ln_x: float, n: int) -> Tuple[np.ndarray, float]:
    """Step 3: the deaths of one iteration in death order (log L ascending).  Death j happens with n - j points live:
    ln w_j = log L_j + ln X + ln(1 - exp(-1 / (n - j))), then ln X -= 1 / (n - j).  Returns (ln w [m], ln X after)."""
    dead_log_l = np.asarray(dead_log_l, dtype=np.float64)
    ln_w = np.empty(dead_log_l.size)
    for j, l in enumerate(dead_log_l.tolist()):
        a = 1.0 / (n - j)
        ln_w[j] = -math.inf if l == -math.inf else l + ln_x + math.log(-math.expm1(-a))
        ln_x -= a
    return ln_w, ln_x


def live_log_weights(live_log_l, ln_x: float, n: int) -> np.ndarray:
    """ln w = log L + ln X - ln n of the live points at the stop."""
    return (np.asarray(live_log_l, dtype=np.float64) + ln_x) - math.log(n)


def live_fraction(ln_x: float, live_log_l, dead_ln_w, n: int) -> float:
    """Z_live / (Z_dead + Z_live) with ln Z_live = ln X + logsumexp(log L_live) - ln n (the termination test)."""
    ln_live = ln_x + logsumexp(live_log_l) - math.log(n)
    ln_dead = logsumexp(dead_ln_w)
    if ln_live == -math.inf:
        return 0.0
    return math.exp(ln_live - np.logaddexp(ln_dead, ln_live))


def summarize(ln_w, log_l, n: int) -> dict:
    """log_z, H, log_z_err = sqrt(H / n) and Kish's n_eff of a weighted sequence (dead in death order, then live)."""
    ln_w, log_l = np.asarray(ln_w, dtype=np.float64), np.asarray(log_l, dtype=np.float64)
    log_z = logsumexp(ln_w)
    p = np.exp(ln_w - log_z)
    on = p > 0
    h = float(np.sum(p[on] * log_l[on])) - log_z
    return dict(log_z=log_z, h=h, log_z_err=math.sqrt(max(h, 0.0) / n),
                n_eff=float(np.sum(p)) ** 2 / float(np.sum(p * p)))


# ---- the sampler -----------------------------------------------------------------------------------------------------
class DeviceNestedSampler:
    """Nested sampler whose live set, constrained walks and dead-point store stay on the GPU.

    log_likelihood: a torch callable theta [W, ndim] (cuda float64, contiguous) -> [W] float64 on the same device, e.g.
    ``lk.engine.torch_log_prob(CF_OUT_LOGL)`` (log L ignores the engine's box: the prior belongs to the sampler).
    There is no tensor fallback: without the HIP library or a GPU the constructor raises."""

    def __init__(self, prior: Prior, log_likelihood: Callable, *, n_live: int, n_batch: int = None, n_walk: int = None,
                 seed: int = 42, sigma: float = 1e-6):
        import torch

        from . import _lib as L

        self.L, self.lib = L, L.lib()  # raises if the HIP library is missing
        if self.lib.cf_device_count() < 1 or not torch.cuda.is_available():
            raise L.CosmofitError(-2, "DeviceNestedSampler runs its walks in the library's HIP kernels: no GPU is visible "
                                      "(there is no tensor fallback)")
        self.prior, self.ndim = prior, prior.dimensionality()
        self._c_prior = prior.c_struct()
        self.n_live = int(n_live)
        self.n_batch = self.n_live // 2 if n_batch is None else int(n_batch)
        self.n_walk = 20 * self.ndim if n_walk is None else int(n_walk)
        if self.n_live < 4:
            raise ValueError("n_live must be >= 4")
        if not 1 <= self.n_batch <= self.n_live - 2:
            raise ValueError("n_batch must be in 1 .. n_live - 2 (the walk needs two survivors)")
        if self.n_walk < 1:
            raise ValueError("n_walk must be >= 1")
        self.log_likelihood, self.seed = log_likelihood, int(seed)
        self.gamma, self.sigma = 2.38 / math.sqrt(2.0 * self.ndim), float(sigma)
        self.device = torch.device("cuda", torch.cuda.current_device())
        n, d, f64 = self.n_live, self.ndim, dict(dtype=torch.float64, device=self.device)
        self._live_u, self._live_th, self._live_l = torch.empty((n, d), **f64), torch.empty((n, d), **f64), None
        # walkers and proposals: at most n - 2 rows (two points survive every iteration)
        self._wu, self._wth, self._wl = torch.empty((n, d), **f64), torch.empty((n, d), **f64), torch.empty(n, **f64)
        self._pu, self._pth = torch.empty((n, d), **f64), torch.empty((n, d), **f64)
        self._ok = torch.empty(n, dtype=torch.int32, device=self.device)
        self._counts = torch.zeros(3, dtype=torch.int64, device=self.device)  # accepted, out of the cube, non-finite
        self._dead_th, self._dead_l, self._dead_lnw = [], [], []
        self._ln_x, self._it, self._n_like, self._n_walk_props = 0.0, 0, 0, 0
        self.n_nonfinite_start = 0
        self._results = None
        self._post_dev = None  # (the results they belong to, points, weights) on the device, for marginals() / mean_std()

    # ---- device steps --------------------------------------------------------------------------------------------
    def _loglike(self, theta):
        import torch

        out = self.log_likelihood(theta)
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.device == theta.device and
                out.shape == (theta.shape[0],)):
            raise ValueError("log_likelihood must return a float64 tensor [W] on the device of theta")
        self._n_like += theta.shape[0]
        return out.contiguous()

    def _start(self):
        import torch

        L, lib = self.L, self.lib
        L.check(lib.cf_ns_prior_draw(C.byref(self._c_prior), self.n_live, ns_key(self.seed, 0, 0), self._live_u.data_ptr(),
                                     self._live_th.data_ptr(), stream_of(self.device)))
        lv = self._loglike(self._live_th)
        bad = ~torch.isfinite(lv)
        self.n_nonfinite_start = int(bad.sum())
        self._live_l = torch.where(bad, torch.full_like(lv, -math.inf), lv)

    def _iterate(self, sorted_l, order, host):
        """Steps 2-6 of one iteration; host = sorted_l on the host."""
        import torch

        L, lib, n, d = self.L, self.lib, self.n_live, self.ndim
        lstar = host[self.n_batch - 1]
        m = int(np.searchsorted(host, lstar, side="right"))
        if n - m < 2:
            raise RuntimeError(f"nested sampling: {m} of {n} live points share log L <= {lstar!r} (a likelihood plateau); "
                               "fewer than two survivors are left for the walk")
        self._it += 1
        ln_w, self._ln_x = kill(host[:m], self._ln_x, n)
        dead = order[:m]
        self._dead_th.append(self._live_th.index_select(0, dead))
        self._dead_l.append(host[:m].copy())
        self._dead_lnw.append(ln_w)
        slots = torch.sort(dead).values
        surv = torch.sort(order[m:]).values
        su, sth, sl = (self._live_u.index_select(0, surv), self._live_th.index_select(0, surv),
                       self._live_l.index_select(0, surv))
        ns, stream, p = n - m, stream_of(self.device), C.byref(self._c_prior)
        wu, wth, wl, pu, pth, ok = self._wu, self._wth, self._wl, self._pu, self._pth, self._ok
        L.check(lib.cf_ns_walk_start(su.data_ptr(), sth.data_ptr(), sl.data_ptr(), ns, d, m, ns_key(self.seed, self._it, 0),
                                     wu.data_ptr(), wth.data_ptr(), wl.data_ptr(), stream))
        lstar_ptr = sorted_l.data_ptr() + (self.n_batch - 1) * sorted_l.element_size()
        for s in range(1, self.n_walk + 1):
            L.check(lib.cf_ns_propose(p, su.data_ptr(), ns, m, ns_key(self.seed, self._it, s), self.gamma, self.sigma,
                                      wu.data_ptr(), wth.data_ptr(), pu.data_ptr(), pth.data_ptr(), ok.data_ptr(), stream))
            lp = self._loglike(pth[:m])
            L.check(lib.cf_ns_accept(m, d, lstar_ptr, pu.data_ptr(), pth.data_ptr(), ok.data_ptr(), lp.data_ptr(),
                                     wu.data_ptr(), wth.data_ptr(), wl.data_ptr(), self._counts.data_ptr(), stream))
        self._n_walk_props += m * self.n_walk
        self._live_u.index_copy_(0, slots, wu[:m])
        self._live_th.index_copy_(0, slots, wth[:m])
        self._live_l.index_copy_(0, slots, wl[:m])

    # ---- nautilus's interface ----------------------------------------------------------------------------------------
    def run(self, f_live: float = 0.01, max_iterations: int = None, verbose: bool = False) -> bool:
        """Iterate until Z_live / Z < f_live (returns True) or until n_iterations reaches max_iterations (returns False).
        A second call continues from the current live set."""
        import torch

        if self._live_l is None:
            self._start()
        self._results = None
        while True:
            sorted_l, order = torch.sort(self._live_l, stable=True)
            host = sorted_l.cpu().numpy()  # the one host synchronisation of the iteration
            frac = live_fraction(self._ln_x, host, self._dead_lnw_all(), self.n_live)
            if verbose:
                print(f"nested: iteration {self._it:4d}  n_like {self._n_like:10d}  ln X {self._ln_x:9.3f}  "
                      f"Z_live/Z {frac:.3e}  L* {host[self.n_batch - 1]:.4f}")
            if frac < f_live:
                return True
            if max_iterations is not None and self._it >= max_iterations:
                return False
            self._iterate(sorted_l, order, host)

    def _dead_lnw_all(self) -> np.ndarray:
        return np.concatenate(self._dead_lnw) if self._dead_lnw else np.empty(0)

    def _final(self):
        """Dead points in death order, then the live points in index order: (theta [N, d], ln w [N], log L [N]) + summary."""
        if self._live_l is None:
            raise RuntimeError("run() the sampler first")
        if self._results is None:
            import torch

            live_l = self._live_l.cpu().numpy()
            ln_w = np.concatenate([self._dead_lnw_all(), live_log_weights(live_l, self._ln_x, self.n_live)])
            log_l = np.concatenate(self._dead_l + [live_l])
            theta = torch.cat(self._dead_th + [self._live_th]).cpu().numpy()
            self._results = (theta, ln_w, log_l, summarize(ln_w, log_l, self.n_live))
        return self._results

    def posterior(self):
        """(points [N, ndim], log_w [N], log_l [N]) as numpy float64: log_w normalised to logsumexp 0, zero-weight rows
        dropped (nautilus's ``posterior()`` without equal-weight resampling)."""
        theta, ln_w, log_l, s = self._final()
        keep = ln_w > -math.inf
        return theta[keep], ln_w[keep] - s["log_z"], log_l[keep]

    def _posterior_on_device(self):
        """(points [N, ndim], weights [N] = exp(log_w)) of ``posterior()`` as float64 tensors on the sampler's device, uploaded
        once per run (``run()`` drops the results they belong to)."""
        import torch

        self._final()
        if self._post_dev is None or self._post_dev[0] is not self._results:
            theta, log_w, _ = self.posterior()
            self._post_dev = (self._results, torch.from_numpy(np.ascontiguousarray(theta)).to(self.device),
                              torch.from_numpy(np.exp(log_w)).to(self.device))
        return self._post_dev[1], self._post_dev[2]

    def marginals(self, derived=None, **kw) -> dict:
        """``marginals.corner_data`` of the posterior points with weights exp(log_w): the numbers behind the weighted
        triangle plot of the nautilus scripts.  derived: a ``derived.Spec`` whose columns are appended to the sampled ones
        (``derived.augment``) -- the S8 / q0 / j0 / r_d columns of bao/desi_cmb_union3_fs8.py:282-294."""
        from . import marginals

        pts, w = self._posterior_on_device()
        if derived is not None:
            from . import derived as D

            pts = D.augment(derived, pts)
        return marginals.corner_data(pts, weights=w, **kw)

    def posterior_derived(self, spec):
        """(columns [N, n_q], weights [N]) on the sampler's device: ``derived.columns`` of the points of ``posterior()`` beside
        their weights exp(log_w), for ``marginals._weighted_quantile`` / ``weighted_mean_std`` / ``corner_data``."""
        from . import derived as D

        pts, w = self._posterior_on_device()
        return D.columns(spec, pts), w

    def fit_report(self, engine=None, **kw) -> dict:
        """``fit_report.chain_report`` of the posterior points with their weights exp(log_w): the residual block of the
        nautilus scripts (bao/desi_fs_lya.py:96-141, sn/pantheon_dipole_xyz.py:118-143) for every posterior point.  engine:
        the likelihood's ``LikelihoodEngine`` (default: the one behind ``engine.torch_log_prob()`` when that is the
        sampler's callable).  Keywords: block, thresholds, center, n_data."""
        from . import fit_report

        if "weights" in kw:
            raise TypeError("the nested sampler passes its own posterior weights")
        eng = fit_report.engine_of(self.log_likelihood, engine, "DeviceNestedSampler.fit_report")
        pts, w = self._posterior_on_device()
        return fit_report.chain_report(eng, pts, weights=w, **kw)

    def influence(self, engine=None, **kw) -> dict:
        """``influence.chain_report`` of the posterior points with their weights exp(log_w): which data carry the chi^2 of
        the posterior.  engine: as for ``fit_report``.  Keywords: block, thresholds."""
        from . import fit_report, influence

        if "weights" in kw:
            raise TypeError("the nested sampler passes its own posterior weights")
        eng = fit_report.engine_of(self.log_likelihood, engine, "DeviceNestedSampler.influence")
        pts, w = self._posterior_on_device()
        return influence.chain_report(eng, pts, weights=w, **kw)

    def leave_group_out(self, engine=None, **kw) -> dict:
        """``leaveout.chain_leave_group_out`` of the posterior points with their weights exp(log_w) as the base weights: per
        group of data the chi^2 it carries given the others and the posterior without it.  engine: as for ``fit_report``.
        Keywords: groups (required), block, columns, theta_ref, names."""
        from . import fit_report, leaveout

        if "weights" in kw:
            raise TypeError("the nested sampler passes its own posterior weights")
        eng = fit_report.engine_of(self.log_likelihood, engine, "DeviceNestedSampler.leave_group_out")
        pts, w = self._posterior_on_device()
        return leaveout.chain_leave_group_out(eng, pts, weights=w, **kw)

    def mean_std(self):
        """``marginals.weighted_mean_std`` of the same points and weights: (mean [ndim], std [ndim]) on the device, what the
        nautilus scripts print per parameter (getdist's ``mean`` and ``std``)."""
        from . import marginals

        pts, w = self._posterior_on_device()
        return marginals.weighted_mean_std(pts, w)

    @property
    def log_z(self) -> float:
        return self._final()[3]["log_z"]

    @property
    def log_z_err(self) -> float:
        return self._final()[3]["log_z_err"]

    @property
    def information(self) -> float:
        """H = sum p_i log L_i - log Z (nats)."""
        return self._final()[3]["h"]

    @property
    def n_eff(self) -> float:
        return self._final()[3]["n_eff"]

    @property
    def n_like(self) -> int:
        """Likelihood evaluations (rows passed to log_likelihood: the start and every walk step)."""
        return self._n_like

    @property
    def n_iterations(self) -> int:
        return self._it

    def walk_counts(self) -> dict:
        """Walk proposals and their fates (the accept kernel counts on the device: reading synchronises)."""
        acc, out, bad = (int(v) for v in self._counts.cpu().tolist())
        return dict(proposed=self._n_walk_props, accepted=acc, out_of_cube=out, nonfinite=bad)

    @property
    def acceptance(self) -> float:
        """Accepted / proposed steps of the constrained walk."""
        c = self.walk_counts()
        return c["accepted"] / max(c["proposed"], 1)
