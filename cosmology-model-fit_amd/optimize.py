"""
Batched box-constrained maximization on the GPU: best fits, fits with coordinates held fixed (the nested-model fits behind the
reference's Delta chi^2 significances) and profile likelihoods.  Each problem's finite-difference stencil and line-search trials
are rows of one likelihood call, so a thousand problems cost about as many calls as one.

Algorithm, as built.  The objective f is any torch callable theta [W, ndim] (cuda float64) -> [W] float64, e.g.
``lk.engine.torch_log_prob(CF_OUT_LOGL)`` or ``CF_OUT_LOGP``; it is MAXIMIZED inside the box [lo, hi].  ndim <= 16.  The free
coordinates are common to one call; every other coordinate keeps each problem's start value (a profile or a nested model).

* Coordinates.  u = (theta - lo) / (hi - lo), confined to [delta, 1 - delta] with delta = 2^-40: the box of the reference is open,
  so every row the objective sees, theta = lo + u (hi - lo), lies strictly inside it.
* Gradient.  Central differences with step h in u (default 1e-6: laplace.py's gradient step of 1e-6 box widths), two rows per
  free coordinate; within 2h of a face the inward one-sided second-order form (-3 f(u) + 4 f(u +- h) - f(u +- 2h)) / (+-2h).
* Direction.  Projected BFGS on -f with a dense n_free x n_free inverse-Hessian approximation H per problem.  A coordinate at a
  face whose gradient points out of the box is held (its gradient and direction are 0).  d = H pg; if pg.d <= 0 (not an ascent
  direction), H is reset to sigma I, sigma scaled so that the largest coordinate move is 10 % of the box at the first
  iteration and min(10 %, 4 x the last accepted step's largest move) later; after a failed search also at most 4^-K x the
  failed direction's largest move (the backtracking continued).  The update uses y = grad(-f) change on the
  coordinates that are not held (0 on the held ones) and is skipped when the curvature condition fails (s.y <= 0 or
  (s.y)^2 <= 1e-20 |s|^2 |y|^2).
* Line search.  K trial points P(u + alpha_k d), alpha_k = 4^-k, k < K (default 4), in one call; P clamps to [delta, 1 - delta].
  The largest alpha that passes Armijo, f_k >= f + c1 g.(u_k - u) with c1 = 1e-4, is taken; otherwise the best trial if it
  improves f.  "Improves" means by more than the rounding noise of f: f_k > f + 4 eps |f|.  If no trial improves f, H is reset
  once; if the search after that reset fails too, the problem stops.
* Statuses: CONVERGED (max |projected box-scaled gradient| <= gtol + gtol_rel |f|), NOISE_FLOOR (no ascent after a reset),
  ITER_CAP, NONFINITE_START (f of the start is not finite; the problem never moves), NONFINITE_STENCIL.  The finite-difference
  noise floor of the gradient is ~ eps |f| / h (eps = 2^-52): 2.2e-10 |f| at h = 1e-6.  The defaults gtol = 1e-5 and
  gtol_rel = 16 eps / h put the threshold 16 x above that floor at any |f| and, for |f| up to ~3e3, 1e-5 in units of f per box
  width: for a log-likelihood that is a shift below 1e-5 / lambda of the box along an axis whose curvature is lambda.
* Iteration: (1) cf_opt_stencil, (2) the likelihood on 2 n_free rows per active problem, (3) cf_opt_direction (gradient,
  convergence test, BFGS update, direction, K trial rows), (4) the likelihood on K rows per active problem, (5) cf_opt_accept,
  (6) cf_opt_compact drops the finished problems from the active list; the number still active is the one host read of the
  iteration (the next call's W).  All launches are asynchronous on torch's current stream.
* Each problem's arithmetic reads only its own rows, sums run in index order and no float atomics are used: with a
  batch-invariant objective (the engine is), a problem's result is bit-identical whatever else is in the batch and wherever it
  sits.
* Random starts: uniform in [delta, 1 - delta] from the ensemble's counter-based generator under ``opt_key(seed, purpose)``
  (a domain tag of its own), stream = coordinate, counter = start index: a seed always gives the same starts.

There is no tensor fallback: without the HIP library or a GPU the functions raise, after validating their arguments.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from ._args import require_gpu, stream_of
from .ensemble import _U64, _mix_int

# ---- random-stream keys ----------------------------------------------------------------------------------------------
_OPT_TAG = 0x4F5054494D495A31  # "OPTIMIZ1": the optimizer's domain tag (the nested sampler's is "NESTEDS1")
_GOLDEN = 0x9E3779B97F4A7C15
PURPOSE_BEST_FIT, PURPOSE_PROFILE = 0, 1


def opt_key(seed: int, purpose: int = PURPOSE_BEST_FIT) -> int:
    """Unsigned 64-bit key of stream 0 for the random starts of (seed, purpose); stream s (the coordinate) has key + s."""
    return _mix_int(_mix_int((seed * _GOLDEN + _OPT_TAG) & _U64) ^ (purpose & _U64))


RUNNING, CONVERGED, NOISE_FLOOR, ITER_CAP, NONFINITE_START, NONFINITE_STENCIL = range(6)
STATUS_NAMES = {RUNNING: "running", CONVERGED: "converged", NOISE_FLOOR: "noise_floor", ITER_CAP: "iteration_cap",
                NONFINITE_START: "nonfinite_start", NONFINITE_STENCIL: "nonfinite_stencil"}
MAX_NDIM = 16
MAX_TRIALS = 8
DELTA = 2.0 ** -40
EPS = 2.0 ** -52
DEFAULTS = dict(h=1e-6, n_trials=4, gtol=1e-5, gtol_rel=None, max_iter=200, c1=1e-4)

__all__ = ["maximize", "best_fit", "profile", "sigma_from_delta_chi2", "crossings", "opt_key", "OptimizeResult", "FitResult",
           "ProfileResult", "STATUS_NAMES"]


def sigma_from_delta_chi2(dchi2: float, k: int = 1) -> float:
    """Likelihood-ratio significance of Delta chi^2 for k extra parameters: the two-sided normal quantile of the chi^2_k
    tail probability.  For k = 1 this is sqrt(Delta chi^2), the convention of the reference's comments."""
    dchi2, k = float(dchi2), int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    if not dchi2 > 0.0:
        return 0.0
    if k == 1:
        return math.sqrt(dchi2)
    from scipy import stats

    return float(stats.norm.isf(0.5 * stats.chi2.sf(dchi2, k)))


def crossings(grid, dchi2, level: float = 1.0):
    """(lo, hi) where a 1-D Delta chi^2 profile crosses `level` on each side of its minimum, by linear interpolation between
    grid points; None on a side where it does not cross inside the grid (a profile truncated by the prior)."""
    x, d = np.asarray(grid, dtype=np.float64), np.asarray(dchi2, dtype=np.float64)
    if x.ndim != 1 or x.shape != d.shape or x.size < 2:
        raise ValueError("grid and dchi2 must be 1-D of the same length >= 2")
    d = np.where(np.isnan(d), np.inf, d)
    i0 = int(np.argmin(d))

    def cross(a, b):  # d[a] < level <= d[b]
        return float(x[a] + (level - d[a]) * (x[b] - x[a]) / (d[b] - d[a])) if np.isfinite(d[b]) else float(x[a])

    lo = hi = None
    for i in range(i0, 0, -1):
        if d[i - 1] >= level:
            lo = cross(i, i - 1)
            break
    for i in range(i0, x.size - 1):
        if d[i + 1] >= level:
            hi = cross(i, i + 1)
            break
    return lo, hi


# ---- results ---------------------------------------------------------------------------------------------------------
@dataclass
class OptimizeResult:
    """B problems (numpy): x [B, ndim], log_prob [B], status [B], n_iter [B], grad_norm [B] (max |projected box-scaled
    gradient| at the end; inf for a non-finite start), x0 [B, ndim] (the start rows the objective saw), plus n_like (total
    likelihood rows), n_calls (likelihood calls) and iterations (device iterations)."""
    x: np.ndarray
    log_prob: np.ndarray
    status: np.ndarray
    n_iter: np.ndarray
    grad_norm: np.ndarray
    x0: np.ndarray
    n_like: int
    n_calls: int
    iterations: int

    @property
    def converged(self) -> np.ndarray:
        return (self.status == CONVERGED) | (self.status == NOISE_FLOOR)

    def status_counts(self) -> dict:
        return {STATUS_NAMES[s]: int(np.sum(self.status == s)) for s in STATUS_NAMES if s != RUNNING}


@dataclass
class FitResult:
    """The best converged problem (ties: the lowest start index) and all problems.  ``best_converged`` is False when no
    problem converged (then the best finite one is reported)."""
    x: np.ndarray
    log_prob: float
    status: int
    index: int
    best_converged: bool
    problems: OptimizeResult

    @property
    def chi2(self) -> float:
        """-2 log_prob: chi^2 when the objective is log L = -chi^2 / 2."""
        return -2.0 * self.log_prob


@dataclass
class ProfileResult:
    """values [G] or [G1, G2] (the best converged start per grid point), x [..., ndim] (its argmax theta), status [...],
    delta_chi2 = 2 (max - values) with max the larger of the best fit and the grid maximum, the best fit, all problems."""
    index: tuple
    grid: tuple
    values: np.ndarray
    x: np.ndarray
    status: np.ndarray
    delta_chi2: np.ndarray
    log_prob_max: float
    best: FitResult
    problems: OptimizeResult

    def interval(self, delta_chi2: float = 1.0):
        """1-D profiles: (lo, hi) of {Delta chi^2 < delta_chi2} by linear interpolation between grid points; None on a side
        where the profile does not cross inside the grid (truncated by the prior)."""
        if len(self.index) != 1:
            raise ValueError("interval() is defined for 1-D profiles")
        return crossings(self.grid[0], self.delta_chi2, delta_chi2)


# ---- argument handling (before any device check, so the CPU tests reach it) ----------------------------------------
def _bounds(bounds) -> np.ndarray:
    b = np.asarray(bounds, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 2 or b.shape[0] < 1:
        raise ValueError(f"bounds must be [ndim, 2], got shape {b.shape}")
    if b.shape[0] > MAX_NDIM:
        raise ValueError(f"the optimizer takes at most {MAX_NDIM} parameters, got {b.shape[0]}")
    if not (np.all(np.isfinite(b)) and np.all(b[:, 0] < b[:, 1])):
        raise ValueError("bounds must be finite with lo < hi")
    return b


def _options(h, n_trials, gtol, gtol_rel, max_iter, c1) -> dict:
    if not (0.0 < h <= 0.01):
        raise ValueError("h must be in (0, 0.01]")
    if not (1 <= int(n_trials) <= MAX_TRIALS):
        raise ValueError(f"n_trials must be in 1..{MAX_TRIALS}")
    if not (gtol >= 0.0 and math.isfinite(gtol)):
        raise ValueError("gtol must be finite and >= 0")
    gtol_rel = 16.0 * EPS / h if gtol_rel is None else float(gtol_rel)
    if not (gtol_rel >= 0.0 and math.isfinite(gtol_rel)):
        raise ValueError("gtol_rel must be finite and >= 0")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1")
    if not (0.0 < c1 < 1.0):
        raise ValueError("c1 must be in (0, 1)")
    return dict(h=float(h), n_trials=int(n_trials), gtol=float(gtol), gtol_rel=gtol_rel, max_iter=int(max_iter), c1=float(c1))


def _index(i, ndim: int) -> int:
    if isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)):
        raise ValueError(f"parameter index must be an int, got {i!r}")
    if not 0 <= int(i) < ndim:
        raise ValueError(f"parameter index {i} out of range for ndim = {ndim}")
    return int(i)


def _free_list(free, ndim: int) -> list:
    if free is None:
        return list(range(ndim))
    idx = sorted(_index(i, ndim) for i in free)
    if not idx or len(set(idx)) != len(idx):
        raise ValueError("free must list distinct parameter indices, at least one")
    return idx


def _as_rows(x0, ndim: int) -> np.ndarray:
    try:
        import torch

        if isinstance(x0, torch.Tensor):
            x0 = x0.detach().to("cpu", torch.float64).numpy()
    except ImportError:
        pass
    a = np.array(x0, dtype=np.float64, ndmin=2)
    if a.ndim != 2 or a.shape[1] != ndim or a.shape[0] < 1:
        raise ValueError(f"x0 must be [B, {ndim}], got shape {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError("x0 must be finite")
    return np.ascontiguousarray(a)


def _params(b: np.ndarray, free: list, o: dict):
    from . import _lib as L

    p = L.cf_opt_params()
    p.ndim, p.n_free = b.shape[0], len(free)
    for j, c in enumerate(free):
        p.free_idx[j] = c
    for c in range(b.shape[0]):
        p.lo[c], p.width[c] = b[c, 0], b[c, 1] - b[c, 0]
    p.h, p.delta, p.c1, p.gtol, p.gtol_rel = o["h"], DELTA, o["c1"], o["gtol"], o["gtol_rel"]
    p.n_trials, p.max_iter = o["n_trials"], o["max_iter"]
    return p


# ---- the device loop -------------------------------------------------------------------------------------------------
class _State:
    """Per-problem device state (cf_opt_state) of B problems."""

    def __init__(self, B: int, ndim: int, device):
        import torch

        f64, i32, M = dict(dtype=torch.float64, device=device), dict(dtype=torch.int32, device=device), MAX_NDIM
        self.u, self.f = torch.empty((B, ndim), **f64), torch.empty(B, **f64)
        self.g, self.g_prev, self.s, self.d = (torch.zeros((B, M), **f64) for _ in range(4))
        self.hinv = torch.zeros((B, M, M), **f64)
        self.gnorm = torch.full((B,), math.inf, **f64)
        self.form = torch.zeros((B, M), dtype=torch.int8, device=device)
        self.status, self.n_iter = torch.zeros(B, **i32), torch.zeros(B, **i32)
        from . import _lib as L

        self.flags = torch.full((B,), L.CF_OPT_NEED_RESET, **i32)

    def c_struct(self):
        from . import _lib as L

        s = L.cf_opt_state()
        for name in ("u", "f", "g", "g_prev", "s", "hinv", "d", "gnorm", "form", "status", "n_iter", "flags"):
            setattr(s, name, getattr(self, name).data_ptr())
        return s


def _call(log_prob, theta, problem=None):
    import torch

    out = log_prob(theta) if problem is None else log_prob(theta, problem)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.device == theta.device and
            out.shape == (theta.shape[0],)):
        raise ValueError("log_prob must return a float64 tensor [W] on the device of theta")
    return out.contiguous()


def _run(log_prob, p, u, theta, L, lib, problem_index: bool = False) -> OptimizeResult:
    """Iterate from the start rows u / theta [B, ndim] (device) until every problem has a status.  problem_index: the objective
    is called as log_prob(theta, problem) with the int32 problem index of every row (see ``maximize``)."""
    import torch

    B, d, nf, K = u.shape[0], p.ndim, p.n_free, p.n_trials
    dev = u.device
    stream = stream_of(dev)
    st = _State(B, d, dev)
    st.u.copy_(u)
    f = _call(log_prob, theta, torch.arange(B, dtype=torch.int32, device=dev) if problem_index else None)
    fin = torch.isfinite(f)
    st.f.copy_(torch.where(fin, f, torch.full_like(f, -math.inf)))
    st.status.copy_(torch.where(fin, 0, NONFINITE_START).to(torch.int32))
    cs, pp = st.c_struct(), C.byref(p)
    ps = C.byref(cs)
    act = torch.nonzero(fin).reshape(-1).to(torch.int32)
    nxt = torch.empty(B, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = torch.empty((B * 2 * nf, d), dtype=torch.float64, device=dev)
    trials = torch.empty((B * K, d), dtype=torch.float64, device=dev)
    n_act, n_like, n_calls, iterations = int(act.numel()), B, 1, 0
    while n_act > 0:
        L.check(lib.cf_opt_stencil(pp, ps, act.data_ptr(), n_act, rows.data_ptr(), stream))
        fs = _call(log_prob, rows[: n_act * 2 * nf], act[:n_act].repeat_interleave(2 * nf) if problem_index else None)
        L.check(lib.cf_opt_direction(pp, ps, act.data_ptr(), n_act, fs.data_ptr(), trials.data_ptr(), stream))
        ft = _call(log_prob, trials[: n_act * K], act[:n_act].repeat_interleave(K) if problem_index else None)
        L.check(lib.cf_opt_accept(pp, ps, act.data_ptr(), n_act, ft.data_ptr(), stream))
        L.check(lib.cf_opt_compact(act.data_ptr(), n_act, st.status.data_ptr(), nxt.data_ptr(), count.data_ptr(), stream))
        n_like += n_act * (2 * nf + K)
        n_calls += 2
        iterations += 1
        act, nxt = nxt, act
        n_act = int(count.item())  # the one host read of the iteration
    lo = torch.tensor(np.ctypeslib.as_array(p.lo)[:d], dtype=torch.float64, device=dev)
    w = torch.tensor(np.ctypeslib.as_array(p.width)[:d], dtype=torch.float64, device=dev)
    x = st.u * w + lo
    return OptimizeResult(x=x.cpu().numpy(), log_prob=st.f.cpu().numpy(), status=st.status.cpu().numpy().astype(np.int64),
                          n_iter=st.n_iter.cpu().numpy().astype(np.int64), grad_norm=st.gnorm.cpu().numpy(),
                          x0=theta.cpu().numpy(), n_like=n_like, n_calls=n_calls, iterations=iterations)


def _starts(p, x0: np.ndarray, key: Optional[int], L, lib):
    """Device u / theta of the rows of x0: free coordinates drawn (key given) or converted from x0, fixed ones from x0."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy(np.ascontiguousarray(x0)).to(dev)
    u, th = torch.empty_like(x), torch.empty_like(x)
    L.check(lib.cf_opt_starts(C.byref(p), x.shape[0], x.data_ptr(), 0 if key is None else key, 0 if key is None else 1,
                              u.data_ptr(), th.data_ptr(), stream_of(dev)))
    return u, th


# ---- public interface ------------------------------------------------------------------------------------------------
def maximize(log_prob: Callable, bounds, x0, *, free=None, h=1e-6, n_trials=4, gtol=1e-5, gtol_rel=None, max_iter=200,
             c1=1e-4, problem_index=False) -> OptimizeResult:
    """Maximise log_prob from the B start rows x0 [B, ndim] (tensor or array) inside the box bounds [ndim, 2].  free: the
    indices that move (default all); the others keep each row's value (the objective sees lo + u (hi - lo) with u clamped to
    [2^-40, 1 - 2^-40], the same value within an ulp or two).

    problem_index=True: every problem has an objective of its own (``mocks.MockSet``: a data set per problem).  The objective
    is then called as ``log_prob(theta, problem)`` with ``problem`` an int32 device tensor [rows], the problem each row belongs
    to: ``arange(B)`` for the start rows; for the stencil rows every entry of the active list repeated 2 n_free times (a
    problem's rows are consecutive); for the trial rows every entry repeated n_trials times."""
    b = _bounds(bounds)
    ndim = b.shape[0]
    fr = _free_list(free, ndim)
    o = _options(h, n_trials, gtol, gtol_rel, max_iter, c1)
    x = _as_rows(x0, ndim)
    L, lib = require_gpu("optimize.maximize")
    p = _params(b, fr, o)
    u, th = _starts(p, x, None, L, lib)
    return _run(log_prob, p, u, th, L, lib, bool(problem_index))


def _best_of(res: OptimizeResult, idx=None):
    """Index of the best converged problem among idx (ties: the lowest index), else of the best finite one."""
    idx = np.arange(res.status.size) if idx is None else np.asarray(idx)
    f = res.log_prob[idx]
    conv = res.converged[idx]
    if np.any(conv):
        return int(idx[np.argmax(np.where(conv, f, -np.inf))]), True
    fin = np.isfinite(f)
    return (int(idx[np.argmax(np.where(fin, f, -np.inf))]) if np.any(fin) else int(idx[0])), False


def _fixed(fixed, ndim: int, b: np.ndarray) -> dict:
    out = {}
    for k, v in (fixed or {}).items():
        i, v = _index(k, ndim), float(v)
        if not (b[i, 0] < v < b[i, 1]):
            raise ValueError(f"fixed value {v} of parameter {i} is not strictly inside ({b[i, 0]}, {b[i, 1]})")
        out[i] = v
    if len(out) >= ndim:
        raise ValueError("every parameter is fixed: nothing to maximise")
    return out


def best_fit(log_prob: Callable, bounds, *, n_starts=32, seed=0, x0=None, fixed=None, problem_index=False, **options) -> FitResult:
    """Multi-start maximization: the rows of x0 (e.g. the top log P rows of a device chain) first, then n_starts uniform
    random starts of ``seed``.  fixed = {index: value} holds those coordinates (the nested-model fit, e.g. {2: 0.0} for
    v = 0).  Returns the best converged problem (ties: the lowest start index) and all problems.  problem_index: as in
    ``maximize`` (the problem is the start)."""
    b = _bounds(bounds)
    ndim = b.shape[0]
    fx = _fixed(fixed, ndim, b)
    o = _options(**{**DEFAULTS, **options})
    n_starts = int(n_starts)
    if n_starts < 0:
        raise ValueError("n_starts must be >= 0")
    given = _as_rows(x0, ndim) if x0 is not None else np.empty((0, ndim))
    if given.shape[0] + n_starts < 1:
        raise ValueError("best_fit needs at least one start")
    fr = [i for i in range(ndim) if i not in fx]
    rand = np.tile(0.5 * (b[:, 0] + b[:, 1]), (n_starts, 1))
    for i, v in fx.items():
        given[:, i], rand[:, i] = v, v
    L, lib = require_gpu("optimize.best_fit")
    import torch

    p = _params(b, fr, o)
    parts = []
    if given.shape[0]:
        parts.append(_starts(p, given, None, L, lib))
    if n_starts:
        parts.append(_starts(p, rand, opt_key(seed, PURPOSE_BEST_FIT), L, lib))
    u, th = torch.cat([q[0] for q in parts]), torch.cat([q[1] for q in parts])
    res = _run(log_prob, p, u, th, L, lib, bool(problem_index))
    k, ok = _best_of(res)
    return FitResult(x=res.x[k].copy(), log_prob=float(res.log_prob[k]), status=int(res.status[k]), index=k, best_converged=ok,
                     problems=res)


def profile(log_prob: Callable, bounds, index, grid, *, n_starts=8, seed=0, best: FitResult = None, problem_index=False,
            **options) -> ProfileResult:
    """Profile likelihood: at every grid point the profiled coordinates are held at the grid values and the rest maximised.
    1-D: index int, grid 1-D -> [G]; 2-D: index pair, grid pair (g1, g2) -> [G1, G2].  Start 0 of every grid point is the
    global best fit (``best``, computed with 32 starts of ``seed`` when not given) with the profiled coordinates overwritten;
    starts 1 .. n_starts - 1 are random.  All G x n_starts problems run as one batch.  problem_index: as in ``maximize``
    (problem p is start p % n_starts of grid point p // n_starts)."""
    b = _bounds(bounds)
    ndim = b.shape[0]
    if isinstance(index, (tuple, list)):
        if len(index) != 2:
            raise ValueError("a 2-D profile takes an index pair")
        idx = (_index(index[0], ndim), _index(index[1], ndim))
        if idx[0] == idx[1]:
            raise ValueError("the two profiled indices must differ")
        if not (isinstance(grid, (tuple, list)) and len(grid) == 2):
            raise ValueError("a 2-D profile takes two grids")
        grids = tuple(np.asarray(g_, dtype=np.float64) for g_ in grid)
    else:
        idx = (_index(index, ndim),)
        grids = (np.asarray(grid, dtype=np.float64),)
    for i, g_ in zip(idx, grids):
        if g_.ndim != 1 or g_.size < 1:
            raise ValueError("every grid must be 1-D and non-empty")
        if not np.all((g_ > b[i, 0]) & (g_ < b[i, 1])):
            raise ValueError(f"grid values of parameter {i} must lie strictly inside ({b[i, 0]}, {b[i, 1]})")
    if len(idx) >= ndim:
        raise ValueError("a profile over every parameter leaves nothing to maximise")
    n_starts = int(n_starts)
    if n_starts < 1:
        raise ValueError("n_starts must be >= 1")
    o = _options(**{**DEFAULTS, **options})
    L, lib = require_gpu("optimize.profile")
    import torch

    if best is None:
        best = best_fit(log_prob, b, n_starts=32, seed=seed, problem_index=problem_index, **options)
    shape = tuple(g_.size for g_ in grids)
    pts = np.stack([m.reshape(-1) for m in np.meshgrid(*grids, indexing="ij")], axis=1)  # [P, len(idx)]
    P = pts.shape[0]
    x0 = np.tile(np.asarray(best.x, dtype=np.float64), (P * n_starts, 1))
    x0[:, list(idx)] = np.repeat(pts, n_starts, axis=0)
    fr = [i for i in range(ndim) if i not in idx]
    p = _params(b, fr, o)
    u, th = _starts(p, x0, opt_key(seed, PURPOSE_PROFILE), L, lib)
    u0, th0 = _starts(p, x0[::n_starts], None, L, lib)
    u[::n_starts], th[::n_starts] = u0, th0
    res = _run(log_prob, p, u.contiguous(), th.contiguous(), L, lib, bool(problem_index))
    pick = np.array([_best_of(res, np.arange(q * n_starts, (q + 1) * n_starts))[0] for q in range(P)])
    values = res.log_prob[pick]
    fin = values[np.isfinite(values)]
    fmax = max(best.log_prob, float(fin.max())) if fin.size else best.log_prob
    return ProfileResult(index=idx, grid=grids, values=values.reshape(shape), x=res.x[pick].reshape(shape + (ndim,)),
                         status=res.status[pick].reshape(shape), delta_chi2=(2.0 * (fmax - values)).reshape(shape),
                         log_prob_max=fmax, best=best, problems=res)
