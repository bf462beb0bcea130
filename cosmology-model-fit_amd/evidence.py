"""
Bridge-sampling evidence from a chain that lives on the device: ln Z of a posterior in a finite box, with an error estimate.

``laplace.log_evidence`` integrates a Gaussian around the MAP over all space, which is wrong by ln 2 per parameter whose posterior
is cut by a wall of the box (the thawing fits' w0, the velocity step, fcc).  The bridge estimator (Meng & Wong 1996; Gronau et al.
2017) needs only the chain already held plus N2 draws from a Gaussian fitted to it, and evaluates the real posterior at those
draws, so walls, skewness and points outside the box (-inf) are handled by construction.

Definitions (tests/bridge_reference.py restates them in long double):

* Split: the first half of the samples along the leading axis (for a chain [n_t, W, ndim]: the first n_t // 2 steps of all
  walkers) fits the proposal; the second half, N1 rows, enters the iteration.
* Unbounded coordinates: u = (theta - lo) / (hi - lo), phi = log u - log1p(-u), log J = sum_k [log(hi_k - lo_k) + log u_k +
  log1p(-u_k)]; q(phi) = P*(theta(phi)) J.
* Proposal: mu and the unbiased covariance of the fit half's phi (torch, float64, on the device), R its lower Cholesky factor,
  z = R^-1 (phi - mu), log g(z) = -|z|^2 / 2 - (d / 2) log 2 pi.
* method="normal": l = log q(phi) + log det R - log g(z) at the N1 samples (l1) and at phi~ = mu + R z~ for N2 draws z~ (l2).
  method="warp3": q~(z) = [q(mu + R z) + q(mu - R z)] det R / 2 in place of q det R, for both sets.
* Draws: z~[j, k] = the ensemble generator's normal from streams 2k, 2k + 1 of ``bridge_key(seed)``, counter j.
* Fixed point and error: ``cf_bridge_solve`` (include/cosmofit.h) with l* = the lower median of l1, s1 = n_eff / (n_eff + N2),
  s2 = N2 / (n_eff + N2); ln Z = log r + l*; RE^2 = Var(f1) / (N2 mean(f1)^2) + tau_f Var(f2) / (N1 mean(f2)^2)
  (Fruehwirth-Schnatter 2004), ``log_z_err`` = sqrt(RE^2).
* Autocorrelation: for a chain, n_eff = N1 / max(1, max_k tau_k) with tau = ``chain_stats.integrated_time`` of the second
  half, and tau_f that of the f2 series [n_t2, W, 1]; for flat samples n_eff = N1 and tau_f = 1 unless ``n_eff=`` is given
  (then tau_f = N1 / n_eff).  ``tau_reliable`` is False when a series was shorter than emcee's 50 tau.

The transforms, the draws and the fixed point are csrc/cosmofit_bridge.hip; torch forms the moments and adds the pieces of l.
There is no tensor fallback: without the HIP library or a GPU ``bridge`` raises, after validating its arguments.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from . import _args
from .ensemble import _U64, _mix_int

_BRIDGE_TAG = 0x4252494447455331  # "BRIDGES1": the domain tag of the proposal draws (the optimizer's is "OPTIMIZ1")
_GOLDEN = 0x9E3779B97F4A7C15
MAX_NDIM = 16
CONVERGED, ITER_CAP, NONFINITE = range(3)
STATUS_NAMES = {CONVERGED: "converged", ITER_CAP: "iteration_cap", NONFINITE: "nonfinite"}
METHODS = ("normal", "warp3")
_AUTOCORR_TOL = 50  # emcee's criterion: a tau from fewer than 50 tau steps is not reliable

__all__ = ["bridge", "log_bayes_factor", "bridge_key", "BridgeResult", "STATUS_NAMES", "METHODS"]


def bridge_key(seed: int) -> int:
    """Unsigned 64-bit key of stream 0 of the proposal draws of ``seed``; coordinate k uses streams 2k and 2k + 1."""
    return _mix_int(_mix_int((seed * _GOLDEN + _BRIDGE_TAG) & _U64))


@dataclass
class BridgeResult:
    """What ``bridge`` returns.  log_z +- log_z_err; status: ``STATUS_NAMES``; n_iter: updates of the fixed point; n_fit /
    n_iter_rows (N1) / n_draws (N2): rows of the fit half, the iteration half and the proposal; n_eff, tau_f, tau_reliable: see
    the module text; n_like: objective rows spent; mean [d], chol [d, d]: the proposal in unbounded coordinates (numpy); l1
    [N1], l2 [N2], f2 [N1]: device tensors."""
    log_z: float
    log_z_err: float
    status: int
    n_iter: int
    method: str
    n_fit: int
    n_iter_rows: int
    n_draws: int
    n_eff: float
    tau_f: float
    tau_reliable: bool
    n_like: int
    mean: np.ndarray
    chol: np.ndarray
    l1: object
    l2: object
    f2: object

    @property
    def converged(self) -> bool:
        return self.status == CONVERGED


def log_bayes_factor(a: BridgeResult, b: BridgeResult) -> Tuple[float, float]:
    """(ln Z_a - ln Z_b, its error): the two estimates are independent, so their errors add in quadrature."""
    return a.log_z - b.log_z, math.hypot(a.log_z_err, b.log_z_err)


# ---- argument checks (no device needed) -------------------------------------------------------------------------------------
def _is_tensor(x) -> bool:
    return isinstance(x, torch.Tensor)


def _rows(x, what: str):
    """A float64 torch tensor or numpy array, as it is."""
    if _is_tensor(x):
        if x.dtype != torch.float64:
            raise ValueError(f"bridge takes {what} as float64")
        return x
    a = np.asarray(x)
    if a.dtype != np.float64:
        raise ValueError(f"bridge takes {what} as float64")
    return a


def _box(lo, hi):
    lo, hi = (np.asarray(v.detach().cpu().numpy() if _is_tensor(v) else v, dtype=np.float64).reshape(-1) for v in (lo, hi))
    if lo.shape != hi.shape or not 1 <= lo.size <= MAX_NDIM:
        raise ValueError(f"bridge takes the box as lo, hi [ndim] with 1 <= ndim <= {MAX_NDIM}")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all() and np.isfinite(hi - lo).all()):
        raise ValueError("bridge needs a finite box with lo < hi in every coordinate (unbounded priors are out of scope)")
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def _int(v, name: str, low: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
        raise ValueError(f"{name} must be an integer >= {low}")
    return int(v)


def _validate(log_prob, samples, lo, hi, log_probs, method, n_draws, n_eff, seed, tol, max_iter, chunk):
    if not callable(log_prob):
        raise ValueError("bridge takes log_prob as a callable theta [W, ndim] -> [W]")
    lo, hi = _box(lo, hi)
    d = lo.size
    x = _rows(samples, "the samples")
    if x.ndim not in (2, 3) or x.shape[-1] != d:
        raise ValueError(f"bridge takes samples [n_t, W, {d}] (a chain) or [n, {d}] (flat): the last axis is the box's ndim")
    lead = tuple(x.shape[:-1])
    if log_probs is not None:
        lp = _rows(log_probs, "log_probs")
        if tuple(lp.shape) != lead:
            raise ValueError(f"log_probs must have the samples' leading shape {list(lead)}")
        if _is_tensor(lp) != _is_tensor(x) or (_is_tensor(x) and lp.device != x.device):
            raise ValueError("log_probs must live where the samples live")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}")
    n_lead = lead[0]
    per = lead[1] if len(lead) == 2 else 1
    n_fit, n1 = (n_lead // 2) * per, (n_lead - n_lead // 2) * per
    need = 4 * (d + 1)
    if n_fit < need or n1 < need:
        raise ValueError(f"bridge needs at least 4 (ndim + 1) = {need} rows in each half of the samples (got {n_fit} and {n1})")
    n2 = n1 if n_draws is None else _int(n_draws, "n_draws", 1)
    if n_eff is not None:
        if isinstance(n_eff, bool) or not isinstance(n_eff, (int, float, np.integer, np.floating)) or not 0.0 < float(n_eff) <= n1 \
                or not math.isfinite(float(n_eff)):
            raise ValueError("n_eff must be a number in (0, N1]")
        n_eff = float(n_eff)
    seed = _int(seed, "seed", 0)
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0")
    max_iter = _int(max_iter, "max_iter", 1)
    if max_iter > 2**31 - 1:
        raise ValueError("max_iter must fit in 32 bits")
    chunk = _int(chunk, "chunk", 1)
    return lo, hi, d, x, lead, n_fit, n1, n2, n_eff, seed, float(tol), max_iter, chunk


def _require_gpu():  # a module attribute: a test answers for the device through it
    return _args.require_gpu("evidence.bridge")


def _cholesky(cov: np.ndarray) -> np.ndarray:
    """The lower Cholesky factor, column by column; a column whose pivot is not > 0 is named."""
    d = cov.shape[0]
    R = np.zeros((d, d))
    for k in range(d):
        pivot = cov[k, k] - float(R[k, :k] @ R[k, :k])
        if not (math.isfinite(pivot) and pivot > 0.0):
            raise ValueError(f"the covariance of the fit half is degenerate in column {k} of the unbounded coordinates (pivot "
                             f"{pivot:.3g}): the proposal has no Cholesky factor; is parameter {k} constant or a function of "
                             "the others?")
        R[k, k] = math.sqrt(pivot)
        for i in range(k + 1, d):
            R[i, k] = (cov[i, k] - float(R[i, :k] @ R[k, :k])) / R[k, k]
    return R


# ---- the device pieces ------------------------------------------------------------------------------------------------------
class _Device:
    def __init__(self, L, lib, device, lo, hi):
        self.L, self.lib, self.device, self.lo, self.hi, self.d = L, lib, device, lo, hi, lo.size
        self.torch = torch

    def forward(self, theta, mean, chol):
        t = self.torch
        n = theta.shape[0]
        z = t.empty((n, self.d), dtype=t.float64, device=self.device)
        lj = t.empty(n, dtype=t.float64, device=self.device)
        self.L.check(self.lib.cf_bridge_forward(theta.data_ptr(), n, self.d, _args.ptr(self.lo), _args.ptr(self.hi), _args.ptr(mean), _args.ptr(chol),
                                                z.data_ptr(), lj.data_ptr(), _args.stream_of(self.device)))
        return z, lj

    def points(self, z, mean, chol, mirror: int):
        t = self.torch
        n = z.shape[0]
        theta = t.empty((n, self.d), dtype=t.float64, device=self.device)
        lj = t.empty(n, dtype=t.float64, device=self.device)
        self.L.check(self.lib.cf_bridge_points(z.data_ptr(), n, self.d, _args.ptr(self.lo), _args.ptr(self.hi), _args.ptr(mean), _args.ptr(chol), int(mirror),
                                               theta.data_ptr(), lj.data_ptr(), _args.stream_of(self.device)))
        return theta, lj

    def draw(self, key: int, first: int, n: int):
        t = self.torch
        z = t.empty((n, self.d), dtype=t.float64, device=self.device)
        self.L.check(self.lib.cf_bridge_draw(key, first, n, self.d, z.data_ptr(), _args.stream_of(self.device)))
        return z

    def solve(self, l1, l2, lstar, s1, s2, tol, max_iter):
        t = self.torch
        rec = t.empty(self.L.CF_BRIDGE_RESULT_DOUBLES, dtype=t.float64, device=self.device)
        f2 = t.empty(l1.shape[0], dtype=t.float64, device=self.device)
        self.L.check(self.lib.cf_bridge_solve(l1.data_ptr(), l1.shape[0], l2.data_ptr(), l2.shape[0], lstar, s1, s2, tol, max_iter,
                                              rec.data_ptr(), f2.data_ptr(), _args.stream_of(self.device)))
        return dict(zip(self.L.BRIDGE_RESULT, rec.cpu().tolist())), f2  # the one host read of the solve


def _objective(log_prob, theta, chunk: int):
    """log_prob over theta [n, d] in calls of at most ``chunk`` rows."""
    outs = []
    for a in range(0, theta.shape[0], chunk):
        rows = theta[a:a + chunk].contiguous()
        out = log_prob(rows)
        if not isinstance(out, torch.Tensor) or out.shape != (rows.shape[0],) or out.dtype != torch.float64:
            raise ValueError("log_prob must map a float64 tensor [W, ndim] to a float64 tensor [W]")
        outs.append(out)
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def _tau(series, floor_one: bool = True):
    """(max over the dimensions of emcee's integrated time of a device chain [n_t, W, k], floored at 1; reliable?)."""
    from . import chain_stats

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tau = np.asarray(chain_stats.integrated_time(series, tol=_AUTOCORR_TOL, quiet=True), dtype=np.float64)
    ok = np.isfinite(tau)
    reliable = bool(ok.all() and (_AUTOCORR_TOL * tau <= series.shape[0]).all())
    return max(1.0, float(tau[ok].max())) if ok.any() else 1.0, reliable


def bridge(log_prob: Callable, samples, lo, hi, log_probs=None, method: str = "normal", n_draws: Optional[int] = None,
           n_eff: Optional[float] = None, seed: int = 0, tol: float = 1e-10, max_iter: int = 1000, chunk: int = 65536) -> BridgeResult:
    """ln Z = log of the integral of exp(log_prob) over the box [lo, hi], by bridge sampling.

    log_prob: torch callable theta [W, ndim] (cuda float64) -> [W], the unnormalised log posterior, -inf outside the box
    (``engine.torch_log_prob()``, ``gp.torch_log_prob()``); with the engine's normalised box prior Z is the evidence the nested
    sampler reports.  samples: [n_t, W, ndim] (a device chain, ``get_chain()``) or flat [n, ndim]; log_probs: their recorded log
    posterior of the same leading shape (``get_log_prob()``), which saves re-evaluating the N1 iteration rows.  Tensors on the
    GPU are used where they are; CPU tensors and numpy arrays are uploaded to the current device.  method: "normal" or "warp3"
    (the symmetrised mixture: smaller error on skewed targets for N1 + 2 N2 objective rows).  n_draws: N2 (default N1).
    n_eff: the effective size of the iteration half (default: from the autocorrelation of a chain; N1 for flat samples).
    The objective is called with at most ``chunk`` rows.

    ValueError: a wrong argument (raised before a device is asked for), a sample that is not strictly inside the box or whose
    log posterior is not finite, a degenerate covariance.  A NaN from the objective at a draw gives status NONFINITE."""
    lo, hi, d, x, lead, n_fit, n1, n2, n_eff_arg, seed, tol, max_iter, chunk = _validate(
        log_prob, samples, lo, hi, log_probs, method, n_draws, n_eff, seed, tol, max_iter, chunk)
    L, lib = _require_gpu()
    if isinstance(x, torch.Tensor) and x.is_cuda:
        device = x.device
    else:
        device = torch.device("cuda", torch.cuda.current_device())
    as_dev = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(device)
    x = as_dev(x)
    lp = None if log_probs is None else as_dev(_rows(log_probs, "log_probs"))
    n_lead = lead[0]
    half = n_lead // 2
    with torch.cuda.device(device):
        dev = _Device(L, lib, device, lo, hi)
        fit = x[:half].reshape(n_fit, d).contiguous()
        it = x[half:].reshape(n1, d).contiguous()
        zero, eye = np.zeros(d), np.ascontiguousarray(np.eye(d))
        phi, _ = dev.forward(fit, zero, eye)  # mean 0, factor 1: z is phi itself
        if not bool(torch.isfinite(phi).all()):
            raise ValueError("bridge: a sample of the fit half is not strictly inside the box (or is NaN)")
        mu_dev = phi.mean(dim=0)
        pc = phi - mu_dev
        cov_dev = (pc.T @ pc) / (n_fit - 1)
        host = torch.cat([mu_dev, cov_dev.reshape(-1)]).cpu().numpy()
        mean, cov = np.ascontiguousarray(host[:d]), host[d:].reshape(d, d)
        chol = np.ascontiguousarray(_cholesky(0.5 * (cov + cov.T)))
        log_det = float(np.sum(np.log(np.diag(chol))))
        half_log_2pi = 0.5 * d * math.log(2.0 * math.pi)

        def minus_log_g(z):
            return 0.5 * (z * z).sum(dim=1) + half_log_2pi

        n_like = 0
        z1, lj1 = dev.forward(it, mean, chol)
        if not bool(torch.isfinite(lj1).all()):
            raise ValueError("bridge: a sample of the iteration half is not strictly inside the box (or is NaN)")
        if lp is None:
            lp1 = _objective(log_prob, it, chunk)
            n_like += n1
        else:
            lp1 = lp[half:].reshape(n1).contiguous()
        z2 = dev.draw(bridge_key(seed), 0, n2)
        th2, lj2 = dev.points(z2, mean, chol, 0)
        q2 = _objective(log_prob, th2, chunk) + lj2
        n_like += n2
        q1 = lp1 + lj1
        if method == "warp3":
            th1m, lj1m = dev.points(z1, mean, chol, 1)
            th2m, lj2m = dev.points(z2, mean, chol, 1)
            q1 = torch.logaddexp(q1, _objective(log_prob, th1m, chunk) + lj1m) - math.log(2.0)
            q2 = torch.logaddexp(q2, _objective(log_prob, th2m, chunk) + lj2m) - math.log(2.0)
            n_like += n1 + n2
        l1 = (q1 + log_det + minus_log_g(z1)).contiguous()
        l2 = (q2 + log_det + minus_log_g(z2)).contiguous()
        if not bool(torch.isfinite(l1).all()):
            raise ValueError("bridge: a posterior sample must have a finite log posterior (l1 is not finite: is log_probs the "
                             "chain's own, and log_prob finite inside the box?)")
        tau_reliable = True
        if n_eff_arg is not None:
            n_eff = n_eff_arg
        elif len(lead) == 2:
            tau_theta, tau_reliable = _tau(x[half:].contiguous())
            n_eff = n1 / tau_theta
        else:
            n_eff = float(n1)
        s1, s2 = n_eff / (n_eff + n2), n2 / (n_eff + n2)
        lstar = float(torch.sort(l1).values[(n1 - 1) // 2])
        rec, f2 = dev.solve(l1, l2, lstar, s1, s2, tol, max_iter)
        status = int(rec["status"])
        if len(lead) == 2 and status != NONFINITE:
            tau_f, ok = _tau(f2.reshape(n_lead - half, lead[1], 1).contiguous())
            tau_reliable = tau_reliable and ok
        elif n_eff_arg is not None:
            tau_f = n1 / n_eff
        else:
            tau_f = 1.0
    re2 = rec["var_f1"] / (n2 * rec["mean_f1"] ** 2) + tau_f * rec["var_f2"] / (n1 * rec["mean_f2"] ** 2) \
        if status != NONFINITE else math.nan
    return BridgeResult(log_z=rec["log_r"] + lstar, log_z_err=math.sqrt(re2) if re2 >= 0.0 else math.nan, status=status,
                        n_iter=int(rec["n_iter"]) if math.isfinite(rec["n_iter"]) else 0, method=method, n_fit=n_fit,
                        n_iter_rows=n1, n_draws=n2, n_eff=float(n_eff), tau_f=float(tau_f), tau_reliable=bool(tau_reliable),
                        n_like=n_like, mean=mean, chol=chol, l1=l1, l2=l2, f2=f2)
