"""
How many sigma apart are two data sets?  Tension estimators on chains that live on the device.

Everything else in this package answers questions about one likelihood, or about two models on the same data.  The question
the reference's README turns on is about two data sets (do DESI BAO, the compressed CMB and a supernova sample agree under
LambdaCDM?), and a user of ``ShardedEnsemble`` or ``DeviceNestedSampler`` holds the two chains on the GPU already.

* ``difference_chain``: the chain of differences Delta = theta_A - theta_B in the shared parameters, by a fixed pairing.
* ``kde_density``: ``scipy.stats.gaussian_kde(samples.T, bw_method, weights)(at.T)`` on the device.
* ``kde_shift``: the parameter-shift probability of Raveri & Doux (2021): the posterior mass of Delta whose density exceeds
  the density at Delta = 0, from a Gaussian KDE with exact leave-one-out, and its sigmas.
* ``gaussian_shift``: the Gaussian approximation of the same, mean^T cov^-1 mean against chi^2_d.
* ``goodness_of_fit_loss``: Q_DMAP = chi2_joint - chi2_A - chi2_B against chi^2_dof.
* ``suspiciousness``: log R, log I, log S, the Bayesian model dimensionality and the p-value of Handley & Lemos (2019) from
  three nested-sampling runs.
* ``between``: two samplers (or (samples, weights) pairs) in, one dict out.

The density step is an all-pairs sum, n queries x n samples x one exp, and the estimator is only sharp at large n (the noise of
the single zero-shift density dominates at n = 4096, see profiles/NOTES_tension.md).  That sum is csrc/cosmofit_kde.hip
(``cf_kde_sum_device``); torch forms moments and whitens the points; the d x d algebra (Cholesky factor, its inverse) runs on
the host.  There is no CPU fallback for the sums: ``kde_density`` and ``kde_shift`` raise on CPU tensors, after every argument
check, so a wrong argument reads the same with and without a GPU.  ``difference_chain``, ``gaussian_shift``,
``goodness_of_fit_loss`` and ``suspiciousness`` are plain torch / host arithmetic and work anywhere.

Chains are expected thinned by their autocorrelation time (``ShardedEnsemble.get_autocorr_time`` gives it): every error bar
below counts the rows as independent draws.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._args import on_device, stream_of

MAX_NDIM = _lib.CF_KDE_MAX_NDIM

__all__ = ["difference_chain", "kde_density", "kde_shift", "gaussian_shift", "goodness_of_fit_loss", "suspiciousness", "between",
           "shift_offsets", "sigma_of_p", "ShiftResult"]


# ---- argument checks (no device needed) -------------------------------------------------------------------------------
def _chain(x, what: str, estimator: bool = True) -> torch.Tensor:
    """estimator: the chain feeds a density or covariance estimate (1 <= d <= MAX_NDIM, n > d); otherwise any [n, k]."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what} takes the samples as a tensor [n, d]")
    if x.dtype != torch.float64:
        raise ValueError(f"{what} takes float64")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1 or (estimator and x.shape[1] > MAX_NDIM):
        raise ValueError(f"{what} takes samples [n, d] with n >= 1 and 1 <= d <= {MAX_NDIM}" if estimator else
                         f"{what} takes chains [n, k] with n >= 1 and k >= 1")
    if estimator and not x.shape[0] > x.shape[1]:
        raise ValueError(f"{what} needs more samples than dimensions (n > d): the covariance of fewer is singular")
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{what}: the samples must be finite")
    return x


def _weights(w, n: int, like: torch.Tensor, what: str) -> Optional[torch.Tensor]:
    if w is None:
        return None
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float64:
        raise ValueError(f"{what} takes the weights as a float64 tensor")
    if w.dim() != 1 or w.shape[0] != n:
        raise ValueError("weights must be [n], one per sample")
    if w.device != like.device:
        raise ValueError("weights must be on the device of the samples")
    if not bool(torch.isfinite(w).all()):
        raise ValueError(f"{what}: the weights must be finite")
    if not bool((w >= 0).all()) or not float(w.sum()) > 0.0:
        raise ValueError(f"{what}: the weights must be >= 0 with a positive sum")
    return w.contiguous()


def _bandwidth(bandwidth, d: int):
    """'scott' | 'silverman' | a factor > 0 | a d x d kernel covariance (numpy float64, checked symmetric)."""
    if isinstance(bandwidth, str):
        if bandwidth not in ("scott", "silverman"):
            raise ValueError("bandwidth must be 'scott', 'silverman', a factor > 0 or a d x d covariance matrix")
        return bandwidth
    if isinstance(bandwidth, torch.Tensor):
        bandwidth = bandwidth.detach().cpu().numpy()
    if isinstance(bandwidth, bool):
        raise ValueError("bandwidth must be 'scott', 'silverman', a factor > 0 or a d x d covariance matrix")
    if np.ndim(bandwidth) == 0:
        f = float(bandwidth)
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError("a bandwidth factor must be finite and > 0")
        return f
    m = np.asarray(bandwidth, dtype=np.float64)
    if m.shape != (d, d) or not np.isfinite(m).all() or not np.allclose(m, m.T, rtol=1e-12, atol=0.0):
        raise ValueError(f"a bandwidth matrix must be a finite symmetric [{d}, {d}] covariance")
    try:
        np.linalg.cholesky(m)
    except np.linalg.LinAlgError:
        raise ValueError("a bandwidth matrix must be positive definite") from None
    return m


def _columns(cols, k: int, what: str):
    if cols is None:
        return list(range(k))
    cols = [int(c) for c in cols]
    if not cols or any(not -k <= c < k for c in cols):
        raise ValueError(f"{what}: column index out of range (the chain has {k} columns)")
    return cols


def sigma_of_p(p: float) -> float:
    """sqrt(2) erfinv(p): the number of sigmas whose two-sided normal interval holds the probability p."""
    from scipy import special

    return float(math.sqrt(2.0) * special.erfinv(min(max(float(p), 0.0), 1.0)))


# ---- the chain of differences -----------------------------------------------------------------------------------------
def shift_offsets(m: int, n_shifts: int):
    """off_s = ((2 s + 1) m) // (2 n_shifts), s = 0 .. n_shifts - 1: distinct for n_shifts <= m, none of them 0 for m >= 2
    (row i of one chain is never paired with row i of the other, which for two runs of one seed would not be independent)."""
    return [((2 * s + 1) * m) // (2 * n_shifts) for s in range(n_shifts)]


def difference_chain(a, b, columns_a=None, columns_b=None, weights_a=None, weights_b=None, n_shifts: int = 4):
    """(diff [n_shifts * m, d], weights [n_shifts * m]) where ``a`` lives: the chain of differences of two independent chains.

    m = min(n_a, n_b); row s * m + i is a[i, columns_a] - b[(i + off_s) mod n_b, columns_b] with off_s = ``shift_offsets(m,
    n_shifts)[s]``, and its weight is weights_a[i] * weights_b[(i + off_s) mod n_b] (a missing weight vector counts as ones).
    The pairing is deterministic: the same chains give the same rows.  Every row of ``a`` appears n_shifts times, so the rows are
    not independent draws of the difference: n_shifts > 1 smooths the estimate but the n_eff that ``kde_shift`` reports counts
    them as if they were; use n_shifts = 1 for an honest error bar.  Both chains are expected thinned by their autocorrelation
    time (``get_autocorr_time``).  Works on CPU tensors too."""
    a = _chain(a, "difference_chain", False)
    b = _chain(b, "difference_chain", False)
    if b.device != a.device:
        raise ValueError("difference_chain: both chains must be on one device")
    ca, cb = _columns(columns_a, a.shape[1], "columns_a"), _columns(columns_b, b.shape[1], "columns_b")
    if len(ca) != len(cb):
        raise ValueError("difference_chain: columns_a and columns_b must name the same number of shared parameters")
    wa = _weights(weights_a, a.shape[0], a, "difference_chain")
    wb = _weights(weights_b, b.shape[0], a, "difference_chain")
    n_a, n_b = a.shape[0], b.shape[0]
    m = min(n_a, n_b)
    if isinstance(n_shifts, bool) or not isinstance(n_shifts, (int, np.integer)) or not 1 <= n_shifts <= m:
        raise ValueError("n_shifts must be an integer in 1 .. min(n_a, n_b)")
    i = torch.arange(m, device=a.device)
    xa = a[:m][:, ca]
    diffs, ws = [], []
    for off in shift_offsets(m, int(n_shifts)):
        j = (i + off) % n_b
        diffs.append(xa - b[j][:, cb])
        w = torch.ones(m, dtype=torch.float64, device=a.device) if wa is None else wa[:m].clone()
        ws.append(w if wb is None else w * wb[j])
    return torch.cat(diffs).contiguous(), torch.cat(ws).contiguous()


# ---- the kernel density estimate --------------------------------------------------------------------------------------
class _Fit:
    """scipy's gaussian_kde fit of (x, w): total weight, n_eff, mean, kernel covariance, its Cholesky factor on the host."""

    def __init__(self, x: torch.Tensor, w: Optional[torch.Tensor], bandwidth):
        n, d = x.shape
        if w is None:
            W = torch.tensor(float(n), dtype=torch.float64, device=x.device)
            sw2 = W.clone()
            mean = x.sum(dim=0) / W
        else:
            W, sw2 = w.sum(), (w * w).sum()
            mean = (w[:, None] * x).sum(dim=0) / W
        xc = x - mean
        # np.cov(aweights=w, bias=False): sum w (x - mean)(x - mean)^T / (W - sum w^2 / W)
        data_cov = ((xc if w is None else xc * w[:, None]).T @ xc) / (W - sw2 / W)
        host = torch.cat([W.reshape(1), sw2.reshape(1), mean, data_cov.reshape(-1)]).cpu().numpy()
        self.n, self.d = n, d
        self.total, sw2 = float(host[0]), float(host[1])
        self.sum_w2 = sw2
        self.n_eff = self.total * self.total / sw2
        self.mean = host[2:2 + d]
        if isinstance(bandwidth, np.ndarray):
            self.factor, self.cov = None, bandwidth
        else:
            if bandwidth == "scott":
                self.factor = self.n_eff ** (-1.0 / (d + 4))
            elif bandwidth == "silverman":
                self.factor = (self.n_eff * (d + 2) / 4.0) ** (-1.0 / (d + 4))
            else:
                self.factor = bandwidth
            self.cov = host[2 + d:].reshape(d, d) * self.factor**2
        try:
            self.chol = np.linalg.cholesky(self.cov)
        except np.linalg.LinAlgError:
            raise ValueError("the covariance of the samples is singular: no kernel density estimate") from None
        from scipy.linalg import solve_triangular

        self.inv_chol = solve_triangular(self.chol, np.eye(d), lower=True)
        self.norm = (2.0 * math.pi) ** (0.5 * d) * float(np.prod(np.diag(self.chol)))
        self._mean_dev = mean
        self._inv_chol_t = torch.from_numpy(np.ascontiguousarray(self.inv_chol.T)).to(x.device)

    def whiten(self, pts: torch.Tensor) -> torch.Tensor:
        """z = L^-1 (x - mean) per row."""
        return ((pts - self._mean_dev) @ self._inv_chol_t).contiguous()


def _kernel_sums(y: torch.Tensor, w: Optional[torch.Tensor], q: torch.Tensor, self_offset: int = -1, want_sq: bool = False):
    """cf_kde_sum_device on whitened points: (out [m], sq [m] or None)."""
    L, lib = _lib, _lib.lib()
    n, d = y.shape
    m = q.shape[0]
    with torch.cuda.device(y.device):
        out = torch.empty(m, dtype=torch.float64, device=y.device)
        sq = torch.empty(m, dtype=torch.float64, device=y.device) if want_sq else None
        L.check(lib.cf_kde_sum_device(y.data_ptr(), None if w is None else w.data_ptr(), n, d, q.data_ptr(), m, int(self_offset),
                                      out.data_ptr(), None if sq is None else sq.data_ptr(),
                                      stream_of(y.device)))
    return out, sq


def kde_density(samples, at, weights=None, bandwidth="silverman", leave_one_out: bool = False) -> torch.Tensor:
    """``scipy.stats.gaussian_kde(samples.T, bw_method=bandwidth, weights=weights)(at.T)`` on the device: [m] for at [m, d].

    neff = (sum w)^2 / sum w^2; the 'scott' and 'silverman' factors use neff exactly as scipy does; the kernel covariance is
    ``np.cov(samples.T, aweights=w, bias=False) * factor^2``.  A float is a factor; a [d, d] matrix is the kernel covariance
    itself.  Points are centred on the weighted mean and whitened with the inverse Cholesky factor, the all-pairs sum runs in
    csrc/cosmofit_kde.hip, and the result is normalised by (2 pi)^{d/2} sqrt(det) and by the sum of the weights.

    leave_one_out=True: ``at`` must be None or ``samples`` itself; row i is then the density at sample i of the estimate built
    WITHOUT sample i (its term is left out inside the sum, nothing is subtracted) and is normalised by the sum of the weights
    without w_i.  The covariance and the bandwidth stay those of all samples.

    By-product: smooth marginal densities for plots.  Pass one or two columns of a chain as ``samples`` and the points of a 1-D
    or 2-D grid as ``at`` to get the curve or surface a corner plot draws, without binning.

    A point further than ~37 kernel widths from every sample gets exactly 0.0; a NaN or infinite coordinate in ``at`` gives NaN
    in that row only."""
    x = _chain(samples, "kde_density")
    n, d = x.shape
    w = _weights(weights, n, x, "kde_density")
    bw = _bandwidth(bandwidth, d)
    if leave_one_out:
        if at is not None and at is not samples:
            raise ValueError("kde_density: leave_one_out evaluates at the samples themselves (pass at=None or at=samples)")
    else:
        if not isinstance(at, torch.Tensor) or at.dtype != torch.float64 or at.dim() != 2 or at.shape[1] != d or at.shape[0] < 1:
            raise ValueError(f"kde_density takes the evaluation points as a float64 tensor [m, {d}]")
        if at.device != x.device:
            raise ValueError("kde_density: the evaluation points must be on the device of the samples")
    x = on_device(x, "kde_density").contiguous()
    fit = _Fit(x, w, bw)
    y = fit.whiten(x)
    if leave_one_out:
        out, _ = _kernel_sums(y, w, y, 0)
        rest = (fit.total - 1.0) if w is None else (fit.total - w)
        return out / (fit.norm * rest)
    out, _ = _kernel_sums(y, w, fit.whiten(at))
    return out / (fit.norm * fit.total)


@dataclass
class ShiftResult:
    """What ``kde_shift`` returns.  p_exceed: the posterior mass of the difference whose density exceeds the density at the
    tested point; n_sigma = sqrt(2) erfinv(p_exceed), or the bound from 1 - 1 / n_eff when no sample lies below
    (saturated=True); p_zero +- p_zero_se: the density at the tested point and its standard error; p_interval /
    sigma_interval: p_exceed recomputed at p_zero -+ 2 se, widened by the binomial error sqrt(P (1 - P) / n_eff) in quadrature;
    n_eff = (sum w)^2 / sum w^2; count: the rows above, an exact integer (None for weighted chains); densities: the
    leave-one-out density at every sample, a device tensor; factor: the bandwidth factor (None for a matrix)."""
    p_exceed: float
    n_sigma: float
    saturated: bool
    p_zero: float
    p_zero_se: float
    p_interval: Tuple[float, float]
    sigma_interval: Tuple[float, float]
    n_eff: float
    count: Optional[int]
    densities: torch.Tensor
    factor: Optional[float]


def kde_shift(diff, weights=None, bandwidth="silverman", at=None) -> ShiftResult:
    """The parameter-shift probability of a chain of differences [n, d] (``difference_chain``) at the point ``at`` (default:
    zero shift): p_exceed = sum_i w_i [p_{-i}(Delta_i) > p(at)] / sum_i w_i, where p is the Gaussian KDE of the chain
    (``kde_density``'s definitions) and p_{-i} the same estimate without sample i.  Leave-one-out is part of the estimator:
    with the self term a sample's own kernel lifts its density above the threshold and p_exceed is biased high, badly so at
    d >= 4.

    The standard error of p(at) is that of a weighted mean of n iid kernel values K_j:
    se^2 = [sum (w_j K_j)^2 - (sum w_j K_j)^2 sum w_j^2 / (sum w_j)^2] / (sum w_j)^2, with both sums from the device kernel.
    The unweighted count is an integer reduction and therefore exact."""
    x = _chain(diff, "kde_shift")
    n, d = x.shape
    w = _weights(weights, n, x, "kde_shift")
    bw = _bandwidth(bandwidth, d)
    if at is None:
        at_host = np.zeros(d)
    else:
        at_host = np.asarray(at.detach().cpu().numpy() if isinstance(at, torch.Tensor) else at, dtype=np.float64).reshape(-1)
        if at_host.shape != (d,) or not np.isfinite(at_host).all():
            raise ValueError(f"kde_shift: `at` must be a finite point of {d} coordinates")
    x = on_device(x, "kde_shift").contiguous()
    fit = _Fit(x, w, bw)
    y = fit.whiten(x)
    q0 = torch.from_numpy(((at_host - fit.mean) @ fit.inv_chol.T).reshape(1, d)).to(x.device)
    k0, k0sq = _kernel_sums(y, w, q0, -1, want_sq=True)
    out, _ = _kernel_sums(y, w, y, 0)
    rest = (fit.total - 1.0) if w is None else (fit.total - w)
    dens = out / (fit.norm * rest)
    k0, k0sq = float(k0[0]), float(k0sq[0])
    W = fit.total
    p_zero = k0 / (fit.norm * W)
    var = (k0sq - k0 * k0 * fit.sum_w2 / (W * W)) / (W * W)
    se = math.sqrt(max(var, 0.0)) / fit.norm
    thresholds = torch.tensor([p_zero, p_zero + 2.0 * se, p_zero - 2.0 * se], dtype=torch.float64, device=x.device)
    above = dens[None, :] > thresholds[:, None]  # [3, n]
    counts = above.sum(dim=1)
    if w is None:
        c = counts.cpu().tolist()
        count, (p, p_lo, p_hi) = int(c[0]), (c[0] / n, c[1] / n, c[2] / n)
        all_above = c[0] == n
    else:
        mass = ((above.to(torch.float64) * w[None, :]).sum(dim=1) / W).cpu().tolist()
        count, (p, p_lo, p_hi) = None, mass
        all_above = int(counts[0]) == n
    n_eff = fit.n_eff
    cap = 1.0 - 1.0 / n_eff
    binom = math.sqrt(max(p * (1.0 - p), 0.0) / n_eff)
    lo = max(p - math.hypot(p - p_lo, binom), 0.0)
    hi = min(p + math.hypot(p_hi - p, binom), 1.0)
    saturated = bool(all_above)
    return ShiftResult(p_exceed=p, n_sigma=sigma_of_p(cap if saturated else p), saturated=saturated, p_zero=p_zero, p_zero_se=se,
                       p_interval=(lo, hi), sigma_interval=(sigma_of_p(min(lo, cap)), sigma_of_p(min(hi, cap))), n_eff=n_eff, count=count,
                       densities=dens, factor=fit.factor)


# ---- closed forms -----------------------------------------------------------------------------------------------------
def _two_sided_sigma(p_tail: float) -> float:
    from scipy import stats

    if not p_tail < 1.0:
        return 0.0
    return float(stats.norm.isf(0.5 * p_tail))


def gaussian_shift(diff, weights=None) -> dict:
    """The Gaussian approximation of the shift: chi2 = mean^T cov^-1 mean of the difference chain [n, d] (weighted mean;
    ``np.cov(aweights=w, bias=False)``), its chi^2_d tail probability ``p_value`` and ``n_sigma``, the two-sided normal
    quantile of that tail.  The moments are formed in torch where the chain lives (CPU tensors work); the rest on the host.
    Also returns dof, mean [d] and cov [d, d] as numpy."""
    from scipy import stats

    x = _chain(diff, "gaussian_shift")
    n, d = x.shape
    w = _weights(weights, n, x, "gaussian_shift")
    if w is None:
        W = float(n)
        mean = x.sum(dim=0) / W
        xc = x - mean
        cov = xc.T @ xc / (W - 1.0)
    else:
        W, sw2 = w.sum(), (w * w).sum()
        mean = (w[:, None] * x).sum(dim=0) / W
        xc = x - mean
        cov = (xc * w[:, None]).T @ xc / (W - sw2 / W)
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    try:
        chol = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError("gaussian_shift: the covariance of the differences is singular") from None
    from scipy.linalg import solve_triangular

    z = solve_triangular(chol, mean, lower=True)
    chi2 = float(z @ z)
    p_tail = float(stats.chi2.sf(chi2, d))
    return dict(chi2=chi2, dof=d, p_value=p_tail, n_sigma=_two_sided_sigma(p_tail), mean=mean, cov=cov)


def _chi2_of(fit) -> float:
    v = float(getattr(fit, "chi2", fit))
    if not math.isfinite(v):
        raise ValueError("goodness_of_fit_loss takes finite chi^2 values")
    return v


def goodness_of_fit_loss(chi2_a, chi2_b, chi2_joint, dof: int) -> dict:
    """Q_DMAP = chi2_joint - chi2_a - chi2_b: what the best fit loses when the two data sets must share parameters, against
    chi^2 with ``dof`` degrees of freedom (the number of shared parameters both sets constrain).  Each input is a chi^2_min or an
    ``optimize.FitResult`` (its ``chi2``).  Returns dict(q_dmap, dof, p_value, n_sigma); n_sigma is
    ``optimize.sigma_from_delta_chi2(q_dmap, dof)``, sqrt(Q) for one degree of freedom, and 0 for Q <= 0."""
    from scipy import stats

    from .optimize import sigma_from_delta_chi2

    if isinstance(dof, bool) or not isinstance(dof, (int, np.integer)) or dof < 1:
        raise ValueError("dof must be an integer >= 1")
    q = _chi2_of(chi2_joint) - _chi2_of(chi2_a) - _chi2_of(chi2_b)
    p = float(stats.chi2.sf(q, dof)) if q > 0.0 else 1.0
    return dict(q_dmap=q, dof=int(dof), p_value=p, n_sigma=sigma_from_delta_chi2(q, int(dof)))


def _run_summary(run, what: str):
    """(log_z, information D, d = 2 Var_post(log L)) of a nested run or a (log_z, information, log_l, weights) tuple."""
    if isinstance(run, (tuple, list)):
        if len(run) != 4:
            raise ValueError(f"{what}: a run is a DeviceNestedSampler or (log_z, information, log_l, weights)")
        log_z, info, log_l, w = run
    else:
        try:
            _, log_w, log_l = run.posterior()
            log_z, info = run.log_z, run.information
        except AttributeError:
            raise ValueError(f"{what}: a run is a DeviceNestedSampler or (log_z, information, log_l, weights)") from None
        w = np.exp(log_w)
    log_l, w = np.asarray(log_l, dtype=np.float64).reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1)
    if log_l.shape != w.shape or log_l.size < 2:
        raise ValueError(f"{what}: log_l and weights must be two vectors of one length >= 2")
    if not (np.isfinite(log_l).all() and np.isfinite(w).all() and (w >= 0).all() and w.sum() > 0):
        raise ValueError(f"{what}: log_l must be finite and the weights finite, >= 0, with a positive sum")
    log_z, info = float(log_z), float(info)
    if not (math.isfinite(log_z) and math.isfinite(info)):
        raise ValueError(f"{what}: log_z and the information must be finite")
    p = w / w.sum()
    mean = float((p * log_l).sum())
    return log_z, info, 2.0 * float((p * (log_l - mean) ** 2).sum())


def suspiciousness(run_a, run_b, run_joint) -> dict:
    """Handley & Lemos (2019) from three nested-sampling runs (A alone, B alone, both): log R = log Z_AB - log Z_A - log Z_B;
    log I = D_A + D_B - D_AB (Kullback-Leibler divergences, ``DeviceNestedSampler.information``); log S = log R - log I;
    the Bayesian model dimensionality of a run is 2 Var_posterior(log L) and d = d_A + d_B - d_AB; d - 2 log S is chi^2_d
    distributed if the sets agree, which gives ``p_value`` and ``n_sigma``.  A run is a ``DeviceNestedSampler`` or a tuple
    (log_z, information, log_l, weights).  Host arithmetic only.  p_value and n_sigma are NaN when d <= 0."""
    from scipy import stats

    (za, da, ka), (zb, db, kb), (zj, dj, kj) = (_run_summary(r, "suspiciousness") for r in (run_a, run_b, run_joint))
    log_r = zj - za - zb
    log_i = da + db - dj
    log_s = log_r - log_i
    d = ka + kb - kj
    if d > 0.0:
        p = float(stats.chi2.sf(d - 2.0 * log_s, d))
        sigma = _two_sided_sigma(p)
    else:
        p = sigma = float("nan")
    return dict(log_r=log_r, log_i=log_i, log_s=log_s, d=d, d_a=ka, d_b=kb, d_joint=kj, p_value=p, n_sigma=sigma)


# ---- two samplers in, one answer out ----------------------------------------------------------------------------------
def _samples_of(run, discard: int, thin: int, what: str):
    if isinstance(run, (tuple, list)):
        if len(run) != 2:
            raise ValueError(f"{what}: pass a sampler or a (samples, weights) pair")
        return run[0], run[1]
    if hasattr(run, "get_chain"):
        return run.get_chain(discard=discard, thin=thin, flat=True), None
    if hasattr(run, "posterior"):
        pts, log_w, _ = run.posterior()
        dev = getattr(run, "device", "cpu")
        return (torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev),
                torch.from_numpy(np.exp(np.asarray(log_w, dtype=np.float64))).to(dev))
    raise ValueError(f"{what}: pass a ShardedEnsemble, a DeviceNestedSampler or a (samples, weights) pair")


def between(a, b, columns_a, columns_b, discard: int = 0, thin: int = 1, **kw) -> dict:
    """The tension between two posteriors in the parameters they share.  ``a`` and ``b`` are ``ShardedEnsemble`` objects (their
    ``get_chain(discard, thin, flat=True)``), ``DeviceNestedSampler`` objects (their ``posterior()`` with weights exp(log_w))
    or (samples, weights) pairs; columns_a / columns_b name the shared parameters in each.  Keywords: n_shifts
    (``difference_chain``), bandwidth and at (``kde_shift``).

    Returns dict(diff, weights (None when neither side is weighted), kde (a ``ShiftResult``), gaussian (``gaussian_shift``'s
    dict), p_exceed, n_sigma, sigma_interval, gaussian_n_sigma, n, d)."""
    extra = set(kw) - {"n_shifts", "bandwidth", "at"}
    if extra:
        raise TypeError(f"between: unexpected keyword {sorted(extra)[0]!r}")
    xa, wa = _samples_of(a, discard, thin, "between")
    xb, wb = _samples_of(b, discard, thin, "between")
    diff, w = difference_chain(xa, xb, columns_a, columns_b, wa, wb, n_shifts=kw.get("n_shifts", 4))
    if wa is None and wb is None:
        w = None
    kde = kde_shift(diff, w, bandwidth=kw.get("bandwidth", "silverman"), at=kw.get("at"))
    gauss = gaussian_shift(diff, w)
    return dict(diff=diff, weights=w, kde=kde, gaussian=gauss, p_exceed=kde.p_exceed, n_sigma=kde.n_sigma,
                sigma_interval=kde.sigma_interval, gaussian_n_sigma=gauss["n_sigma"], n=diff.shape[0], d=diff.shape[1])
