"""
Linear SN nuisance parameters in closed form: marginalise (or profile) them on the device instead of sampling them.

Every supernova likelihood carries parameters that enter the residual linearly: the absolute magnitude ``M`` (the ``offset``
slot, exactly degenerate with ``H0`` up to the H0 prior), the bulk-flow amplitude (the ``lin`` slot times ``sn_lin_coef``), a
per-survey calibration offset, a host-mass step.  With the SN residual written as

    r(theta, alpha) = r0(theta) - A alpha

where ``r0`` is the engine's own residual row with those slots FIXED in its descriptor (for M: ``Param(fixed=M_ref)`` for
``offset`` and ``alpha = M - M_ref``) and ``A [n_sn, m]`` holds constant templates (``Templates``), a prior ``N(mu_j, sigma_j)``
or a flat one on each ``alpha_j`` gives, with ``P = diag(1 / sigma_j^2)``, ``K = C^-1 A``, ``F = A^T K + P = L_F L_F^T``,

    Wt = K L_F^-T,  ct = L_F^-1 P mu,  U = L_F^T,  pmu = mu^T P mu            (once, on the host: ``project``)
    t = Wt^T r0 + ct,   q = sum_j t_j^2
    chi2_prof  = chi2_engine + pmu - q                 the minimum over alpha, prior penalty included
    alpha_hat  = U^-1 t                                the conditional mean; the conditional covariance is F^-1
    alpha_draw = U^-1 (t + xi),  xi ~ N(0, I)          a draw from p(alpha | theta, data)
    ln L_marg  = ln L_engine + 0.5 q - 0.5 pmu + log_norm

(csrc/cosmofit_marg.hip: the product on FP64 matrix cores, then sixteen lanes per row; ``cf_marg_eval_device``).  A flat prior
has density 1 per unit of alpha_j, or ``1 / (hi_j - lo_j)`` when a box is given; the box only normalises, it does not truncate
(``box_mass`` says when that matters).  Nothing depends on ``M_ref`` except rounding -- ``chi2_engine - q`` cancels when it is far
off, so fix it near the expected value.

``LinearNuisance`` cannot know what the columns of ``A`` mean: it is the caller who fixes the matching slots in the engine.  Name
them in ``slots=`` and a slot that the engine still reads from theta is reported by a warning.

Out of scope: truncating the marginal at the box; nuisances of the BAO / CMB blocks (``r_d`` is not linear); combining with
``covscale``'s amplitude; quasar engines and engines over several devices.  There is no CPU fallback: the evaluation needs the
engine's MI355X.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from ._args import ptr, stream_of

PROBE_LIMIT = 1e-11  # the limit cf_create's pack probe uses
MAX_M = L.CF_MARG_MAX_M
MODES = {"profile": L.CF_MARG_PROFILE, "marginal": L.CF_MARG_MARGINAL}
LD = np.longdouble
_EPS = float(np.finfo(np.float64).eps)
_MARG_TAG = 0x4D4152474E414C31  # "MARGNAL1": the domain tag of the conditional draws (the mock sets' is "MOCKSET1")
_GOLDEN = 0x9E3779B97F4A7C15
_U64 = (1 << 64) - 1

__all__ = ["project", "Templates", "LinearNuisance", "Projection", "recover_key", "set_library_chunk", "MAX_M", "MODES"]


class Templates:
    """Columns of ``A``; ``stack`` puts them side by side."""

    @staticmethod
    def offset(n: int) -> np.ndarray:
        """A column of ones: the absolute magnitude, or any offset common to all SNe."""
        return np.ones(int(n))

    @staticmethod
    def mask(flags) -> np.ndarray:
        """A 0/1 column from booleans [n]: the offset of one survey, a host-mass step, a low-z sample."""
        f = np.asarray(flags)
        if f.ndim != 1 or f.dtype != np.bool_:
            raise ValueError("mask takes booleans [n]")
        return f.astype(np.float64)

    @staticmethod
    def column(v) -> np.ndarray:
        """Any column [n], e.g. the engine's ``lin_coef`` (the bulk-flow amplitude)."""
        c = np.asarray(v, dtype=np.float64)
        if c.ndim != 1:
            raise ValueError("column takes a vector [n]")
        return c.copy()

    @staticmethod
    def stack(*cols) -> np.ndarray:
        return np.ascontiguousarray(np.column_stack([np.asarray(c, dtype=np.float64) for c in cols]))


def _solve_lower(Lo, B):
    """X with L X = B, row by row in long double."""
    X = np.array(B, dtype=LD, ndmin=2)
    for i in range(Lo.shape[0]):
        X[i] = (X[i] - Lo[i, :i] @ X[:i]) / Lo[i, i]
    return X


def _solve_upper_t(Lo, B):
    """X with L^T X = B, from the last row up."""
    X = np.array(B, dtype=LD, ndmin=2)
    for i in range(Lo.shape[0] - 1, -1, -1):
        X[i] = (X[i] - Lo[i + 1:, i] @ X[i + 1:]) / Lo[i, i]
    return X


def _prior(m, mu, sigma, box):
    mu = np.zeros(m) if mu is None else np.asarray(mu, dtype=np.float64).reshape(-1)
    sigma = np.full(m, np.inf) if sigma is None else np.asarray(sigma, dtype=np.float64).reshape(-1)
    if mu.shape != (m,) or sigma.shape != (m,):
        raise ValueError(f"mu and sigma must have one entry per column of A ({m})")
    if not np.isfinite(mu).all():
        raise ValueError("mu must be finite (it is not read where sigma is inf)")
    if not ((sigma > 0) & ~np.isnan(sigma)).all():
        raise ValueError("sigma must be > 0; inf marks a flat prior")
    lo, hi = np.full(m, np.nan), np.full(m, np.nan)
    if box is not None:
        if len(box) != m:
            raise ValueError(f"box must have one entry per column of A ({m}): (lo, hi) or None")
        for j, b in enumerate(box):
            if b is None:
                continue
            lo[j], hi[j] = (float(v) for v in b)
            if not (np.isfinite(lo[j]) and np.isfinite(hi[j]) and lo[j] < hi[j]):
                raise ValueError(f"box[{j}] must be a finite interval (lo, hi)")
    return mu, sigma, lo, hi


def project(chol, A, mu=None, sigma=None, box=None) -> dict:
    """The host algebra: ``dict(Wt, ct, U, pmu, log_norm, F, m_flat, probe_rel)`` for the Cholesky factor ``chol`` of the SN
    covariance (only its lower triangle is read), templates ``A [n, m]`` (a vector is one column) and the prior: ``mu [m]``
    (default 0), ``sigma [m]`` (default and inf: flat), ``box``: per component ``(lo, hi)`` or None, the normalisation of a flat
    prior (for a Gaussian one it is only what ``box_mass`` reports on).

    K comes from two triangular substitutions with the factor in long double; F is symmetrised once and factored in long double.
    A rank-deficient F -- A without full column rank on the flat components -- is refused with the offending column named.
    probe_rel: on three probe vectors r the largest ``|Wt^T r - L_F^-1 A^T C^-1 r|`` (the right side in long double from the
    definitions), divided by the terms summed, ``max_j sum_i |r_i| |Wt_ij|``.  Raises above 1e-11."""
    Lo = np.tril(np.asarray(chol, dtype=np.float64))
    if Lo.ndim != 2 or Lo.shape[0] != Lo.shape[1] or Lo.shape[0] < 1:
        raise ValueError("project takes a square Cholesky factor")
    n = Lo.shape[0]
    if not (np.isfinite(Lo).all() and (np.diag(Lo) > 0).all()):
        raise ValueError("the factor must be finite with a positive diagonal")
    A = np.asarray(A, dtype=np.float64)
    if A.ndim == 1:
        A = A[:, None]
    if A.ndim != 2 or A.shape[0] != n or not 1 <= A.shape[1] <= MAX_M:
        raise ValueError(f"A must be [{n}, m] with 1 <= m <= {MAX_M}, got shape {A.shape}")
    if not np.isfinite(A).all():
        raise ValueError("A must be finite")
    m = A.shape[1]
    mu, sigma, lo, hi = _prior(m, mu, sigma, box)
    proper = np.isfinite(sigma)
    Ll, Al = np.asarray(Lo, dtype=LD), np.asarray(A, dtype=LD)
    P = np.where(proper, LD(1) / np.asarray(np.where(proper, sigma, 1.0), dtype=LD) ** 2, LD(0))
    K = _solve_upper_t(Ll, _solve_lower(Ll, Al))  # [n, m]
    F = Al.T @ K + np.diag(P)
    F = LD(0.5) * (F + F.T)
    LF = np.zeros((m, m), dtype=LD)
    floor = max(n, 16) * _EPS
    for j in range(m):
        d = F[j, j] - LF[j, :j] @ LF[j, :j]
        if not d > floor * F[j, j]:
            raise ValueError(f"project: F = A^T C^-1 A + P is not positive definite at column {j} of A: it is zero or a "
                             f"combination of the columns before it, and its prior is flat (or too wide to tell them apart)")
        LF[j, j] = np.sqrt(d)
        LF[j + 1:, j] = (F[j + 1:, j] - LF[j + 1:, :j] @ LF[j, :j]) / LF[j, j]
    Wt = _solve_lower(LF, K.T).T           # K L_F^-T
    Pmu = P * np.asarray(np.where(proper, mu, 0.0), dtype=LD)
    ct = _solve_lower(LF, Pmu[:, None])[:, 0]
    pmu = float(Pmu @ np.asarray(np.where(proper, mu, 0.0), dtype=LD))
    boxed = ~proper & np.isfinite(lo)
    m_flat = int((~proper).sum())
    log_norm = (-np.log(np.diag(LF)).sum() + LD(0.5) * m_flat * np.log(LD(2) * LD(np.pi))
                - np.log(np.asarray(sigma[proper], dtype=LD)).sum() - np.log(np.asarray(hi[boxed] - lo[boxed], dtype=LD)).sum())
    res = dict(Wt=np.ascontiguousarray(Wt, dtype=np.float64), ct=np.ascontiguousarray(ct, dtype=np.float64),
               U=np.ascontiguousarray(LF.T, dtype=np.float64), pmu=pmu, log_norm=float(log_norm),
               F=np.ascontiguousarray(F, dtype=np.float64), m_flat=m_flat)
    rng = np.random.default_rng(n + 1000 * m)
    probe_rel = 0.0
    for _ in range(3):
        r = Lo @ rng.standard_normal(n)
        g = _solve_upper_t(Ll, _solve_lower(Ll, np.asarray(r, dtype=LD)[:, None]))[:, 0]
        ref = _solve_lower(LF, (Al.T @ g)[:, None])[:, 0]
        got = res["Wt"].T @ r
        scale = float(np.max(np.abs(res["Wt"]).T @ np.abs(r)))  # of the largest component: a column of Wt may vanish
        probe_rel = max(probe_rel, float(np.max(np.abs(np.asarray(got - ref, dtype=np.float64)))) / scale)
    res["probe_rel"] = probe_rel
    if not probe_rel <= PROBE_LIMIT:
        raise ValueError(f"project: the probe of Wt^T r against L_F^-1 A^T C^-1 r differs by {probe_rel:.2e} of the terms summed "
                         f"(limit {PROBE_LIMIT:.0e}): the covariance is too ill-conditioned for this identity")
    return res


def _mix(x: int) -> int:
    """The hash round of ``ensemble._mix_int`` (splitmix64's finaliser), restated so that this module imports without torch."""
    x = (x + _GOLDEN) & _U64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _U64
    return x ^ (x >> 31)


def recover_key(seed: int) -> int:
    """Unsigned 64-bit key of the conditional draws of ``recover(seed=)``: ``mocks.normals(key, S, m, k0=row0)``."""
    return _mix(_mix((int(seed) * _GOLDEN + _MARG_TAG) & _U64))


class Projection:
    """``Wt``, ``ct`` and ``U`` on one device (``cf_marg``): the handle-free half, ``apply`` on caller-supplied residual rows."""

    def __init__(self, proj: dict, device: int = 0):
        Wt = np.ascontiguousarray(proj["Wt"], dtype=np.float64)
        ct = np.ascontiguousarray(proj["ct"], dtype=np.float64)
        U = np.ascontiguousarray(proj["U"], dtype=np.float64)
        if Wt.ndim != 2 or ct.shape != (Wt.shape[1],) or U.shape != (Wt.shape[1], Wt.shape[1]):
            raise ValueError("Projection takes Wt [n, m], ct [m] and U [m, m]")
        self.n, self.m, self.device = int(Wt.shape[0]), int(Wt.shape[1]), int(device)
        self._p = C.c_void_p()
        L.check(L.lib().cf_marg_create(ptr(Wt), ptr(ct), ptr(U), self.n, self.m, float(proj["pmu"]), float(proj["log_norm"]),
                                       self.device, C.byref(self._p)))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            L.lib().cf_marg_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, rows, S: Optional[int] = None, xi=None, want=("t", "q", "alpha")):
        """(t [S, m], q [S], alpha [S, m]; None where not in `want`) for rows[:S, :n], asynchronous on torch's current stream
        (``cf_marg_apply_device``).  rows: float64 [>= S, pitch >= n] on the device with contiguous columns; columns >= n and
        rows >= S are never read.  xi [S, m] or None: alpha = U^-1 (t + xi)."""
        import torch

        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or rows.dim() != 2 or rows.stride(1) != 1:
            raise ValueError("apply takes a float64 tensor [S, >= n] with contiguous columns")
        if not rows.is_cuda or rows.device.index != self.device:
            raise ValueError("apply takes rows on the device of the projection")
        S = rows.shape[0] if S is None else int(S)
        if not 0 <= S <= rows.shape[0] or rows.shape[1] < self.n:
            raise ValueError("apply: S rows of at least n columns")
        if xi is not None and (xi.dtype != torch.float64 or xi.shape != (S, self.m) or not xi.is_contiguous() or xi.device != rows.device):
            raise ValueError("apply takes xi as a contiguous float64 tensor [S, m] on the rows' device")
        f64 = dict(dtype=torch.float64, device=rows.device)
        t = torch.empty((S, self.m), **f64) if "t" in want else None
        q = torch.empty((S,), **f64) if "q" in want else None
        alpha = torch.empty((S, self.m), **f64) if "alpha" in want else None
        dptr = lambda x: None if x is None else x.data_ptr()
        with torch.cuda.device(rows.device):
            L.check(L.lib().cf_marg_apply_device(self._p, rows.data_ptr(), rows.stride(0), S, dptr(xi), dptr(t), dptr(q),
                                                 dptr(alpha), stream_of(rows.device)))
        return t, q, alpha


def set_library_chunk(engine, rows: int = 0):
    """Rows per chunk of the library's own loop over the workspace (0: the default, ``_lib.CF_MARG_CHUNK``).  No result depends
    on it; tests lower it to cross chunk boundaries with few rows."""
    L.check(L.lib().cf_marg_set_chunk(engine._h, int(rows)))


class LinearNuisance:
    """The engine's likelihood with ``alpha`` (the amplitudes of the templates ``A``) integrated out (mode "marginal") or
    minimised out (mode "profile").  The sampled vector is the engine's own theta: one dimension fewer per template than the
    engine that samples them.  ``chi_squared`` is ``chi2_prof`` in both modes.

    The factor is the one the engine was built with (``engine.mock_data["sn_chol"]``).  Every other block, constant and prior
    term is the engine's own.  slots: the engine slots the templates stand for (``("offset",)`` for a column of ones); one that
    the engine reads from theta instead of holding fixed is reported by a warning -- otherwise this class cannot know what A
    means."""

    def __init__(self, engine, A, mu=None, sigma=None, box=None, mode: str = "marginal", slots: Sequence[str] = ()):
        info = getattr(engine, "model_info", {})
        if info.get("quasar"):
            raise ValueError("LinearNuisance: a quasar engine has no dense SN block to project")
        if info.get("multi_device"):
            raise ValueError("LinearNuisance: this engine spans several devices; use one engine per device")
        chol = getattr(engine, "mock_data", {}).get("sn_chol")
        if chol is None or not getattr(engine, "n_sn", 0):
            raise ValueError("LinearNuisance: this engine has no SN block")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        for name in slots:
            if name not in L.SLOTS:
                raise ValueError(f"unknown parameter slot {name!r}; valid: {L.SLOTS}")
            if name in getattr(engine, "sampled_slots", ()):
                warnings.warn(f"LinearNuisance: the engine reads the slot {name!r} from theta; fix it in the engine "
                              f"(Param(fixed=...)) when a template stands for it, or it is counted twice")
        self.engine, self.mode, self.ndim = engine, MODES[mode], int(engine.ndim)
        self.info = project(chol, A, mu=mu, sigma=sigma, box=box)
        self.m = int(self.info["U"].shape[0])
        _, _, self._lo, self._hi = _prior(self.m, mu, sigma, box)
        Ui = np.linalg.inv(np.triu(self.info["U"]))
        self.cov = Ui @ Ui.T  # F^-1: the conditional covariance of alpha, the same for every theta
        self._proj = Projection(self.info, device=int(engine.info()["device"]))

    # ---- lifetime --------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_proj", None) is not None:
            self._proj.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- host numbers ----------------------------------------------------------------------------------------------------------
    def _rows(self, theta):
        x = np.asarray(theta, dtype=np.float64)
        single = x.ndim == 1
        x = np.atleast_2d(x)
        if x.ndim != 2 or x.shape[1] != self.ndim:
            raise ValueError(f"theta must have {self.ndim} columns, got {x.shape}")
        return single, np.ascontiguousarray(x)

    def _host(self, theta, kind, xi=None, want_out=True, want_alpha=False):
        """cf_marg_eval on host rows theta [W, ndim]: (out [W] or None, alpha [W, m] or None)."""
        W = theta.shape[0]
        out = np.empty(W) if want_out else None
        alpha = np.empty((W, self.m)) if want_alpha else None
        L.check(L.lib().cf_marg_eval(self.engine._h, self._proj._p, ptr(theta), W, kind, self.mode, ptr(xi), ptr(out), ptr(alpha)))
        return out, alpha

    def _eval(self, theta, kind):
        single, th = self._rows(theta)
        out = self._host(th, kind)[0]
        return float(out[0]) if single else out

    def chi_squared(self, theta):
        """chi2_prof: the engine's chi^2 minimised over alpha, prior penalty included; one row [ndim] -> float, [W, ndim] -> [W]."""
        return self._eval(theta, L.CF_OUT_CHI2)

    def log_likelihood(self, theta):
        """The engine's log L with alpha integrated out (mode "marginal") or at alpha_hat (mode "profile")."""
        return self._eval(theta, L.CF_OUT_LOGL)

    def log_probability(self, theta):
        """The engine's log P with the same replacement; -inf where the engine says so."""
        return self._eval(theta, L.CF_OUT_LOGP)

    def log_probs_vectorized(self, theta):
        return self.log_probability(np.atleast_2d(theta))

    # ---- device ----------------------------------------------------------------------------------------------------------------
    def _check_tensor(self, x):
        import torch

        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != self.ndim:
            raise ValueError(f"theta must be a float64 tensor [W, {self.ndim}] on the engine's GPU")
        return x.contiguous()

    def _device(self, theta, kind, xi=None, want_out=True, want_alpha=False):
        import torch

        W = theta.shape[0]
        out = torch.empty(W, dtype=torch.float64, device=theta.device) if want_out else None
        alpha = torch.empty((W, self.m), dtype=torch.float64, device=theta.device) if want_alpha else None
        dptr = lambda x: None if x is None else x.data_ptr()
        if W:
            with torch.cuda.device(theta.device):
                L.check(L.lib().cf_marg_eval_device(self.engine._h, self._proj._p, theta.data_ptr(), W, kind, self.mode, dptr(xi),
                                                    dptr(out), dptr(alpha), stream_of(theta.device)))
        return out, alpha

    def torch_log_prob(self, kind: int = L.CF_OUT_LOGP):
        """Callable ``f(x: cuda float64 tensor [W, ndim]) -> tensor [W]``, asynchronous on torch's current stream: what
        ``ShardedEnsemble``, ``replicas``, ``optimize.best_fit`` / ``profile`` and ``nested.DeviceNestedSampler`` take.  It
        carries no ``.engine`` attribute: the engine's residual reports would describe alpha = 0 (M = M_ref)."""

        def f(x):
            return self._device(self._check_tensor(x), kind)[0]

        return f

    def _alpha(self, theta, xi_of):
        """alpha rows for host numbers (numpy out) or a device tensor (tensor out); xi_of(S, device) -> tensor or None."""
        import torch

        if isinstance(theta, torch.Tensor):
            th = self._check_tensor(theta)
            return self._device(th, L.CF_OUT_LOGL, xi=xi_of(th.shape[0], th.device), want_out=False, want_alpha=True)[1]
        _, th = self._rows(theta)
        xi = xi_of(th.shape[0], torch.device("cuda", self._proj.device))
        xi = None if xi is None else np.ascontiguousarray(xi.cpu().numpy())
        return self._host(th, L.CF_OUT_LOGL, xi=xi, want_out=False, want_alpha=True)[1]

    def conditional(self, theta):
        """``(alpha_hat [S, m], cov [m, m])`` of p(alpha | theta, data) = N(alpha_hat(theta), F^-1).  A row the engine's
        likelihood rejects (a non-finite chi^2) has NaN.  theta: host numbers (numpy out) or a device tensor (tensors out)."""
        import torch

        a = self._alpha(theta, lambda S, dev: None)
        cov = torch.from_numpy(self.cov).to(a.device) if isinstance(a, torch.Tensor) else self.cov.copy()
        return a, cov

    def recover(self, theta, seed: int = 0, row0: int = 0):
        """One draw of alpha [S, m] from p(alpha | theta, data) per row: restores the marginalised columns of a chain
        (M = M_ref + alpha).  The normals are ``mocks.normals(recover_key(seed), S, m, k0=row0)``: the draw of row i depends on
        (seed, row0 + i) only, so a chain can be recovered piece by piece with the same numbers."""
        from . import mocks

        key = recover_key(seed)
        return self._alpha(theta, lambda S, dev: mocks.normals(key, S, self.m, k0=int(row0), device=dev))

    def box_mass(self, theta):
        """[S, m]: per component the Gaussian mass of its box interval under N(alpha_hat_j, (F^-1)_jj); NaN for a component
        without a box.  Close to 1 wherever "a box prior on alpha_j" and "a flat prior normalised by the box" agree."""
        import torch

        a, _ = self.conditional(theta)
        on_host = not isinstance(a, torch.Tensor)
        a = torch.from_numpy(a) if on_host else a
        sd = torch.from_numpy(np.sqrt(np.diag(self.cov))).to(a.device)
        lo, hi = torch.from_numpy(self._lo).to(a.device), torch.from_numpy(self._hi).to(a.device)
        ndtr = lambda x: 0.5 * torch.erfc(-x / math.sqrt(2.0))
        mass = ndtr((hi - a) / sd) - ndtr((lo - a) / sd)
        return mass.numpy() if on_host else mass
