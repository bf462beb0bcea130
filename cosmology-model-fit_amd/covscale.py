"""
A free amplitude on the SN covariance: sample ``s`` in ``C(s) = C0 + s C1`` beside the cosmology, without refactorising.

The engine takes the supernova covariance as one Cholesky factor fixed at ``cf_create``, so every sampler treats the SN error
model as known.  The reference floats error-model nuisances wherever the covariance is small or diagonal (the quasar scripts'
intrinsic scatter, ``f_cc``, ``f_err``); for the dense SN block a new amplitude would need a new factor per likelihood call.
One scalar amplitude does not: with ``C0 = L0 L0^T`` the factor the engine holds, diagonalise once on the host,

    A = L0^-1 C1 L0^-T = Q diag(lambda) Q^T,        T = Q^T L0^-1,

and for a residual row ``r`` with ``y = T r``

    quad(s)   = r^T C(s)^-1 r      = sum_k y_k^2 / (1 + s lambda_k)
    logdet(s) = ln|C(s)| - ln|C0|  = sum_k log1p(s lambda_k)

valid while ``1 + s lambda_k > 0`` for every k (csrc/cosmofit_cscale.hip: the product on FP64 matrix cores with the first
reduction fused into its epilogue, then one wave per row; ``cf_cscale_eval_device``).  ``C1``: the identity (intrinsic scatter,
``s = sigma_int^2``), a 0/1 diagonal (the scatter of one survey or redshift range), a systematics matrix (``C0`` statistical,
``s`` the systematics amplitude), or any symmetric matrix (negative eigenvalues only bound ``s``).

* ``decompose(chol0, C1)``: ``(T, lam, info)`` on the host, numpy only.
* ``ScaledCovariance(engine, C1, s_bounds, power=1)``: the likelihood over ``[theta_engine..., p]`` with ``s = p ** power``.

Out of scope: two free amplitudes at once (two matrices do not diagonalise together); the BAO block, quasar engines and
engines over several devices; ``fit_report`` / ``influence`` / ``leaveout``, which go on describing ``C0``.  There is no CPU
fallback: the evaluation needs the engine's MI355X.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from ._args import ptr, stream_of

PROBE_LIMIT = 1e-11  # the limit cf_create's pack probe uses
MAX_S = L.CF_CSCALE_MAX_S



def _c1_matrix(C1, n: int) -> np.ndarray:
    c = np.asarray(C1, dtype=np.float64)
    if c.ndim == 0:
        return float(c) * np.eye(n)
    if c.shape == (n,):
        return np.diag(c)
    if c.shape != (n, n):
        raise ValueError(f"C1 must be a scalar, a vector [{n}] or a matrix [{n}, {n}], got shape {c.shape}")
    return 0.5 * (c + c.T)


def _lower_inverse(Lo: np.ndarray) -> np.ndarray:
    """Linv of a lower-triangular factor by forward substitution, one row at a time."""
    n = Lo.shape[0]
    X = np.zeros((n, n))
    for i in range(n):
        X[i, :i] = -(Lo[i, :i] @ X[:i, :i])
        X[i, i] = 1.0
        X[i, :i + 1] /= Lo[i, i]
    return X


def _quad_via_T(T, lam, r, s):
    y = T @ r
    return float(np.sum(y * y / (1.0 + s * lam)))


def decompose(chol0, C1):
    """``(T, lam, info)`` of ``C(s) = C0 + s C1`` with ``C0 = L0 L0^T``: ``T = Q^T L0^-1`` [n, n] and the eigenvalues ``lam`` [n]
    (ascending) of ``L0^-1 C1 L0^-T``, so that ``T C(s) T^T = I + s diag(lam)``.

    chol0: the Cholesky factor of C0; only its lower triangle is read.  C1: a scalar (times the identity), a vector (a diagonal)
    or a symmetric matrix [n, n].  Eigenvalues with ``|lam_k| <= n eps max|lam|`` are set to exactly 0, so that a rank-deficient
    C1 (scatter on a subset) puts no rounding-noise bound on s.  info: ``s_min = -1 / lam_max`` (or -inf), ``s_max = -1 / lam_min``
    (or +inf), ``n_zeroed``, and ``probe_rel``: on three probe vectors at s in {a point inside (s_min, 0), 0, 1 (or the middle of
    (0, s_max))} the largest ``|quad via T - quad via np.linalg.cholesky(C0 + s C1)| / quad``.  Raises above 1e-11."""
    Lo = np.tril(np.asarray(chol0, dtype=np.float64))
    if Lo.ndim != 2 or Lo.shape[0] != Lo.shape[1] or Lo.shape[0] < 1:
        raise ValueError("decompose takes a square Cholesky factor")
    n = Lo.shape[0]
    if not (np.isfinite(Lo).all() and (np.diag(Lo) > 0).all()):
        raise ValueError("the factor must be finite with a positive diagonal")
    c1 = _c1_matrix(C1, n)
    if not np.isfinite(c1).all():
        raise ValueError("C1 must be finite")
    Linv = _lower_inverse(Lo)
    A = Linv @ c1 @ Linv.T
    A = 0.5 * (A + A.T)
    lam, Q = np.linalg.eigh(A)
    T = Q.T @ Linv
    top = float(np.max(np.abs(lam)))
    noise = np.abs(lam) <= n * np.finfo(np.float64).eps * top
    lam = np.where(noise, 0.0, lam)
    lmax, lmin = float(lam.max()), float(lam.min())
    s_min = -1.0 / lmax if lmax > 0 else -np.inf
    s_max = -1.0 / lmin if lmin < 0 else np.inf
    inside = 0.5 * s_min if np.isfinite(s_min) else -0.5 * min(1.0, s_max)
    upper = 1.0 if s_max > 2.0 else 0.5 * s_max
    rng = np.random.default_rng(n)
    C0 = Lo @ Lo.T
    probe_rel = 0.0
    for _ in range(3):
        r = Lo @ rng.standard_normal(n)
        for s in (inside, 0.0, upper):
            Ls = np.linalg.cholesky(C0 + s * c1)
            z = np.linalg.solve(Ls, r)
            ref = float(z @ z)
            probe_rel = max(probe_rel, abs(_quad_via_T(T, lam, r, s) - ref) / ref)
    info = dict(s_min=float(s_min), s_max=float(s_max), n_zeroed=int(noise.sum()), probe_rel=float(probe_rel),
                probe_s=(float(inside), 0.0, float(upper)))
    if not probe_rel <= PROBE_LIMIT:
        raise ValueError(f"decompose: the probe of quad via T against a Cholesky factor of C0 + s C1 differs by {probe_rel:.2e} "
                         f"(limit {PROBE_LIMIT:.0e}): C0 is too ill-conditioned for this identity")
    return np.ascontiguousarray(T), np.ascontiguousarray(lam), info


class Decomposition:
    """``T`` and ``lam`` on one device (``cf_cscale``): the handle-free half, ``apply`` on caller-supplied residual rows."""

    def __init__(self, T, lam, device: int = 0):
        T = np.ascontiguousarray(T, dtype=np.float64)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if T.ndim != 2 or T.shape[0] != T.shape[1] or lam.shape != (T.shape[0],):
            raise ValueError("Decomposition takes T [n, n] and lam [n]")
        self.n, self.device = int(T.shape[0]), int(device)
        self._p = C.c_void_p()
        L.check(L.lib().cf_cscale_create(ptr(T), self.n, self.n, ptr(lam), self.device, C.byref(self._p)))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            L.lib().cf_cscale_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, rows, s, S: Optional[int] = None, want_y: bool = False, want=("quad", "logdet")):
        """(quad [S, n_s], logdet [S, n_s], y [S, n] or None) for rows[:S, :n] and the amplitudes s [S, n_s], asynchronous on
        torch's current stream (``cf_cscale_apply_device``).  rows: float64 [>= S, pitch >= n] on the device with contiguous
        columns; columns >= n and rows >= S are never read."""
        import torch

        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or rows.dim() != 2 or rows.stride(1) != 1:
            raise ValueError("apply takes a float64 tensor [S, >= n] with contiguous columns")
        if not rows.is_cuda or rows.device.index != self.device:
            raise ValueError("apply takes rows on the device of the decomposition")
        S = rows.shape[0] if S is None else int(S)
        if not 0 <= S <= rows.shape[0] or rows.shape[1] < self.n:
            raise ValueError("apply: S rows of at least n columns")
        if s.dtype != torch.float64 or s.dim() != 2 or s.shape[0] != S or not s.is_contiguous() or s.device != rows.device:
            raise ValueError("apply takes the amplitudes as a contiguous float64 tensor [S, n_s] on the rows' device")
        n_s = s.shape[1]
        f64 = dict(dtype=torch.float64, device=rows.device)
        quad = torch.empty((S, n_s), **f64) if "quad" in want else None
        logdet = torch.empty((S, n_s), **f64) if "logdet" in want else None
        y = torch.empty((S, self.n), **f64) if want_y else None
        dptr = lambda t: None if t is None else t.data_ptr()
        with torch.cuda.device(rows.device):
            L.check(L.lib().cf_cscale_apply_device(self._p, rows.data_ptr(), rows.stride(0), S, s.data_ptr(), n_s, dptr(quad),
                                                   dptr(logdet), dptr(y), stream_of(rows.device)))
        return quad, logdet, y


def set_library_chunk(engine, rows: int = 0):
    """Rows per chunk of the library's own loop over the workspace (0: the default, ``_lib.CF_CSCALE_CHUNK``).  No result depends
    on it; tests lower it to cross chunk boundaries with few rows."""
    L.check(L.lib().cf_cscale_set_chunk(engine._h, int(rows)))


class ScaledCovariance:
    """The engine's likelihood with the SN covariance ``C0 + s C1``.  The sampled vector is ``[theta_engine..., p]`` with
    ``s = p ** power`` (power = 2 makes p an intrinsic scatter in magnitudes when C1 is the identity or a 0/1 diagonal).

    The factor of C0 is the one the engine was built with (``engine.mock_data["sn_chol"]``).  The prior is flat in p (not
    normalised) over ``s_bounds = (s_lo, s_hi)``, intersected with the open domain ``(s_min, s_max)`` of the decomposition;
    ``bounds_cut`` says whether that cut them (a warning is issued too).  Outside the bounds ``log_probability`` is -inf.  Every
    other block, constant and prior term is the engine's own."""

    def __init__(self, engine, C1, s_bounds: Sequence[float], power: int = 1):
        info = getattr(engine, "model_info", {})
        if info.get("quasar"):
            raise ValueError("ScaledCovariance: a quasar engine has no dense SN covariance to scale")
        if info.get("multi_device"):
            raise ValueError("ScaledCovariance: this engine spans several devices; use one engine per device")
        chol = getattr(engine, "mock_data", {}).get("sn_chol")
        if chol is None or not getattr(engine, "n_sn", 0):
            raise ValueError("ScaledCovariance: this engine has no SN block")
        if power not in (1, 2):
            raise ValueError("power must be 1 (p = s) or 2 (p = sqrt(s))")
        lo, hi = (float(v) for v in s_bounds)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("s_bounds must be a finite interval (s_lo, s_hi)")
        if power == 2 and lo < 0:
            raise ValueError("power = 2 samples p = sqrt(s): s_bounds must not go below 0")
        self.engine, self.power, self.ndim = engine, int(power), int(engine.ndim) + 1
        T, lam, self.info = decompose(chol, C1)
        self._lam, self.transform = lam, T  # T [n, n]: y = T r
        # the open domain, pulled in by a relative 1e-9 so that the box itself is inside it
        d_lo, d_hi = self.info["s_min"], self.info["s_max"]
        cut_lo = d_lo * (1 - 1e-9) if np.isfinite(d_lo) else -np.inf
        cut_hi = d_hi * (1 - 1e-9) if np.isfinite(d_hi) else np.inf
        self.bounds_cut = lo < cut_lo or hi > cut_hi
        self.s_bounds = (max(lo, cut_lo), min(hi, cut_hi))
        if self.bounds_cut:
            warnings.warn(f"ScaledCovariance: s_bounds ({lo:g}, {hi:g}) cut to the domain of the decomposition, "
                          f"({self.s_bounds[0]:g}, {self.s_bounds[1]:g})")
        if not self.s_bounds[0] < self.s_bounds[1]:
            raise ValueError("s_bounds does not meet the domain (s_min, s_max) of the decomposition")
        self.p_bounds = self.s_bounds if power == 1 else (float(np.sqrt(self.s_bounds[0])), float(np.sqrt(self.s_bounds[1])))
        self._dec = Decomposition(T, lam, device=int(engine.info()["device"]))

    # ---- lifetime --------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_dec", None) is not None:
            self._dec.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def eigenvalues(self) -> np.ndarray:
        """lambda [n], ascending, rounding-noise ones exactly 0."""
        return self._lam.copy()

    @property
    def s_range(self):
        """(s_min, s_max): the open interval on which C(s) is positive definite."""
        return self.info["s_min"], self.info["s_max"]

    # ---- host numpy ------------------------------------------------------------------------------------------------------------
    def _split(self, theta_ext):
        x = np.asarray(theta_ext, dtype=np.float64)
        single = x.ndim == 1
        x = np.atleast_2d(x)
        if x.ndim != 2 or x.shape[1] != self.ndim:
            raise ValueError(f"theta must have {self.ndim} columns (the engine's {self.ndim - 1} and p), got {x.shape}")
        p = x[:, -1]
        return single, np.ascontiguousarray(x[:, :-1]), p, np.ascontiguousarray(p ** self.power)

    def _host(self, theta, s, kind, want_parts=False):
        """cf_cscale_eval on host rows theta [W, ndim] and amplitudes s [W, n_s]."""
        W, n_s = s.shape
        out = np.empty((W, n_s))
        parts = np.empty((W, n_s, 2)) if want_parts else None
        L.check(L.lib().cf_cscale_eval(self.engine._h, self._dec._p, ptr(theta), ptr(s), n_s, W, kind, ptr(out), ptr(parts)))
        return out, parts

    def _eval(self, theta_ext, kind):
        single, theta, p, s = self._split(theta_ext)
        out = self._host(theta, s[:, None].copy(), kind)[0][:, 0]
        if kind == L.CF_OUT_LOGP:
            out = np.where((p > self.p_bounds[0]) & (p < self.p_bounds[1]), out, -np.inf)
        return float(out[0]) if single else out

    def chi_squared(self, theta_ext):
        """The engine's chi^2 with its SN term replaced by quad(s); one row [ndim + 1] -> float, or [W, ndim + 1] -> [W]."""
        return self._eval(theta_ext, L.CF_OUT_CHI2)

    def log_likelihood(self, theta_ext):
        """The engine's log L plus 0.5 chi2_SN(C0) - 0.5 (quad + logdet); -inf where s leaves the domain."""
        return self._eval(theta_ext, L.CF_OUT_LOGL)

    def log_probability(self, theta_ext):
        """The engine's log P with the same replacement, and -inf where p leaves its bounds."""
        return self._eval(theta_ext, L.CF_OUT_LOGP)

    def log_probs_vectorized(self, theta_ext):
        return self.log_probability(np.atleast_2d(theta_ext))

    def parts(self, theta_ext, want_y: bool = False) -> dict:
        """quad and logdet [W] of the rows (numpy); with want_y also y = T r [W, n]."""
        single, theta, p, s = self._split(theta_ext)
        _, parts = self._host(theta, s[:, None].copy(), L.CF_OUT_CHI2, want_parts=True)
        res = dict(quad=parts[:, 0, 0], logdet=parts[:, 0, 1], s=s)
        if want_y:
            import torch

            dev = torch.device("cuda", self._dec.device)
            rows = torch.from_numpy(np.ascontiguousarray(self.engine.parts(theta)["delta"])).to(dev)
            with torch.cuda.device(dev):
                res["y"] = self._dec.apply(rows, torch.from_numpy(s[:, None].copy()).to(dev), want_y=True, want=())[2].cpu().numpy()
        return res

    # ---- device ----------------------------------------------------------------------------------------------------------------
    def _device(self, theta, s, kind):
        import torch

        out = torch.empty(s.shape, dtype=torch.float64, device=theta.device)
        if theta.shape[0]:
            with torch.cuda.device(theta.device):
                L.check(L.lib().cf_cscale_eval_device(self.engine._h, self._dec._p, theta.data_ptr(), s.data_ptr(), s.shape[1],
                                                      theta.shape[0], kind, out.data_ptr(), None,
                                                      stream_of(theta.device)))
        return out

    def torch_log_prob(self, kind: int = L.CF_OUT_LOGP):
        """Callable ``f(x: cuda float64 tensor [W, ndim + 1]) -> tensor [W]``, asynchronous on torch's current stream: what
        ``ShardedEnsemble``, ``replicas``, ``optimize.best_fit`` / ``profile`` and ``nested.DeviceNestedSampler`` take."""
        import torch

        lo, hi = self.p_bounds

        def f(x):
            if not x.is_cuda or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != self.ndim:
                raise ValueError(f"theta must be a float64 tensor [W, {self.ndim}] on the engine's GPU")
            theta = x[:, :-1].contiguous()
            p = x[:, -1]
            s = (p if self.power == 1 else p * p).contiguous()[:, None]
            out = self._device(theta, s, kind)[:, 0]
            if kind == L.CF_OUT_LOGP:
                out = torch.where((p > lo) & (p < hi), out, torch.full_like(out, -float("inf")))
            return out

        return f

    def scan(self, theta, s_grid, kind: int = L.CF_OUT_LOGL):
        """[W, len(s_grid)] values of `kind` (log L by default) for the engine rows theta [W, ndim] at every amplitude of the
        grid: the profile or the marginal over s for every sample of an existing chain.  Grids longer than 16 are split over
        calls; within a call the product is done once.  theta: a cuda tensor (the result is one too) or host numbers."""
        import torch

        grid = np.asarray(s_grid, dtype=np.float64).reshape(-1)
        if grid.size < 1:
            raise ValueError("scan needs at least one amplitude")
        on_host = not isinstance(theta, torch.Tensor)
        if on_host:
            th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
            theta = torch.from_numpy(np.ascontiguousarray(th)).to(torch.device("cuda", self._dec.device))
        if theta.dim() != 2 or theta.shape[1] != self.ndim - 1 or theta.dtype != torch.float64 or not theta.is_cuda:
            raise ValueError(f"scan takes engine rows [W, {self.ndim - 1}] (float64)")
        theta = theta.contiguous()
        W = theta.shape[0]
        cols = []
        for j0 in range(0, grid.size, MAX_S):
            g = torch.from_numpy(grid[j0:j0 + MAX_S]).to(theta.device)
            cols.append(self._device(theta, g[None, :].expand(W, -1).contiguous(), kind))
        out = torch.cat(cols, dim=1)
        return out.cpu().numpy() if on_host else out
