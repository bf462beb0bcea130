"""
Template scans: which of K candidate templates do the SN data prefer, and how significant is the best one once the search is
accounted for?

``nuisance`` answers "what happens with THIS template in the model" for up to 16 templates treated jointly.  A scan asks the
other question: every member of a family -- every redshift step, every window of bins, every hemisphere or sky patch, every
single datum -- is tried ONE AT A TIME on top of a base model, for every row of a chain or every null draw.  With ``C = L L^T``
the SN covariance, ``K = C^-1``, base templates ``A0 [n, m0]`` (precisions ``P0``, prior means 0) and candidates ``a_k``
(optional zero-mean Gaussian priors of width ``sigma_k``):

    F0  = A0^T K A0 + P0                  K' = K - K A0 F0^-1 A0^T K        (= K - Wt Wt^T with ``nuisance.project``'s Wt)
    g_k = K' a_k      F_k = a_k^T g_k + 1 / sigma_k^2      v_k = g_k / sqrt(F_k)              (once, on the host: ``prepare``)
    s_k(row) = v_k^T r0                   the signed z-score of candidate k given the base
    dchi2_k  = s_k^2 = chi2_prof(base) - chi2_prof(base + a_k)      alpha_hat_k = s_k / sqrt(F_k),  error 1 / sqrt(F_k)

(csrc/cosmofit_scan.hip: one FP64 matrix-core product per chunk with the reductions fused behind it; the [S, K] map reaches
memory only when asked for).  Under the null and flat priors ``s_k ~ N(0, 1)``; a null residual is ``L xi`` with
``xi ~ N(0, I)``, so ``null_matrix = L^T V`` turns the device generator's normals into null scores with the same kernel, and

    p_global = (1 + #{null best >= observed best}) / (1 + n_draws)

is the look-elsewhere-corrected p-value of the winner.  A candidate the base already spans is *dead*: no prior on its amplitude
and ``a_k^T g_k <= 1e-12 a_k^T K a_k``.  Its column of V is zero, its score exactly 0.0, and it never wins.

``base_jacobian=theta_ref`` appends the columns ``d r0 / d theta_j`` (central differences of ``engine.parts``' residual rows)
to the base: the scores are then profiled over the cosmology to first order, null draws included.

A DIPOLE direction scan does not belong here: the templates ``c_i (n_i . d)`` span three columns for every direction d, so
``nuisance`` with m = 3 covers them all at once.  Hemispheres, caps, steps and windows are not linear in their parameters and
do need the scan.

Out of scope: BAO / CMB / quasar blocks; candidates that enter non-linearly (their linearisation is the caller's template);
joint fits of several candidates (hand the winner to ``nuisance``); combining with ``covscale``; engines over several devices.
There is no CPU fallback: the evaluation needs the engine's MI355X.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from . import nuisance as N
from ._args import ptr, stream_of

PROBE_LIMIT = N.PROBE_LIMIT    # the limit ``nuisance.project`` uses
DEAD_REL = 1e-12               # a candidate is dead when a^T K' a <= DEAD_REL a^T K a (and it has no prior)
MAX_BASE = N.MAX_M
LD = np.longdouble
_SCAN_TAG = 0x5343414E4E554C31  # "SCANNUL1": the domain tag of the null draws
_NULL_PIECE = 4096

__all__ = ["prepare", "null_matrix", "Candidates", "Scan", "TemplateScan", "null_key", "global_p", "set_library_chunk",
           "statistic", "MAX_BASE"]


# ---- host algebra -----------------------------------------------------------------------------------------------------------
def _columns(a, n, what):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[0] != n:
        raise ValueError(f"{what} must be [{n}, k], got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} must be finite")
    return np.ascontiguousarray(a)


def _widths(sigma, m, what):
    s = np.full(m, np.inf) if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (m,)).copy()
    if not ((s > 0) & ~np.isnan(s)).all():
        raise ValueError(f"{what} must be > 0; inf marks a flat prior")
    return s


def _ld_cholesky(F):
    m = F.shape[0]
    LF = np.zeros((m, m), dtype=LD)
    for j in range(m):
        d = F[j, j] - LF[j, :j] @ LF[j, :j]
        LF[j, j] = np.sqrt(d)
        LF[j + 1:, j] = (F[j + 1:, j] - LF[j + 1:, :j] @ LF[j, :j]) / LF[j, j]
    return LF


def _probe_columns(K):
    return np.unique(np.round(np.linspace(0, K - 1, min(K, 8))).astype(np.int64))


def prepare(chol, cand, base=None, base_sigma=None, cand_sigma=None, base_mu=None) -> dict:
    """The host algebra: ``dict(V [n, K], F [K], live [K] bool, aKa [K], probe_rel, probe_columns, m0, Wt)`` for the Cholesky
    factor ``chol`` of the SN covariance (only its lower triangle is read), candidates ``cand [n, K]``, base templates
    ``base [n, m0]`` (0 <= m0 <= 16; None: no base) with prior widths ``base_sigma [m0]`` (default and inf: flat), and prior
    widths ``cand_sigma`` (a scalar or [K]) on the candidates' amplitudes.  Prior means are zero: a non-zero ``base_mu`` is
    refused (shift the data instead).

    ``G = K' A_cand`` is formed in float64 with LAPACK triangular solves and the deflation ``nuisance.project`` provides.
    Thousands of columns are too many for long-double substitutions, so the result is probed: for at least 8 columns (the first
    and the last among them) and three probe rows r, ``|r^T v_k - s_k|`` with ``s_k`` from the definitions in long double,
    relative to ``max_k sum_i |r_i| |V_ik|``.  Raises above 1e-11.

    A candidate the base spans (``a^T K' a <= 1e-12 a^T K a``) has a zero column of V.  Without a prior it is dead (``live``
    False, F = 0); with one it stays live with F = 1 / sigma^2 and a score of exactly 0.0, which is its score up to 1e-12."""
    from scipy.linalg import solve_triangular

    Lo = np.tril(np.asarray(chol, dtype=np.float64))
    if Lo.ndim != 2 or Lo.shape[0] != Lo.shape[1] or Lo.shape[0] < 1:
        raise ValueError("prepare takes a square Cholesky factor")
    n = Lo.shape[0]
    if not (np.isfinite(Lo).all() and (np.diag(Lo) > 0).all()):
        raise ValueError("the factor must be finite with a positive diagonal")
    A = _columns(cand, n, "cand")
    K = A.shape[1]
    if not 1 <= K <= L.CF_SCAN_MAX_K:
        raise ValueError("the scan takes 1 <= K < 2^24 candidates")
    sig = _widths(cand_sigma, K, "cand_sigma")
    prec = np.where(np.isfinite(sig), 1.0 / np.where(np.isfinite(sig), sig, 1.0) ** 2, 0.0)
    if base_mu is not None and np.any(np.asarray(base_mu, dtype=np.float64) != 0.0):
        raise ValueError("the scan takes base priors of mean zero: subtract A0 mu from the data instead")
    Y = solve_triangular(Lo, A, lower=True)
    aKa = np.einsum("ik,ik->k", Y, Y)
    G = solve_triangular(Lo, Y, lower=True, trans="T")
    m0, Wt, A0, s0 = 0, np.zeros((n, 0)), np.zeros((n, 0)), np.zeros(0)
    if base is not None and np.size(base):
        A0 = _columns(base, n, "base")
        m0 = A0.shape[1]
        if m0 > MAX_BASE:
            raise ValueError(f"the base takes at most {MAX_BASE} templates, got {m0}")
        s0 = _widths(base_sigma, m0, "base_sigma")
        Wt = N.project(Lo, A0, sigma=s0)["Wt"]
        G = G - Wt @ (Wt.T @ A)
    aga = np.einsum("ik,ik->k", A, G)
    spanned = aga <= DEAD_REL * aKa   # what is left of g_k is the rounding of a complete cancellation: taken as zero
    live = ~((prec == 0.0) & spanned)
    G[:, spanned] = 0.0
    F = np.where(live, np.where(spanned, 0.0, aga) + prec, 0.0)
    if not (F[live] > 0).all():
        raise ValueError("prepare: a candidate with a prior has a negative a^T K' a: the base is too ill-conditioned")
    V = np.where(live[None, :], G / np.sqrt(np.where(live, F, 1.0))[None, :], 0.0)
    res = dict(V=np.ascontiguousarray(V), F=F, live=live, aKa=aKa, m0=m0, Wt=Wt, n=n, K=K)
    # the probe: long-double definitions on a few columns
    cols = _probe_columns(K)
    Ll = np.asarray(Lo, dtype=LD)
    solve_c = lambda B: N._solve_upper_t(Ll, N._solve_lower(Ll, np.asarray(B, dtype=LD)))
    Ac = np.asarray(A[:, cols], dtype=LD)
    Gc = solve_c(Ac)
    if m0:
        A0l = np.asarray(A0, dtype=LD)
        KA0 = solve_c(A0l)
        P0 = np.where(np.isfinite(s0), LD(1) / np.asarray(np.where(np.isfinite(s0), s0, 1.0), dtype=LD) ** 2, LD(0))
        F0 = A0l.T @ KA0 + np.diag(P0)
        LF = _ld_cholesky(LD(0.5) * (F0 + F0.T))
        Gc = Gc - KA0 @ N._solve_upper_t(LF, N._solve_lower(LF, KA0.T @ Ac))
    Fc = np.einsum("ik,ik->k", Ac, Gc) + np.asarray(prec[cols], dtype=LD)
    rng = np.random.default_rng(n + 1000 * K + m0)
    probe_rel = 0.0
    for _ in range(3):
        r = Lo @ rng.standard_normal(n)
        scale = float(np.max(np.abs(r) @ np.abs(V)))
        for j, k in enumerate(cols):
            if spanned[k] or scale == 0.0:
                continue
            ref = (np.asarray(r, dtype=LD) @ Gc[:, j]) / np.sqrt(Fc[j])
            probe_rel = max(probe_rel, abs(float(LD(r @ V[:, k]) - ref)) / scale)
    res["probe_rel"], res["probe_columns"] = probe_rel, cols
    if not probe_rel <= PROBE_LIMIT:
        raise ValueError(f"prepare: the probe of r^T v_k against the long-double definitions differs by {probe_rel:.2e} of the "
                         f"terms summed (limit {PROBE_LIMIT:.0e}): the covariance is too ill-conditioned for this identity")
    return res


def null_matrix(chol, V) -> np.ndarray:
    """``L^T V``: applied to standard normals xi it gives the scores of the null residual ``L xi``."""
    return np.ascontiguousarray(np.tril(np.asarray(chol, dtype=np.float64)).T @ np.asarray(V, dtype=np.float64))


def statistic(s, sign: int = 0):
    """The statistic of signed scores: s^2 (sign 0), max(s, 0)^2 (sign +1), max(-s, 0)^2 (sign -1)."""
    s = np.asarray(s)
    u = s if sign == 0 else np.maximum(s, 0.0) if sign > 0 else np.maximum(-s, 0.0)
    return u * u


def null_key(seed: int) -> int:
    """Unsigned 64-bit key of the null draws of ``TemplateScan.null(seed=)``: ``mocks.normals(key, n_draws, n, k0=row0)``."""
    return N._mix(N._mix((int(seed) * N._GOLDEN + _SCAN_TAG) & N._U64))


def global_p(observed: float, null, sign: int = 0, level: float = 0.6827) -> dict:
    """The look-elsewhere arithmetic: p_global = (1 + #{null >= observed}) / (1 + n_draws) with its Clopper-Pearson interval
    at `level`, the equivalent two-sided Gaussian sigma, the local sigma sqrt(observed), p_local (the chi^2_1 tail; half of it
    for a one-sided scan) and the effective number of trials p_global / p_local."""
    from scipy import stats

    from . import mocks

    null = np.asarray(null, dtype=np.float64).reshape(-1)
    observed = float(observed)
    if null.size < 1 or not np.isfinite(null).all() or not (math.isfinite(observed) and observed >= 0.0):
        raise ValueError("the observed statistic must be finite and >= 0 and the null values finite, at least one draw")
    x = int(np.sum(null >= observed))
    p = (1 + x) / (1 + null.size)
    lo, hi = mocks.clopper_pearson(x, null.size, level)
    p_local = float(stats.chi2.sf(observed, 1)) * (1.0 if sign == 0 else 0.5)
    return dict(p_global=p, p_interval=(lo, hi), sigma_global=mocks.sigma_of_p(p), local_sigma=math.sqrt(observed),
                p_local=p_local, n_trials=(p / p_local if p_local > 0 else math.inf), n_draws=int(null.size), n_exceed=x,
                level=level)


# ---- candidate families -----------------------------------------------------------------------------------------------------
class Candidates:
    """Builders of candidate families.  Each returns ``(cols [n, K], table)``; ``table`` is a list of K dicts describing the
    columns.  ``stack`` puts families side by side, ``times`` weights one."""

    @staticmethod
    def steps(z, thresholds=None):
        """1 for ``z > z_t``.  Default thresholds: the midpoints between distinct sorted redshifts."""
        z = np.asarray(z, dtype=np.float64).reshape(-1)
        if thresholds is None:
            u = np.unique(z)
            thresholds = 0.5 * (u[1:] + u[:-1])
        t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        cols = (z[:, None] > t[None, :]).astype(np.float64)
        return cols, [dict(kind="step", z_t=float(v)) for v in t]

    @staticmethod
    def windows(z, edges, max_bins=None):
        """1 for ``edges[i] <= z < edges[j]``, every i < j (with j - i <= max_bins when given)."""
        z = np.asarray(z, dtype=np.float64).reshape(-1)
        e = np.asarray(edges, dtype=np.float64).reshape(-1)
        if e.size < 2 or not (np.diff(e) > 0).all():
            raise ValueError("windows takes at least two strictly ascending edges")
        pairs = [(i, j) for i in range(e.size - 1) for j in range(i + 1, e.size) if max_bins is None or j - i <= int(max_bins)]
        cols = np.stack([((z >= e[i]) & (z < e[j])).astype(np.float64) for i, j in pairs], axis=1)
        return cols, [dict(kind="window", lo=float(e[i]), hi=float(e[j]), bins=j - i) for i, j in pairs]

    @staticmethod
    def _unit(v, what):
        v = np.atleast_2d(np.asarray(v, dtype=np.float64))
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError(f"{what} must be [k, 3]")
        norm = np.linalg.norm(v, axis=1)
        if not (norm > 0).all():
            raise ValueError(f"{what} must not hold a zero vector")
        return v / norm[:, None]

    @staticmethod
    def hemispheres(dirs, centres):
        """``sign(n . d)``: +1 on the hemisphere of each centre, -1 opposite, 0 on its equator."""
        n, c = Candidates._unit(dirs, "dirs"), Candidates._unit(centres, "centres")
        return np.sign(n @ c.T), [dict(kind="hemisphere", centre=tuple(map(float, v))) for v in c]

    @staticmethod
    def caps(dirs, centres, radii_deg):
        """1 inside the cap of each radius (degrees) about each centre, ``n . d >= cos(radius)``; centres major, radii minor."""
        n, c = Candidates._unit(dirs, "dirs"), Candidates._unit(centres, "centres")
        rad = np.asarray(radii_deg, dtype=np.float64).reshape(-1)
        if not ((rad > 0) & (rad <= 180)).all():
            raise ValueError("radii must be in (0, 180] degrees")
        dot = n @ c.T
        cols = (dot[:, :, None] >= np.cos(np.deg2rad(rad))[None, None, :]).astype(np.float64).reshape(n.shape[0], -1)
        return cols, [dict(kind="cap", centre=tuple(map(float, v)), radius_deg=float(r)) for v in c for r in rad]

    @staticmethod
    def labels(ids):
        """One 0/1 column per distinct label (sorted): a survey, a host type, a calibration group."""
        ids = np.asarray(ids).reshape(-1)
        u = np.unique(ids)
        return (ids[:, None] == u[None, :]).astype(np.float64), [dict(kind="label", label=v.item()) for v in u]

    @staticmethod
    def singles(n: int):
        """One column per datum: the identity.  With no base its scores are ``influence``'s z_i."""
        return np.eye(int(n)), [dict(kind="single", index=i) for i in range(int(n))]

    @staticmethod
    def fibonacci_sphere(N_pts: int) -> np.ndarray:
        """N nearly uniform unit vectors [N, 3] (the golden-angle spiral): centres for ``hemispheres`` and ``caps``."""
        N_pts = int(N_pts)
        if N_pts < 1:
            raise ValueError("fibonacci_sphere needs N >= 1")
        i = np.arange(N_pts) + 0.5
        zc = 1.0 - 2.0 * i / N_pts
        phi = math.pi * (3.0 - math.sqrt(5.0)) * i
        rho = np.sqrt(np.maximum(0.0, 1.0 - zc * zc))
        return np.column_stack([rho * np.cos(phi), rho * np.sin(phi), zc])

    @staticmethod
    def times(family, weight):
        """A family with every column multiplied by a per-SN weight [n]: an attenuation with redshift, a survey mask."""
        cols, table = family
        w = np.asarray(weight, dtype=np.float64).reshape(-1)
        if w.shape[0] != cols.shape[0]:
            raise ValueError("times takes one weight per SN")
        return cols * w[:, None], [dict(t, weighted=True) for t in table]

    @staticmethod
    def stack(*families):
        return (np.ascontiguousarray(np.concatenate([f[0] for f in families], axis=1)), [t for f in families for t in f[1]])


# ---- the device object ------------------------------------------------------------------------------------------------------
class Scan:
    """``V`` and the live flags on one device (``cf_scan``): the handle-free half, ``apply`` on caller-supplied rows."""

    def __init__(self, V, live=None, device: int = 0):
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.ndim != 2:
            raise ValueError("Scan takes V [n, K]")
        self.n, self.K, self.device = int(V.shape[0]), int(V.shape[1]), int(device)
        lv = None if live is None else np.ascontiguousarray(np.asarray(live, dtype=bool).astype(np.uint8))
        if lv is not None and lv.shape != (self.K,):
            raise ValueError("live must be [K]")
        self._p = C.c_void_p()
        L.check(L.lib().cf_scan_create(ptr(V), self.n, self.K, self.K, ptr(lv), self.device, C.byref(self._p)))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            L.lib().cf_scan_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def apply(self, rows, S: Optional[int] = None, sign: int = 0, weights=None, want=("best", "best_k", "s_best"), colacc=None):
        """dict of the outputs named in `want` ("best", "best_k", "s_best" [S], "map" [S, K]) for rows[:S, :n], asynchronous on
        torch's current stream (``cf_scan_apply_device``).  rows: float64 [>= S, pitch >= n] on the device with contiguous
        columns; columns >= n and rows >= S are never read.  colacc: a float64 tensor [2 K + 1] of running accumulators the
        call adds to (weights [S] or ones)."""
        import torch

        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float64 or rows.dim() != 2 or rows.stride(1) != 1:
            raise ValueError("apply takes a float64 tensor [S, >= n] with contiguous columns")
        if not rows.is_cuda or rows.device.index != self.device:
            raise ValueError("apply takes rows on the device of the scan")
        S = rows.shape[0] if S is None else int(S)
        if not 0 <= S <= rows.shape[0] or rows.shape[1] < self.n:
            raise ValueError("apply: S rows of at least n columns")
        out = _outputs(S, self.K, rows.device, want)
        _check_side(weights, colacc, S, self.K, rows.device)
        dptr = lambda x: None if x is None else x.data_ptr()
        with torch.cuda.device(rows.device):
            L.check(L.lib().cf_scan_apply_device(self._p, rows.data_ptr(), rows.stride(0), S, int(sign), dptr(weights),
                                                 dptr(out.get("best")), dptr(out.get("best_k")), dptr(out.get("s_best")),
                                                 dptr(out.get("map")), self.K, dptr(colacc), stream_of(rows.device)))
        return out


_WANT = ("best", "best_k", "s_best", "map", "chi2")


def _outputs(S, K, device, want):
    import torch

    unknown = set(want) - set(_WANT)
    if unknown:
        raise ValueError(f"want must be among {_WANT}, got {sorted(unknown)}")
    shape = {"map": (S, K)}
    return {k: torch.empty(shape.get(k, (S,)), dtype=torch.int32 if k == "best_k" else torch.float64, device=device) for k in want}


def _check_side(weights, colacc, S, K, device):
    import torch

    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64 or weights.shape != (S,)
                                or not weights.is_contiguous() or weights.device != device):
        raise ValueError("weights must be a contiguous float64 tensor [S] on the rows' device")
    if colacc is not None and (not isinstance(colacc, torch.Tensor) or colacc.dtype != torch.float64 or colacc.shape != (2 * K + 1,)
                               or not colacc.is_contiguous() or colacc.device != device):
        raise ValueError("colacc must be a contiguous float64 tensor [2 K + 1] on the rows' device")


def set_library_chunk(engine, rows: int = 0):
    """Rows per chunk of the library's own loop over the workspace (0: the default, ``_lib.CF_SCAN_CHUNK``).  No score depends
    on it; tests lower it to cross chunk boundaries with few rows."""
    L.check(L.lib().cf_scan_set_chunk(engine._h, int(rows)))


class TemplateScan:
    """The scan of the candidates ``cand`` (an array [n, K], or a ``Candidates`` family ``(cols, table)``) on the SN block of
    ``engine``, on top of ``base`` templates (prior widths ``base_sigma``) and, with ``base_jacobian=theta_ref``, the
    first-order cosmology refit (``jacobian_free``: the coordinates of theta that are free under the null model; default all).
    sign: 0 two-sided, +1 / -1 one-sided.  The factor is the one the engine was built with.

    It is a report on an engine, not a likelihood: it carries no ``.engine`` attribute."""

    def __init__(self, engine, cand, base=None, base_sigma=None, cand_sigma=None, base_jacobian=None, sign: int = 0,
                 jacobian_step: float = 1e-4, jacobian_free: Optional[Sequence[int]] = None):
        info = getattr(engine, "model_info", {})
        if info.get("quasar"):
            raise ValueError("TemplateScan: a quasar engine has no dense SN block to scan")
        if info.get("multi_device"):
            raise ValueError("TemplateScan: this engine spans several devices; use one engine per device")
        chol = getattr(engine, "mock_data", {}).get("sn_chol")
        if chol is None or not getattr(engine, "n_sn", 0):
            raise ValueError("TemplateScan: this engine has no SN block")
        if sign not in (-1, 0, 1):
            raise ValueError("sign must be -1, 0 or +1")
        cols, table = cand if isinstance(cand, tuple) else (cand, None)
        self._engine, self.sign, self.ndim, self.n = engine, int(sign), int(engine.ndim), int(engine.n_sn)
        cols = _columns(cols, self.n, "cand")
        self.table = table if table is not None else [dict(kind="column", index=k) for k in range(cols.shape[1])]
        if len(self.table) != cols.shape[1]:
            raise ValueError("the table must have one entry per candidate")
        base = np.zeros((self.n, 0)) if base is None else _columns(base, self.n, "base")
        sig = _widths(base_sigma, base.shape[1], "base_sigma")
        self.jacobian, self.jacobian_kept = None, ()
        if base_jacobian is not None:
            J = self._jacobian(np.asarray(base_jacobian, dtype=np.float64), float(jacobian_step))
            if jacobian_free is not None:  # the coordinates the null model leaves free; the others stay at theta_ref
                free = sorted({int(j) for j in jacobian_free})
                if not free or free[0] < 0 or free[-1] >= self.ndim:
                    raise ValueError(f"jacobian_free must name coordinates in 0 .. {self.ndim - 1}")
                J = J[:, free]
            if base.shape[1] + J.shape[1] > MAX_BASE:
                raise ValueError(f"base templates plus free cosmology parameters must stay <= {MAX_BASE}")
            self.jacobian = J
            keep = self._independent(chol, base, J)
            self.jacobian_kept = tuple(keep)
            base = np.column_stack([base, J[:, keep]])
            sig = np.concatenate([sig, np.full(len(keep), np.inf)])
        self.base = base
        self.info = prepare(chol, cols, base=base if base.shape[1] else None, base_sigma=sig, cand_sigma=cand_sigma)
        self.K = int(self.info["K"])
        self.device = int(engine.info()["device"])
        self._chol = np.tril(np.asarray(chol, dtype=np.float64))
        self._scan = Scan(self.info["V"], self.info["live"], device=self.device)
        self._null = None

    # ---- lifetime ----------------------------------------------------------------------------------------------------------
    def close(self):
        for s in (getattr(self, "_scan", None), getattr(self, "_null", None)):
            if s is not None:
                s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- the cosmology Jacobian --------------------------------------------------------------------------------------------
    def _jacobian(self, theta_ref, rel_step):
        """d r0 / d theta_j [n, ndim] by central differences of ``engine.parts``' residual rows (host)."""
        if theta_ref.shape != (self.ndim,):
            raise ValueError(f"base_jacobian takes theta_ref [{self.ndim}]")
        h = rel_step * np.maximum(np.abs(theta_ref), 1.0)
        pts = np.repeat(theta_ref[None, :], 2 * self.ndim, axis=0)
        for j in range(self.ndim):
            pts[2 * j, j] += h[j]
            pts[2 * j + 1, j] -= h[j]
        rows = np.asarray(self._engine.parts(pts)["delta"], dtype=np.float64)[:, :self.n]
        if not np.isfinite(rows).all():
            raise ValueError("base_jacobian: the residual rows about theta_ref are not finite (theta_ref too close to the box?)")
        return np.stack([(rows[2 * j] - rows[2 * j + 1]) / (2.0 * h[j]) for j in range(self.ndim)], axis=1)

    @staticmethod
    def _independent(chol, base, J, tol=1e-8):
        """The Jacobian columns that are not combinations of the base and the columns before them, in the metric of the
        covariance (the offset and H0 columns of an SN-only engine coincide up to a factor: one of them is enough)."""
        from scipy.linalg import solve_triangular

        Lo = np.tril(np.asarray(chol, dtype=np.float64))
        Q = []
        for a in base.T:
            y = solve_triangular(Lo, a, lower=True)
            for q in Q:
                y = y - q * (q @ y)
            nrm = np.linalg.norm(y)
            if nrm > 0:
                Q.append(y / nrm)
        keep = []
        for j in range(J.shape[1]):
            y0 = solve_triangular(Lo, J[:, j], lower=True)
            y = y0.copy()
            for _ in range(2):
                for q in Q:
                    y = y - q * (q @ y)
            if np.linalg.norm(y) > tol * np.linalg.norm(y0):
                Q.append(y / np.linalg.norm(y))
                keep.append(j)
        return keep

    # ---- evaluation --------------------------------------------------------------------------------------------------------
    def _theta_tensor(self, x):
        import torch

        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != self.ndim:
            raise ValueError(f"theta must be a float64 tensor [S, {self.ndim}] on the engine's GPU")
        return x.contiguous()

    def _device(self, theta, want, weights=None, colacc=None):
        import torch

        S = theta.shape[0]
        out = _outputs(S, self.K, theta.device, want)
        _check_side(weights, colacc, S, self.K, theta.device)
        dptr = lambda x: None if x is None else x.data_ptr()
        if S:
            with torch.cuda.device(theta.device):
                L.check(L.lib().cf_scan_eval_device(self._engine._h, self._scan._p, theta.data_ptr(), S, self.sign, dptr(weights),
                                                    dptr(out.get("chi2")), dptr(out.get("best")), dptr(out.get("best_k")),
                                                    dptr(out.get("s_best")), dptr(out.get("map")), self.K, dptr(colacc),
                                                    stream_of(theta.device)))
        return out

    def _host(self, theta, want, weights=None, colacc=None):
        theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
        if theta.ndim != 2 or theta.shape[1] != self.ndim:
            raise ValueError(f"theta must have {self.ndim} columns, got {theta.shape}")
        theta = np.ascontiguousarray(theta)
        S = theta.shape[0]
        out = {k: np.empty((S, self.K) if k == "map" else (S,), dtype=np.int32 if k == "best_k" else np.float64) for k in want}
        L.check(L.lib().cf_scan_eval(self._engine._h, self._scan._p, ptr(theta), S, self.sign, ptr(weights), ptr(out.get("chi2")),
                                     ptr(out.get("best")), ptr(out.get("best_k")), ptr(out.get("s_best")), ptr(out.get("map")),
                                     self.K, ptr(colacc)))
        return out

    def rows(self, theta) -> dict:
        """``dict(best, best_k, s_best, chi2)``, each [S] numpy, for host numbers theta [S, ndim] (or one row): the largest
        statistic over the live candidates, its candidate (ties: the smallest k; -1 with NaN for a row with a non-finite score),
        the signed score there and the engine's own chi^2."""
        return self._host(theta, ("best", "best_k", "s_best", "chi2"))

    def torch_rows(self, theta) -> dict:
        """``rows`` for a device-resident theta [S, ndim]: tensors out, asynchronous on torch's current stream."""
        return self._device(self._theta_tensor(theta), ("best", "best_k", "s_best", "chi2"))

    def map(self, theta):
        """The scores s_k [S, K] (numpy for host numbers, a tensor for a device tensor); dchi2_k = s_k^2 and
        alpha_hat_k = s_k / sqrt(F_k)."""
        import torch

        if isinstance(theta, torch.Tensor):
            return self._device(self._theta_tensor(theta), ("map",))["map"]
        return self._host(theta, ("map",))["map"]

    def alpha_hat(self, s):
        """(alpha_hat, error) of the candidates from their scores [.., K] (numpy): s / sqrt(F) and 1 / sqrt(F); NaN where dead."""
        with np.errstate(divide="ignore", invalid="ignore"):
            root = np.where(self.info["live"], np.sqrt(self.info["F"]), np.nan)
            return np.asarray(s) / root, 1.0 / root

    def report(self, flat_chain, weights=None) -> dict:
        """One pass over a chain [S, ndim] (a device tensor, or host numbers that are moved there): per candidate the posterior
        mean and scatter of s_k (``s_mean``, ``s_std``), the mean dchi2_k (``dchi2_mean``), ``alpha_hat`` and ``alpha_err`` at
        the posterior mean, the weighted fraction of samples in which k wins (``win_fraction``); per sample ``best``,
        ``best_k``, ``s_best`` and ``chi2`` on the device, and ``best_quantiles`` (5, 16, 50, 84, 95 %) of best."""
        import torch

        dev = torch.device("cuda", self.device)
        if not isinstance(flat_chain, torch.Tensor):
            flat_chain = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(flat_chain, dtype=np.float64)))).to(dev)
        th = self._theta_tensor(flat_chain)
        if th.shape[0] < 1:
            raise ValueError("report needs at least one sample")
        if weights is not None and not isinstance(weights, torch.Tensor):
            weights = torch.from_numpy(np.ascontiguousarray(np.asarray(weights, dtype=np.float64))).to(dev)
        if weights is not None and not bool((torch.isfinite(weights) & (weights >= 0)).all()):
            raise ValueError("weights must be finite and >= 0")
        acc = torch.zeros(2 * self.K + 1, dtype=torch.float64, device=th.device)
        out = self._device(th, ("best", "best_k", "s_best", "chi2"), weights=weights, colacc=acc)
        a = acc.cpu().numpy()
        sw = a[-1]
        s_mean, s2_mean = a[0:-1:2] / sw, a[1:-1:2] / sw
        k = out["best_k"].long()
        ok = k >= 0
        w = torch.ones_like(out["best"]) if weights is None else weights
        wins = torch.bincount(k[ok], weights=w[ok], minlength=self.K).cpu().numpy() / sw
        alpha, err = self.alpha_hat(s_mean)
        best_ok = out["best"][ok]
        q = torch.tensor([0.05, 0.16, 0.5, 0.84, 0.95], dtype=torch.float64, device=th.device)
        quant = torch.quantile(best_ok, q).cpu().numpy() if best_ok.numel() else np.full(5, np.nan)
        return dict(s_mean=s_mean, s_std=np.sqrt(np.maximum(s2_mean - s_mean * s_mean, 0.0)), dchi2_mean=s2_mean, alpha_hat=alpha,
                    alpha_err=err, win_fraction=wins, w_sum=float(sw), live=self.info["live"].copy(), table=self.table,
                    best_quantiles=quant, n_bad=int((~ok).sum().item()), **out)

    # ---- the null ------------------------------------------------------------------------------------------------------------
    def null(self, n_draws: int, seed: int = 0, row0: int = 0):
        """The best statistic of each of n_draws null draws [n_draws] on the device: the normals
        ``mocks.normals(null_key(seed), n_draws, n, k0=row0)`` pushed through ``L^T V`` by the same kernels.  Draw i depends on
        (seed, row0 + i) only, so a set can be drawn in pieces with the same bits."""
        import torch

        from . import mocks

        n_draws, row0 = int(n_draws), int(row0)
        if n_draws < 0 or row0 < 0:
            raise ValueError("null needs n_draws >= 0 and row0 >= 0")
        if self._null is None:
            self._null = Scan(null_matrix(self._chol, self.info["V"]), self.info["live"], device=self.device)
        dev = torch.device("cuda", self.device)
        key = null_key(seed)
        pieces = []
        for s0 in range(0, n_draws, _NULL_PIECE):
            m = min(_NULL_PIECE, n_draws - s0)
            xi = mocks.normals(key, m, self.n, k0=row0 + s0, device=dev)
            pieces.append(self._null.apply(xi, sign=self.sign, want=("best",))["best"])
        return torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.float64, device=dev)

    def significance(self, theta_or_chain, n_draws: int = 10000, seed: int = 0, level: float = 0.6827) -> dict:
        """The winner and its look-elsewhere-corrected significance.  One theta [ndim]: its own best candidate.  A chain
        [S, ndim]: the candidate whose posterior-mean score has the largest statistic (the scores are linear in the residuals, so
        this is the scan of the posterior-mean residual).  Returns ``global_p``'s dict plus ``best``, ``best_k``, ``s_best``,
        ``alpha_hat``, ``alpha_err`` and ``candidate`` (the winner's row of the table)."""
        import torch

        x = theta_or_chain
        single = (x.dim() if isinstance(x, torch.Tensor) else np.ndim(x)) == 1
        if single:
            x = x[None, :] if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)[None, :]
        rep = self.report(x)
        stat = np.where(self.info["live"], statistic(rep["s_mean"], self.sign), -1.0)
        k = int(np.argmax(stat))
        if not (stat[k] >= 0.0 and np.isfinite(stat[k])):
            raise ValueError("significance: no live candidate with a finite score")
        s = float(rep["s_mean"][k])
        out = global_p(float(stat[k]), self.null(n_draws, seed).cpu().numpy(), sign=self.sign, level=level)
        out.update(best=float(stat[k]), best_k=k, s_best=s, alpha_hat=float(rep["alpha_hat"][k]), alpha_err=float(rep["alpha_err"][k]),
                   candidate=self.table[k])
        return out
