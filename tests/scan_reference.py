"""A long-double restatement of the template scan (include/cosmofit.h: cf_scan_eval_device), written from the definitions: for
every candidate a_k the generalised-least-squares fit of [A0, a_k] to a residual row under C = L L^T with the zero-mean Gaussian
priors, dchi2_k as the drop in the minimised chi^2 (prior penalties included) between the fit of the base alone and the fit of
base + a_k, and the score as the fitted amplitude of a_k over its error.  C^-1 is applied by two triangular substitutions with
the factor; V is never formed.  ``restate`` eliminates the base block of the joint normal equations once for all candidates;
``fit_one`` solves the joint system of one candidate as it stands and evaluates the chi^2 at the solution from the residual
vector, and is what ``restate`` is checked against.  No engine code involved; numpy (and, for the float64 shortlist of the
largest shape, scipy's LAPACK substitutions) only.  It is the judge of the CPU and GPU tests."""
import numpy as np

from cscale_reference import cholesky
from infl_reference import BAR, EPS, LD, solve_lower, solve_upper_t  # noqa: F401  (BAR and EPS are re-exported)

DEAD_REL = 1e-12  # the issue's rule: dead when a^T K' a <= 1e-12 a^T K a and no prior on the amplitude


def _precisions(sigma, m, dtype=LD):
    s = np.full(m, np.inf) if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (m,))
    proper = np.isfinite(s)
    return np.where(proper, dtype(1) / np.asarray(np.where(proper, s, 1.0), dtype=dtype) ** 2, dtype(0))


def _solvers(chol, dtype):
    if dtype is LD:
        Lo = np.tril(np.asarray(chol, dtype=LD))
        return lambda B: solve_upper_t(Lo, solve_lower(Lo, B)), cholesky, solve_lower
    from scipy.linalg import solve_triangular

    Lo = np.tril(np.asarray(chol, dtype=np.float64))
    return (lambda B: solve_triangular(Lo, solve_triangular(Lo, B, lower=True), lower=True, trans="T"), np.linalg.cholesky,
            lambda Lf, B: solve_triangular(Lf, B, lower=True))


def restate(chol, cand, rows, base=None, base_sigma=None, cand_sigma=None, dtype=LD):
    """dict for residual rows [S, n] and candidates [n, K]: s [S, K] (fitted amplitude over its error; 0 for a dead candidate),
    dchi2 [S, K], alpha_hat [S, K], alpha_err [K], F [K] (1 / alpha_err^2), live [K], chi2_0 [S] and chi2_base [S] (the chi^2
    minimised over the base alone).  dtype: long double (the judge) or float64 (a shortlist for a shape too large to judge in
    full)."""
    A = np.asarray(cand, dtype=dtype)
    A = A[:, None] if A.ndim == 1 else A
    R = np.atleast_2d(np.asarray(rows, dtype=dtype))
    n, K = A.shape
    solve_c, chol_small, solve_small = _solvers(chol, dtype)
    Pk = _precisions(cand_sigma, K, dtype)
    KR = solve_c(R.T)                                  # [n, S]
    KA = solve_c(A)                                    # [n, K]
    chi2_0 = (R.T * KR).sum(axis=0)
    gkk = (A * KA).sum(axis=0)
    num = A.T @ KR                                     # [K, S]: a_k^T C^-1 r
    d = gkk + Pk
    chi2_base = chi2_0
    if base is not None and np.size(base):
        A0 = np.asarray(base, dtype=dtype)
        A0 = A0[:, None] if A0.ndim == 1 else A0
        m0 = A0.shape[1]
        F0 = A0.T @ solve_c(A0) + np.diag(_precisions(base_sigma, m0, dtype))
        L0 = chol_small(dtype(0.5) * (F0 + F0.T))
        if L0 is None:
            raise ValueError("the base is rank deficient")
        u = solve_small(L0, A0.T @ KA)                 # [m0, K]
        t0 = solve_small(L0, A0.T @ KR)                # [m0, S]
        num = num - u.T @ t0
        d = d - (u * u).sum(axis=0)
        chi2_base = chi2_0 - (t0 * t0).sum(axis=0)
    live = ~((Pk == 0) & (d - Pk <= dtype(DEAD_REL) * gkk))
    safe = np.where(live, d, dtype(1))
    s = np.where(live[:, None], num / np.sqrt(safe)[:, None], dtype(0)).T
    return dict(s=s, dchi2=s * s, alpha_hat=np.where(live[:, None], num / safe[:, None], dtype(0)).T,
                alpha_err=np.where(live, 1 / np.sqrt(safe), np.inf), F=np.where(live, d, dtype(0)), live=live, chi2_0=chi2_0,
                chi2_base=chi2_base)


def fit_one(chol, a, rows, base=None, base_sigma=None, a_sigma=None):
    """(score [S], dchi2 [S], alpha_hat [S], alpha_err) of ONE candidate by brute force: the joint normal equations of [A0, a]
    solved as they stand, the chi^2 at the solution from the residual vector r - D alpha and the prior penalties, minus the
    same for the base alone."""
    Lo = np.tril(np.asarray(chol, dtype=LD))
    solve_c = lambda B: solve_upper_t(Lo, solve_lower(Lo, B))
    R = np.atleast_2d(np.asarray(rows, dtype=LD)).T    # [n, S]
    a = np.asarray(a, dtype=LD).reshape(-1, 1)
    A0 = np.zeros((a.shape[0], 0), dtype=LD) if base is None else np.asarray(base, dtype=LD).reshape(a.shape[0], -1)
    m0 = A0.shape[1]

    def minimum(D, P):
        if D.shape[1] == 0:
            return (R * solve_c(R)).sum(axis=0), None, None
        Fm = D.T @ solve_c(D) + np.diag(P)
        LF = cholesky(LD(0.5) * (Fm + Fm.T))
        alpha = solve_upper_t(LF, solve_lower(LF, D.T @ solve_c(R)))
        res = R - D @ alpha
        return (res * solve_c(res)).sum(axis=0) + (P[:, None] * alpha * alpha).sum(axis=0), alpha, LF

    P0 = _precisions(base_sigma, m0)
    chi2_base, _, _ = minimum(A0, P0)
    chi2_both, alpha, LF = minimum(np.concatenate([A0, a], axis=1), np.concatenate([P0, _precisions(a_sigma, 1)]))
    e = np.zeros((m0 + 1, 1), dtype=LD)
    e[-1] = 1
    err = np.sqrt(solve_upper_t(LF, solve_lower(LF, e))[-1, 0])
    return alpha[-1] / err, chi2_base - chi2_both, alpha[-1], err


def statistic(s, sign):
    """s^2, max(s, 0)^2 or max(-s, 0)^2."""
    s = np.asarray(s)
    u = s if sign == 0 else np.maximum(s, 0) if sign > 0 else np.maximum(-s, 0)
    return u * u


def best(s, live, sign):
    """(best [S], best_k [S], s_best [S], gap [S]) of scores [S, K] over the live candidates: np.argmax's first maximum; gap is
    the distance to the runner-up statistic (inf with one live candidate)."""
    stat = np.where(np.asarray(live)[None, :], statistic(s, sign), -1)
    k = np.argmax(stat, axis=1)
    rows = np.arange(stat.shape[0])
    top = stat[rows, k]
    rest = stat.copy()
    rest[rows, k] = -1
    second = rest.max(axis=1)
    gap = np.where(second >= 0, np.asarray(top - second, dtype=np.float64), np.inf)
    return top, k.astype(np.int64), np.asarray(s)[rows, k], gap


def scale(V, rows):
    """max_k sum_i |r_i| |V_ik| for every row [S]: the scale of the terms a score sums."""
    return (np.abs(np.atleast_2d(np.asarray(rows, dtype=np.float64))) @ np.abs(np.asarray(V, dtype=np.float64))).max(axis=1)
