"""A long-double restatement of the closed-form treatment of linear SN nuisance parameters (include/cosmofit.h:
cf_marg_eval_device), written from the definitions: form C = L L^T, factor and solve with it, build F = A^T C^-1 A + P, take
alpha_hat = F^-1 (A^T C^-1 r + P mu), chi2_prof as the chi^2 AT alpha_hat with the prior penalty, ln L_marg from the Gaussian
integral and the conditional density N(alpha_hat, F^-1).  It never forms Wt.  No engine code involved; numpy only.  It is the
judge of the CPU and GPU tests."""
import numpy as np

from cscale_reference import cholesky
from infl_reference import BAR, EPS, LD, solve_lower, solve_upper_t  # noqa: F401  (BAR and EPS are re-exported)

LN_2PI = np.log(LD(2) * LD(np.pi))
_FACTORS = {}


def covariance_factor(chol):
    """The long-double factor of C = L L^T formed from the double factor `chol` (cached per factor: the tests share few)."""
    key = (chol.shape[0], float(chol[-1, -1]), float(chol[0, 0]), float(np.abs(chol).sum()))
    if key not in _FACTORS:
        Lo = np.tril(np.asarray(chol, dtype=LD))
        _FACTORS[key] = cholesky(Lo @ Lo.T)
    return _FACTORS[key]


def solve_c(Lc, B):
    """C^-1 B for B [n, k]."""
    return solve_upper_t(Lc, solve_lower(Lc, B))


def prior_arrays(m, mu=None, sigma=None, box=None):
    """(mu [m], P [m], proper [m] bool, lo [m], hi [m]) in long double; lo / hi NaN where no box."""
    mu = np.zeros(m) if mu is None else np.asarray(mu, dtype=np.float64)
    sigma = np.full(m, np.inf) if sigma is None else np.asarray(sigma, dtype=np.float64)
    proper = np.isfinite(sigma)
    P = np.where(proper, LD(1) / np.asarray(np.where(proper, sigma, 1.0), dtype=LD) ** 2, LD(0))
    lo, hi = np.full(m, np.nan), np.full(m, np.nan)
    for j, b in enumerate(box or ()):
        if b is not None:
            lo[j], hi[j] = b
    return np.asarray(np.where(proper, mu, 0.0), dtype=LD), P, proper, lo, hi


def restate(chol, A, rows, mu=None, sigma=None, box=None):
    """dict for residual rows [S, n]: alpha_hat [S, m], t [S, m] (= L_F^-1 (A^T C^-1 r + P mu)), q [S], chi2_0 [S] (r^T C^-1 r),
    chi2_prof [S] (the chi^2 at alpha_hat plus the prior penalty, evaluated directly), dlogl [S] (ln L_marg - ln L_engine),
    log_norm, pmu, F, LF [m, m] and Finv (the conditional covariance), all long double."""
    A = np.asarray(A, dtype=LD)
    A = A[:, None] if A.ndim == 1 else A
    m = A.shape[1]
    rows = np.atleast_2d(np.asarray(rows, dtype=LD))
    Lc = covariance_factor(np.asarray(chol, dtype=np.float64))
    mu, P, proper, lo, hi = prior_arrays(m, mu, sigma, box)
    K = solve_c(Lc, A)
    F = A.T @ K + np.diag(P)
    F = LD(0.5) * (F + F.T)
    LF = cholesky(F)
    if LF is None:
        return None
    G = solve_c(Lc, rows.T)                           # [n, S] = C^-1 r
    b = A.T @ G + (P * mu)[:, None]                   # [m, S]
    t = solve_lower(LF, b)
    alpha = solve_upper_t(LF, t)                      # [m, S]
    chi2_0 = (rows.T * G).sum(axis=0)
    res = rows.T - A @ alpha                          # [n, S]
    pen = (P[:, None] * (alpha - mu[:, None]) ** 2).sum(axis=0)
    chi2_prof = (res * solve_c(Lc, res)).sum(axis=0) + pen
    boxed = ~proper & np.isfinite(lo)
    m_flat = int((~proper).sum())
    sig = np.asarray(np.asarray(sigma, dtype=np.float64)[proper], dtype=LD) if proper.any() else np.zeros(0, dtype=LD)
    log_norm = (-np.log(np.diag(LF)).sum() + LD(0.5) * m_flat * LN_2PI - np.log(sig).sum()
                - np.log(np.asarray(hi[boxed] - lo[boxed], dtype=LD)).sum())
    Finv = solve_upper_t(LF, solve_lower(LF, np.eye(m, dtype=LD)))
    return dict(alpha_hat=alpha.T, t=t.T, q=(t * t).sum(axis=0), chi2_0=chi2_0, chi2_prof=chi2_prof,
                dlogl=LD(-0.5) * (chi2_prof - chi2_0) + log_norm, log_norm=log_norm, pmu=(P * mu) @ mu, F=F, LF=LF, Finv=Finv)


def conditional_logpdf(ref, alpha, row_alpha_hat):
    """ln N(alpha; alpha_hat, F^-1) for alpha [S, m] in long double."""
    d = np.asarray(alpha, dtype=LD) - np.asarray(row_alpha_hat, dtype=LD)
    z = d @ ref["LF"]                                 # (L_F^T d)^T
    m = d.shape[1]
    return LD(-0.5) * (z * z).sum(axis=1) + np.log(np.diag(ref["LF"])).sum() - LD(0.5) * m * LN_2PI


def scales(proj, rows, chi2_engine, xi=None):
    """The scales the bar applies to, from the terms summed: for t, sum_i |r_i| |Wt_ij| + |ct_j| [S, m]; for values,
    chi2_engine + pmu + sum_j (that)^2 [S]; for alpha, |U^-1| applied to the scale of t (plus |xi|) [S, m]."""
    a = np.abs(np.atleast_2d(rows)) @ np.abs(proj["Wt"]) + np.abs(proj["ct"])[None, :]
    val = np.abs(np.asarray(chi2_engine, dtype=np.float64)) + proj["pmu"] + (a * a).sum(axis=1)
    Ui = np.abs(np.linalg.inv(np.triu(proj["U"])))
    return a, val, (a + (0.0 if xi is None else np.abs(xi))) @ Ui.T


def from_projection(proj, rows, xi=None):
    """(t, q, alpha) in long double from a projection's own arrays: what the device computes, without its rounding."""
    t = np.asarray(rows, dtype=LD) @ np.asarray(proj["Wt"], dtype=LD) + np.asarray(proj["ct"], dtype=LD)
    v = t if xi is None else t + np.asarray(xi, dtype=LD)
    U = np.triu(np.asarray(proj["U"], dtype=LD))
    alpha = solve_upper_t(U.T, v.T).T
    return t, (t * t).sum(axis=1), alpha
