"""High-precision reference of the solve stage: chi^2 = || L^-1 delta ||^2 by row-by-row forward substitution in np.longdouble
(x87 extended, 64-bit significand), rounded to float64 once at the end.  The residual rows delta come from the float64 numpy
oracle (oracle_np.sn_parts); log P is oracle_np.log_probability rebuilt from the long-double chi^2."""
import numpy as np

from oracle import oracle_np as onp

# a platform whose long double is a plain double would make this reference no better than the code under test
assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not extended precision on this platform"


def chi2_longdouble(chol, delta):
    """chol: lower factor [N, N] (the strict upper triangle is never read); delta [B, N] float64 -> chi^2 [B] float64."""
    L = np.asarray(chol, dtype=np.float64)
    n = L.shape[0]
    y = np.zeros((n, delta.shape[0]), dtype=np.longdouble)
    d = np.ascontiguousarray(np.asarray(delta, dtype=np.longdouble).T)
    for i in range(n):
        row = L[i, :i].astype(np.longdouble)
        y[i] = (d[i] - row @ y[:i]) / np.longdouble(L[i, i])
    return np.sum(y * y, axis=0).astype(np.float64)


def reference(lk, base):
    """dict(chi2, logp, chi2_f64) over the base rows: long-double chi^2, log P from it, and the float64 oracle's chi^2."""
    with np.errstate(all="ignore"):
        delta = np.array([onp.sn_parts(lk, t)[3] for t in base])
        chi2_f64 = np.array([onp.solve_triangular_chi2(lk.chol, row) for row in delta])
    chi2 = chi2_longdouble(lk.chol, delta)
    prior = np.array([onp.log_prior(lk, t) for t in base])
    with np.errstate(invalid="ignore"):
        logp = np.where(np.isinf(prior), -np.inf, prior + (-0.5 * chi2 + lk.logl_const))
    return dict(chi2=chi2, logp=logp, chi2_f64=chi2_f64)
