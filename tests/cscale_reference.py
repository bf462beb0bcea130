"""A long-double restatement of the scaled covariance (include/cosmofit.h: cf_cscale_eval_device), written from the definitions:
form C(s) = C0 + s C1 with C0 = L0 L0^T, factor it, substitute, and take the log-determinant difference.  No eigenvalues, no T,
no engine code involved; numpy only.  It is the judge of the GPU tests.

At the Pantheon+ size (n = 1701) numpy's long-double products make one call of ``quad_logdet`` take half a minute, too long for
a test, so its result for that one case is recorded in tests/golden/cscale_pantheon_ref.npz: run this file on a machine with an
MI355X (``python tests/cscale_reference.py``; the residual rows are the engine's own) to record it again."""
import os

import numpy as np

from infl_reference import BAR, EPS, LD, solve_lower  # noqa: F401  (BAR and EPS are re-exported)


def cholesky(A):
    """The lower Cholesky factor of A [n, n] in long double, column by column; None when A is not positive definite."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    Lf = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - Lf[j, :j] @ Lf[j, :j]
        if not d > 0:
            return None
        Lf[j, j] = np.sqrt(d)
        Lf[j + 1:, j] = (A[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def c1_matrix(C1, n):
    c = np.asarray(C1, dtype=LD)
    if c.ndim == 0:
        return c * np.eye(n, dtype=LD)
    return np.diag(c) if c.ndim == 1 else c


def quad_logdet(chol0, C1, rows, s_values):
    """(quad [S, m], logdet [m]) in long double for residual rows [S, n] and m amplitudes: quad = r^T C(s)^-1 r by one
    substitution with the factor of C(s), logdet = ln|C(s)| - ln|C0| from the two diagonals.  NaN where C(s) is not positive
    definite."""
    L0 = np.tril(np.asarray(chol0, dtype=LD))
    n = L0.shape[0]
    C0, c1 = L0 @ L0.T, c1_matrix(C1, n)
    rows = np.atleast_2d(np.asarray(rows, dtype=LD))
    ld0 = 2 * np.log(np.diag(cholesky(C0))).sum()  # of the same C0 the sums below start from: the difference at s = 0 is exactly 0
    quad = np.full((rows.shape[0], len(s_values)), np.nan, dtype=LD)
    logdet = np.full(len(s_values), np.nan, dtype=LD)
    for j, s in enumerate(s_values):
        Ls = cholesky(C0 + LD(s) * c1)
        if Ls is None:
            continue
        z = solve_lower(Ls, rows.T)
        quad[:, j] = (z * z).sum(axis=0)
        logdet[j] = 2 * np.log(np.diag(Ls)).sum() - ld0
    return quad, logdet


def scales(T, lam, rows, s_values):
    """The scales the bar applies to: for quad, sum_k w_k (sum_i |T_ki| |r_i|)^2 with w_k = 1 / (1 + s lam_k), [S, m]; for
    logdet, sum_k |log1p(s lam_k)|, [m]."""
    a = np.abs(np.atleast_2d(rows)) @ np.abs(T).T  # [S, n]
    s = np.asarray(s_values, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = 1.0 / (1.0 + s[:, None] * lam[None, :])  # [m, n]
        return (a * a) @ w.T, np.abs(np.log1p(s[:, None] * lam[None, :])).sum(axis=1)


# ---- the recorded Pantheon+-sized case (tests/test_gpu_cscale.py) ---------------------------------------------------------------
PANTHEON_FIXTURE = "cscale_pantheon_ref"
PANTHEON_P = 0.12  # the extra low-z scatter in magnitudes: s = p^2


def pantheon_case(pkg, n, S):
    """(likelihood, synthetic data, C1 = the 0/1 diagonal of z <= 0.2, theta [S, 4]) of the recorded case."""
    import resid_shapes as RS

    lk, syn = RS.sn_likelihood(pkg, n)
    return lk, syn, (syn["z_cmb"] <= 0.2).astype(np.float64), RS.sn_thetas(pkg, S)


def split(x):
    """A long-double array as two doubles (hi, lo) whose sum is x to 2^-105: what an .npz can carry on every platform."""
    hi = np.asarray(x, dtype=np.float64)
    return hi, np.asarray(np.asarray(x, dtype=LD) - hi, dtype=np.float64)


def record_pantheon(out_path=None):
    import cscale_shapes as CS
    from conftest import GOLDEN, load_pkg

    pkg = load_pkg()
    lk, syn, c1, theta = pantheon_case(pkg, CS.N_PANTHEON, CS.S_PANTHEON)
    parts = lk.engine.parts(theta)
    quad, logdet = quad_logdet(syn["chol"], c1, parts["delta"], [PANTHEON_P ** 2])
    q_hi, q_lo = split(quad[:, 0])
    l_hi, l_lo = split(logdet)
    out_path = out_path or os.path.join(GOLDEN, PANTHEON_FIXTURE + ".npz")
    np.savez(out_path, theta=theta, p=PANTHEON_P, chi2_sn0=parts["chi2_blocks"][:, 0], quad_hi=q_hi, quad_lo=q_lo, logdet_hi=l_hi,
             logdet_lo=l_lo)
    lk.engine.close()
    print("recorded", out_path)


if __name__ == "__main__":
    import sys

    record_pantheon(sys.argv[1] if len(sys.argv) > 1 else None)
