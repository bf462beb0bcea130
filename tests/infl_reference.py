"""A long-double restatement of the attribution (include/cosmofit.h: cf_infl_device): g = C^-1 r by two triangular substitutions
with the Cholesky factor -- never through a precision matrix -- and from it the per-datum shares of chi^2, the leave-one-out
residuals, their z-scores and the per-sample table.  No engine code involved; numpy only."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
COLUMNS = ("chi2", "max_z", "max_z_index", "max_drop", "max_drop_index")
BAR = 1e-10  # the project's parity bar, on the scale of the terms summed


def solve_lower(L, B):
    """X with L X = B for the lower triangle of L [n, n] and B [n, m], row by row in long double."""
    L, X = np.asarray(L, dtype=LD), np.array(B, dtype=LD, ndmin=2)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_upper_t(L, B):
    """X with L^T X = B, from the last row up."""
    L, X = np.asarray(L, dtype=LD), np.array(B, dtype=LD, ndmin=2)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def g_rows(L, rows):
    """g [S, n] = C^-1 r for every row r of rows [S, n], C = L L^T: forward, then backward substitution."""
    return solve_upper_t(L, solve_lower(L, np.asarray(rows, dtype=LD).T)).T


def inverse_factor(L):
    """Linv [n, n] in long double (lower triangular)."""
    n = np.asarray(L).shape[0]
    return solve_lower(L, np.eye(n, dtype=LD))


def precision(L):
    """(K, bound): K = Linv^T Linv in long double and |Linv|^T |Linv|, the scale an entry's rounding is measured on."""
    X = inverse_factor(L)
    return X.T @ X, np.abs(X).T @ np.abs(X)


def g_rows_inv(inv_cov, rows):
    """g for a block whose precision matrix is given (BAO): r K with K symmetrised as the library does."""
    A = np.asarray(inv_cov, dtype=LD)
    return np.asarray(rows, dtype=LD) @ (LD(0.5) * (A + A.T))


def scale(K, rows):
    """sum_j |K_ij| |r_j| for every row: the scale of the terms of g_i."""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(rows, dtype=np.float64)) @ np.abs(np.asarray(K, dtype=np.float64))


def row_arrays(rows, g, kdiag):
    """(contrib, z, loo, drop), each [S, n] long double; a datum with K_ii = 0 is one the likelihood ignores: z, loo, drop 0."""
    rows, g, kd = np.asarray(rows, dtype=LD), np.asarray(g, dtype=LD), np.asarray(kdiag, dtype=LD)
    live = kd > 0
    safe = np.where(live, kd, LD(1))
    with np.errstate(invalid="ignore"):
        z = np.where(live[None, :], g / np.sqrt(safe)[None, :], LD(0))
        loo = np.where(live[None, :], g / safe[None, :], LD(0))
        drop = np.where(live[None, :], g * g / safe[None, :], LD(0))
        return rows * g, z, loo, drop


def sample_table(rows, g, kdiag):
    """[S, len(COLUMNS)] long double: chi2 = sum_i r_i g_i, max |z_i| and its index, max g_i^2 / K_ii and its index
    (np.argmax: the first NaN, else the first maximum)."""
    contrib, z, _, drop = row_arrays(rows, g, kdiag)
    out = np.empty((contrib.shape[0], len(COLUMNS)), dtype=LD)
    for s in range(contrib.shape[0]):
        kz, kd = int(np.argmax(np.abs(z[s]))), int(np.argmax(drop[s]))
        out[s] = (contrib[s].sum(), np.abs(z[s, kz]), kz, drop[s, kd], kd)
    return out


def top_two_gap(values):
    """(first, second) indices of the two largest of values [n] (the second is the first again when n = 1)."""
    order = np.argsort(-np.asarray(values, dtype=LD), kind="stable")
    return int(order[0]), int(order[min(1, order.size - 1)])


def deleted_problem(cov, r, i):
    """(e_i, chi2 without datum i) by brute force: the conditional mean of datum i given the others from the covariance with
    row and column i deleted, and the chi^2 of the remaining data under that covariance."""
    cov, r = np.asarray(cov, dtype=LD), np.asarray(r, dtype=LD)
    keep = np.arange(r.size) != i
    Ld = np.linalg.cholesky(np.asarray(cov[np.ix_(keep, keep)], dtype=np.float64))
    # refine the double factor's solve in long double: one step of iterative refinement on C_dd x = b
    Cdd = cov[np.ix_(keep, keep)]

    def solve(b):
        x = g_rows(Ld, b[None, :])[0]
        for _ in range(3):
            x = x + g_rows(Ld, (b - Cdd @ x)[None, :])[0]
        return x

    x = solve(r[keep])
    return r[i] - cov[i, keep] @ x, r[keep] @ x


def attribution(contrib_a, contrib_b, order):
    """(delta, cumulative in `order`, total) of two contrib vectors (or paired rows: the mean over the pairs)."""
    d = np.atleast_2d(np.asarray(contrib_a, dtype=LD) - np.asarray(contrib_b, dtype=LD))
    delta = d.mean(axis=0)
    return delta, np.cumsum(delta[np.asarray(order)]), d.sum(axis=1).mean()
