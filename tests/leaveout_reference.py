"""A long-double restatement of the leave-group-out quantities (include/cosmofit.h: cf_group_*, cf_reweight_device): the Cholesky
factor of K_BB and its inverse, q_B and e_B from g, the brute-force deleted problem they must equal, the record of the importance
summary in plain sums, and the closed forms the reweighting is checked against.  No engine code involved; numpy only."""
import numpy as np

import infl_reference as IR

LD = np.longdouble
EPS = IR.EPS
BAR = IR.BAR  # the project's parity bar, on the scale of the terms summed
RW_SLOTS = ("lmax", "sum_w", "sum_w2", "max_w", "n_used", "n_skipped", "sum_w0", "sum_w0_sq")
RW_MEAN = 8


_SPLIT = LD(2**32 + 1)  # Dekker's splitter for a 64-bit significand


def _two_prod(a, b):
    """(p, e) with a * b = p + e exactly (Dekker), elementwise in long double."""
    p = a * b
    ta, tb = _SPLIT * a, _SPLIT * b
    ah, bh = ta - (ta - a), tb - (tb - b)
    al, bl = a - ah, b - bh
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def dot2(a, b):
    """sum_k a_k b_k as if in twice the working precision, rounded once (Ogita, Rump & Oishi's Dot2): exact products, the
    rounding of every addition collected (Knuth's TwoSum).  Without it a long-double factor of an ill-conditioned K_BB is itself
    several double eps from the true one and cannot referee a compensated computation."""
    p, e = _two_prod(np.asarray(a, dtype=LD), np.asarray(b, dtype=LD))
    s, c = LD(0), e.sum(dtype=LD)
    for t in p:
        n = s + t
        z = n - s
        c += (s - (n - z)) + (t - z)
        s = n
    return s + c


def cholesky(A):
    """The lower Cholesky factor of A [m, m] (its lower triangle is read) in long double with doubled-precision dot products."""
    A = np.asarray(A, dtype=LD)
    m = A.shape[0]
    Lf = np.zeros((m, m), dtype=LD)
    for i in range(m):
        for j in range(i):
            Lf[i, j] = (A[i, j] - dot2(Lf[i, :j], Lf[j, :j])) / Lf[j, j]
        Lf[i, i] = np.sqrt(A[i, i] - dot2(Lf[i, :i], Lf[i, :i]))
    return Lf


def invert_lower(Lf):
    """X = Lf^-1 (lower triangular) in long double with doubled-precision dot products, column by column."""
    m = Lf.shape[0]
    X = np.zeros((m, m), dtype=LD)
    for j in range(m):
        X[j, j] = LD(1) / Lf[j, j]
        for i in range(j + 1, m):
            X[i, j] = -dot2(Lf[i, j:i], X[j:i, j]) / Lf[i, i]
    return X


def sub_matrix(K, idx):
    """K_BB from the LOWER triangle of K, in the order of idx."""
    idx = np.asarray(idx, dtype=np.int64)
    hi, lo = np.maximum.outer(idx, idx), np.minimum.outer(idx, idx)
    return np.asarray(K)[hi, lo]


def inverse_factor(K, idx):
    """(X, bound): X_B = L_B^-1 of K_BB = L_B L_B^T in long double, and |X| |L| |X|, the scale an entry's error is measured on
    (the componentwise perturbation bound of a triangular inverse; >= |X_ij|)."""
    Lf = cholesky(sub_matrix(K, idx))
    X = invert_lower(Lf)
    return X, np.abs(X) @ np.abs(Lf) @ np.abs(X)


def group_q(K, g, idx):
    """(q [S], scale [S], e [S, m]) for rows g [S, n]: y = X_B g_B, q = sum_j y_j^2, scale = sum_j (sum_k |X_jk| |g_k|)^2 (the
    terms summed), e_B = X_B^T y = K_BB^-1 g_B."""
    X, _ = inverse_factor(K, idx)
    gb = np.asarray(g, dtype=LD)[:, np.asarray(idx, dtype=np.int64)]
    y = gb @ X.T
    return (y * y).sum(axis=1), ((np.abs(gb) @ np.abs(X).T)**2).sum(axis=1), y @ X


def deleted_group(cov, r, idx):
    """(e_B [m], chi^2 without B) by brute force: the group minus its conditional mean given the others, from the covariance
    with the group's rows and columns deleted, and the chi^2 of the remaining data under that covariance (a double Cholesky
    factor refined in long double, as ``infl_reference.deleted_problem``)."""
    cov, r = np.asarray(cov, dtype=LD), np.asarray(r, dtype=LD)
    idx = np.asarray(idx, dtype=np.int64)
    keep = np.ones(r.size, dtype=bool)
    keep[idx] = False
    Caa = cov[np.ix_(keep, keep)]
    La = np.linalg.cholesky(np.asarray(Caa, dtype=np.float64))

    def solve(b):
        x = IR.g_rows(La, b[None, :])[0]
        for _ in range(3):
            x = x + IR.g_rows(La, (b - Caa @ x)[None, :])[0]
        return x

    x = solve(r[keep])
    return r[idx] - cov[np.ix_(idx, keep)] @ x, r[keep] @ x


# ---- the importance summary -----------------------------------------------------------------------------------------------------
def reweight_record(lw, w0, x, pivot):
    """(record [G, 8 + ncol + ncol (ncol + 1) / 2], scale of the same shape) in long double: the record of cf_reweight_device in
    plain sums, and for every summed slot the sum of the absolute values of its terms (0 for the exact slots)."""
    lw, x = np.asarray(lw, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if lw.ndim == 1:
        lw = lw[:, None]
    S, G = lw.shape
    ncol = x.shape[1]
    w0 = np.ones(S) if w0 is None else np.asarray(w0, dtype=np.float64)
    row_ok = np.isfinite(x).all(axis=1) & np.isfinite(w0) & (w0 >= 0)
    iu = np.triu_indices(ncol)
    rec = np.zeros((G, RW_MEAN + ncol + iu[0].size), dtype=LD)
    scale = np.zeros_like(rec)
    d = np.where(row_ok[:, None], x, 0.0).astype(LD) - np.asarray(pivot, dtype=LD)[None, :]
    for b in range(G):
        used = row_ok & ~np.isnan(lw[:, b]) & (lw[:, b] != np.inf)
        top = used & (w0 > 0)                      # a row of base weight 0 weighs 0 whatever its lw: it does not set the scale
        lmax = lw[top, b].max() if top.any() else -np.inf
        with np.errstate(invalid="ignore"):
            e = np.where(top & (lw[:, b] > -np.inf), np.exp(np.where(top, lw[:, b], -np.inf).astype(LD) - LD(lmax if np.isfinite(lmax) else 0.0)), LD(0))
        w = np.where(used, w0.astype(LD) * e, LD(0))
        wb = np.where(used, w0, 0.0).astype(LD)
        m1 = w[:, None] * np.where(used[:, None], d, LD(0))
        m2 = m1[:, iu[0]] * np.where(used[:, None], d, LD(0))[:, iu[1]]
        rec[b, :RW_MEAN] = (lmax, w.sum(), (w * w).sum(), w.max(), used.sum(), (~used).sum(), wb.sum(), (wb * wb).sum())
        rec[b, RW_MEAN:RW_MEAN + ncol] = m1.sum(axis=0)
        rec[b, RW_MEAN + ncol:] = m2.sum(axis=0)
        scale[b, :RW_MEAN] = (0, w.sum(), (w * w).sum(), 0, 0, 0, wb.sum(), (wb * wb).sum())
        scale[b, RW_MEAN:RW_MEAN + ncol] = np.abs(m1).sum(axis=0)
        scale[b, RW_MEAN + ncol:] = np.abs(m2).sum(axis=0)
    return rec, scale


def gaussian_inverse_ess_fraction(d, s2):
    """1 / ESS_fraction of reweighting N(0, 1) draws to N(d, s2), s2 < 2: E[w^2] / E[w]^2 =
    (1 / s2) (2 / s2 - 1)^(-1/2) exp((2 d / s2)^2 / (2 (2 / s2 - 1)) - d^2 / s2)."""
    a = 2.0 / s2 - 1.0
    return (1.0 / s2) * a**-0.5 * np.exp((2.0 * d / s2)**2 / (2.0 * a) - d * d / s2)


def gaussian_log_weight(x, d, s2):
    """ln of N(d, s2) / N(0, 1) at x."""
    return -0.5 * (x - d)**2 / s2 + 0.5 * x**2 - 0.5 * np.log(s2)
