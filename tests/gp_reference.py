"""
Long-double numpy restatement of the Gaussian-process formulas of include/cosmofit.h (cf_gp_*), written from the model of
ohd/cc_gp.py:14-41 and ohd/gp_lib.py:55-68, not from csrc/cosmofit_gp.hip: the judge of the GP tests (gpytorch is not
available, so the reference script itself cannot run).

    K_ij = s_f^2 exp(-(z_i - z_j)^2 / (2 l^2)) + s C_ij,   r = y - m,   K = L L^T
    log ML = -1/2 r^T K^-1 r - sum log L_ii - n/2 log 2 pi
    alpha = K^-1 r,  v = L^-1 k*,  u = L^-1 dk*
    mean = m + k*^T alpha,  var = s_f^2 - v.v + s noise,  dmean = dk*^T alpha,  dvar = s_f^2 / l^2 - u.u,  cov = -v.u
"""
import numpy as np

LD = np.longdouble
LOG_2PI = np.log(2 * np.arccos(LD(-1)))  # pi to the long double's own precision


def kernel_matrix(z, C, theta):
    m, sf2, ell, s = (LD(t) for t in theta)
    z = np.asarray(z, dtype=LD)
    dz = z[:, None] - z[None, :]
    return sf2 * np.exp(-(dz * dz) / (2 * ell * ell)) + s * np.asarray(C, dtype=LD)


def cholesky(K):
    """Lower factor, column by column, in long double; raises np.linalg.LinAlgError on a pivot <= 0 or non-finite."""
    K = np.array(K, dtype=LD)
    n = K.shape[0]
    Lw = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = K[j, j] - np.dot(Lw[j, :j], Lw[j, :j])
        if not (d > 0 and np.isfinite(d)):
            raise np.linalg.LinAlgError(f"pivot {j} = {d}")
        Lw[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lw[j + 1:, j] = (K[j + 1:, j] - Lw[j + 1:, :j] @ Lw[j, :j]) / Lw[j, j]
    return Lw


def forward(Lw, b):
    """L^-1 b for b [n] or [n, k]."""
    x = np.array(b, dtype=LD)
    n = Lw.shape[0]
    for i in range(n):
        x[i] = (x[i] - Lw[i, :i] @ x[:i]) / Lw[i, i]
    return x


def backward(Lw, b):
    """L^-T b."""
    x = np.array(b, dtype=LD)
    n = Lw.shape[0]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - Lw[i + 1:, i] @ x[i + 1:]) / Lw[i, i]
    return x


def mll_parts(z, y, C, theta):
    """(log ML, r^T K^-1 r, log|K|) in long double."""
    n = len(z)
    Lw = cholesky(kernel_matrix(z, C, theta))
    w = forward(Lw, np.asarray(y, dtype=LD) - LD(theta[0]))
    quad = np.dot(w, w)
    logdet = 2 * np.sum(np.log(np.diag(Lw)))
    return -quad / 2 - logdet / 2 - n * LOG_2PI / 2, quad, logdet


def mll(z, y, C, theta):
    return mll_parts(z, y, C, theta)[0]


def predict(z, y, C, theta, z_star, noise=0.0):
    """[nz, 5] long double: mean, var, dmean, dvar, cov(value, derivative)."""
    m, sf2, ell, s = (LD(t) for t in theta)
    z = np.asarray(z, dtype=LD)
    zs = np.asarray(z_star, dtype=LD)
    Lw = cholesky(kernel_matrix(z, C, theta))
    alpha = backward(Lw, forward(Lw, np.asarray(y, dtype=LD) - m))
    dz = z[:, None] - zs[None, :]                     # [n, nz]
    ks = sf2 * np.exp(-(dz * dz) / (2 * ell * ell))   # k(z_i, z*)
    dks = ks * dz / (ell * ell)                       # d/dz* of it
    v, u = forward(Lw, ks), forward(Lw, dks)
    out = np.empty((zs.size, 5), dtype=LD)
    out[:, 0] = m + ks.T @ alpha
    out[:, 1] = sf2 - np.sum(v * v, axis=0) + s * LD(noise)
    out[:, 2] = dks.T @ alpha
    out[:, 3] = sf2 / (ell * ell) - np.sum(u * u, axis=0)
    out[:, 4] = -np.sum(v * u, axis=0)
    return out


def predict_scales(theta, ref):
    """The scale each of the five predictive columns is judged against (ISSUE 'Bars'): max |mean| over the test points,
    s_f^2, max |dmean|, s_f^2 / l^2, s_f^2 / l.  ref: [nz, 5]."""
    _, sf2, ell, _ = (LD(t) for t in theta)
    return np.array([np.max(np.abs(ref[:, 0])), sf2, np.max(np.abs(ref[:, 2])), sf2 / (ell * ell), sf2 / ell], dtype=LD)


def scaled_errors(got, ref, theta):
    """[5]: max over the test points of |got - ref| / scale, per column.  A column whose scale is 0 (dmean at n = 1 with
    k* flat is never exactly 0, but guard it) is judged absolutely."""
    sc = predict_scales(theta, ref)
    sc = np.where(sc > 0, sc, LD(1))
    return np.max(np.abs(np.asarray(got, dtype=LD) - ref), axis=0) / sc


def mixture(preds, weights=None):
    """Mixture moments of S Gaussians: preds [S, nz, 5] -> [nz, 5] (mean, var, dmean, dvar, cov) with
    mean = E[mean_s], var = E[var_s + mean_s^2] - mean^2, cov = E[cov_s + mean_s dmean_s] - mean dmean."""
    p = np.asarray(preds, dtype=LD)
    S = p.shape[0]
    w = np.full(S, LD(1) / S, dtype=LD) if weights is None else np.asarray(weights, dtype=LD) / np.sum(np.asarray(weights, dtype=LD))
    E = lambda a: np.tensordot(w, a, axes=(0, 0))
    mean, dmean = E(p[:, :, 0]), E(p[:, :, 2])
    out = np.empty(p.shape[1:], dtype=LD)
    out[:, 0] = mean
    out[:, 1] = E(p[:, :, 1] + p[:, :, 0] ** 2) - mean**2
    out[:, 2] = dmean
    out[:, 3] = E(p[:, :, 3] + p[:, :, 2] ** 2) - dmean**2
    out[:, 4] = E(p[:, :, 4] + p[:, :, 0] * p[:, :, 2]) - mean * dmean
    return out


# ---- float64 scipy path: what the restatement is itself checked against ------------------------------------------------
def scipy_mll_parts(z, y, C, theta):
    from scipy.linalg import cho_factor, cho_solve

    m, sf2, ell, s = (float(t) for t in theta)
    z = np.asarray(z, dtype=np.float64)
    dz = z[:, None] - z[None, :]
    K = sf2 * np.exp(-(dz * dz) / (2 * ell * ell)) + s * np.asarray(C, dtype=np.float64)
    cf = cho_factor(K, lower=True)
    r = np.asarray(y, dtype=np.float64) - m
    quad = float(r @ cho_solve(cf, r))
    logdet = 2.0 * float(np.sum(np.log(np.diag(cf[0]))))
    return -0.5 * quad - 0.5 * logdet - 0.5 * len(z) * np.log(2 * np.pi), quad, logdet


def scipy_predict(z, y, C, theta, z_star, noise=0.0):
    from scipy.linalg import cho_factor, cho_solve, solve_triangular

    m, sf2, ell, s = (float(t) for t in theta)
    z = np.asarray(z, dtype=np.float64)
    zs = np.asarray(z_star, dtype=np.float64)
    dz = z[:, None] - z[None, :]
    K = sf2 * np.exp(-(dz * dz) / (2 * ell * ell)) + s * np.asarray(C, dtype=np.float64)
    cf = cho_factor(K, lower=True)
    Lw = np.tril(cf[0])
    alpha = cho_solve(cf, np.asarray(y, dtype=np.float64) - m)
    d = z[:, None] - zs[None, :]
    ks = sf2 * np.exp(-(d * d) / (2 * ell * ell))
    dks = ks * d / (ell * ell)
    v, u = solve_triangular(Lw, ks, lower=True), solve_triangular(Lw, dks, lower=True)
    return np.stack([m + ks.T @ alpha, sf2 - np.sum(v * v, 0) + s * noise, dks.T @ alpha, sf2 / ell**2 - np.sum(u * u, 0),
                     -np.sum(v * u, 0)], axis=1)
