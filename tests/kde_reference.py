"""The judge of the tension module: scipy.stats.gaussian_kde's definitions and the parameter-shift estimator restated in numpy
long double, term by term, with no tiling and no tricks.

* ``kernel_sums``: what cf_kde_sum_device promises, out[i] = sum_{j != self(i)} w_j exp(-|q_i - y_j|^2 / 2) and the sum of the
  squared terms, in long double.
* ``setup`` / ``density``: scipy's gaussian_kde (weights normalised to sum 1, neff = 1 / sum w^2, Scott / Silverman factors from
  neff, covariance np.cov(aweights=w, bias=False) * factor^2, points whitened with the Cholesky factor, normalised by
  (2 pi)^{d/2} sqrt(det)); a float is a factor, a d x d matrix is the kernel covariance itself.  ``leave_one_out`` drops the
  row's own term and normalises by the weight that is left.
* ``shift``: p_exceed = sum w_i [p_{-i}(Delta_i) > p(at)] / sum w_i and the rest of what tension.kde_shift returns.
* ``scipy_kde``: the scipy object for the same arguments, matrix bandwidth included.

Every function computes in ``dtype``, long double unless told otherwise; the estimator-sanity test of
tests/test_tension_cpu.py passes float64, where a statistical scatter of 1e-2 is the subject and not the arithmetic.
"""
import math

import numpy as np

LD = np.longdouble


def factor_of(bandwidth, neff, d, dtype=LD):
    T = dtype
    if isinstance(bandwidth, str):
        if bandwidth == "scott":
            return T(neff) ** (T(-1.0) / T(d + 4))
        if bandwidth == "silverman":
            return (T(neff) * T(d + 2) / T(4.0)) ** (T(-1.0) / T(d + 4))
        raise ValueError(bandwidth)
    return T(float(bandwidth))


def setup(samples, weights=None, bandwidth="silverman", dtype=LD):
    """dict(w [n] summing to 1, neff, mean [d], cov [d, d] the kernel covariance, chol, norm = (2 pi)^{d/2} sqrt(det)), LD."""
    T = dtype
    x = np.asarray(samples, dtype=T)
    n, d = x.shape
    w = np.full(n, T(1.0)) if weights is None else np.asarray(weights, dtype=T)
    w = w / w.sum()
    neff = T(1.0) / (w * w).sum()
    mean = (w[:, None] * x).sum(axis=0)
    if isinstance(bandwidth, np.ndarray):
        cov = np.asarray(bandwidth, dtype=T).reshape(d, d)
    else:
        xc = x - mean
        data_cov = (xc * w[:, None]).T @ xc / (T(1.0) - (w * w).sum())
        cov = data_cov * factor_of(bandwidth, neff, d, T) ** 2
    chol = cholesky(cov, T)
    norm = (T(2.0) * T(np.pi)) ** (T(d) / 2) * np.prod(np.diag(chol))
    return dict(w=w, neff=neff, mean=mean, cov=cov, chol=chol, norm=norm)


def cholesky(a, dtype=LD):
    """Lower Cholesky factor in long double (numpy.linalg has no extended type)."""
    T = dtype
    a = np.asarray(a, dtype=T)
    d = a.shape[0]
    L = np.zeros((d, d), dtype=T)
    for i in range(d):
        for j in range(i + 1):
            s = a[i, j] - (L[i, :j] * L[j, :j]).sum()
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L


def whiten(points, mean, chol, dtype=LD):
    """z with chol z = (x - mean) for every row: forward substitution in long double."""
    T = dtype
    xc = np.asarray(points, dtype=T) - mean
    d = chol.shape[0]
    z = np.zeros_like(xc)
    for i in range(d):
        z[:, i] = (xc[:, i] - z[:, :i] @ chol[i, :i]) / chol[i, i]
    return z


def kernel_sums(y, w, q, self_offset=-1, dtype=LD):
    """(out [m], sq [m]) in long double; query i is sample self_offset + i when self_offset >= 0 and that term is left out."""
    T = dtype
    y, q = np.asarray(y, dtype=T), np.asarray(q, dtype=T)
    n, d = y.shape
    m = q.shape[0]
    w = np.full(n, T(1.0)) if w is None else np.asarray(w, dtype=T)
    r2 = np.zeros((m, n), dtype=T)
    for c in range(d):
        df = q[:, c][:, None] - y[:, c][None, :]
        r2 += df * df
    t = w[None, :] * np.exp(T(-0.5) * r2)
    if self_offset >= 0:
        t[np.arange(m), self_offset + np.arange(m)] = 0
    return t.sum(axis=1), (t * t).sum(axis=1)


def density(samples, at, weights=None, bandwidth="silverman", leave_one_out=False, dtype=LD):
    """gaussian_kde(samples.T, bandwidth, weights)(at.T) in long double; with leave_one_out `at` is `samples` and row i leaves
    sample i out, normalised by 1 - w_i."""
    T = dtype
    s = setup(samples, weights, bandwidth, T)
    y = whiten(samples, s["mean"], s["chol"], T)
    if leave_one_out:
        out, _ = kernel_sums(y, s["w"], y, 0, T)
        return out / (s["norm"] * (T(1.0) - s["w"]))
    out, _ = kernel_sums(y, s["w"], whiten(at, s["mean"], s["chol"], T), -1, T)
    return out / s["norm"]


def sigma_of(p):
    """sqrt(2) erfinv(p): the two-sided normal quantile of a probability."""
    from scipy import special

    return float(math.sqrt(2.0) * special.erfinv(float(p)))


def shift(diff, weights=None, bandwidth="silverman", at=None, leave_one_out=True, dtype=LD):
    """The parameter-shift estimate in long double.  Returns a dict: p_exceed, count (rows above, an int), n_sigma, saturated,
    p_zero, p_zero_se, n_eff, densities [n] (p_{-i}(Delta_i)), ratio [n] = densities / p_zero."""
    T = dtype
    x = np.asarray(diff, dtype=T)
    n, d = x.shape
    s = setup(x, weights, bandwidth, T)
    w = s["w"]
    y = whiten(x, s["mean"], s["chol"], T)
    q0 = whiten(np.zeros((1, d)) if at is None else np.asarray(at, dtype=T).reshape(1, d), s["mean"], s["chol"], T)
    k0, k0sq = kernel_sums(y, w, q0, -1, T)
    p_zero = k0[0] / s["norm"]  # w sums to 1
    sw2 = (w * w).sum()
    var = (k0sq[0] - k0[0] ** 2 * sw2)  # / (sum w)^2 = 1
    se = np.sqrt(max(var, T(0.0))) / s["norm"]
    if leave_one_out:
        dens = kernel_sums(y, w, y, 0, T)[0] / (s["norm"] * (T(1.0) - w))
    else:
        dens = kernel_sums(y, w, y, -1, T)[0] / s["norm"]
    above = dens > p_zero
    p_exceed = (w * above).sum()
    count = int(above.sum())
    neff = s["neff"]
    saturated = bool(above.all())
    p_for_sigma = T(1.0) - T(1.0) / neff if saturated else p_exceed
    return dict(p_exceed=p_exceed, count=count, n_sigma=sigma_of(p_for_sigma), saturated=saturated, p_zero=p_zero, p_zero_se=se,
                n_eff=neff, densities=dens, ratio=dens / p_zero)


def scipy_kde(samples, weights=None, bandwidth="silverman"):
    """scipy.stats.gaussian_kde for the same arguments; a matrix bandwidth is installed as the kernel covariance."""
    from scipy import linalg, stats

    samples = np.asarray(samples, dtype=np.float64)
    if isinstance(bandwidth, np.ndarray):
        kde = stats.gaussian_kde(samples.T, bw_method=1.0, weights=weights)
        kde._data_covariance = np.asarray(bandwidth, dtype=np.float64)
        kde._data_cho_cov = linalg.cholesky(kde._data_covariance, lower=True)
        kde.set_bandwidth(1.0)
        return kde
    return stats.gaussian_kde(samples.T, bw_method=bandwidth, weights=weights)


def gaussian_chain(n, d, k, seed):
    """A Gaussian difference chain [n, d] whose mean lies k sigma from zero along a random direction of a random covariance:
    the exact shift probability is chi^2_d's CDF at k^2."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((d, d))
    cov = a @ a.T + 0.5 * np.eye(d)
    L = np.linalg.cholesky(cov)
    u = rng.standard_normal(d)
    u /= np.linalg.norm(u)
    return (L @ (k * u))[None, :] + rng.standard_normal((n, d)) @ L.T
