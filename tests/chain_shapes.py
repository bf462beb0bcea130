"""Seeded inputs, the long-double reference and the derived error bounds for the chain-statistics kernels
(csrc/cosmofit_chain.hip), shared by tests/test_gpu_chain_kernels.py and tests/test_quasar_shapes_cpu.py.

A chain is [n_t, n_s]: n_t steps of n_s series.  The reference is plain long double: m = sum(x) / n_t, d = x - m,
lagsum(tau) = sum_{t < n_t - tau} d_t d_{t + tau} (an empty sum is 0).

The bounds come from the reference's own terms, u = 2^-53:
* mean: |got - m| <= n_t u max|x| (a length-n_t sum of terms of size <= max|x|, in any order, and the division);
* lag sums: a float64 deviation differs from d_t by at most eta = n_t u max_t|x_t| (the mean's error, the subtraction's
  rounding is far below it), so with S = sum (|d_t| + eta)(|d_{t+tau}| + eta) the perturbed products move the sum by at most
  S - sum |d_t||d_{t+tau}|, and summing n_t of them in any order adds at most n_t u S.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
N_T = [1, 2, 15, 16, 17, 127, 128, 129, 130, 400, 2500]
N_S = [1, 63, 64, 65, 96, 200]
SEGS, R = 8, 16  # CF_CHAIN_SEGS, CF_CHAIN_R of the kernels
# the posterior's real ranges (mean, sd): M, H0, Omega_m, r_d -- large means against small spreads
RANGES = [(-19.3, 0.02), (70.0, 1.0), (0.3, 0.03), (147.0, 0.3)]


def series(n_t, n_s, seed, rho=0.9):
    """AR(1) series, stationary start, series s scaled and shifted to RANGES[s % 4]."""
    rng = np.random.default_rng(5000 + seed)
    x = np.empty((n_t, n_s))
    x[0] = rng.standard_normal(n_s)
    sd = np.sqrt(1.0 - rho * rho)
    for t in range(1, n_t):
        x[t] = rho * x[t - 1] + sd * rng.standard_normal(n_s)
    mean = np.array([RANGES[s % 4][0] for s in range(n_s)])
    spread = np.array([RANGES[s % 4][1] for s in range(n_s)])
    return mean[None, :] + spread[None, :] * x


def lag_ranges(n_t):
    """(lag0, nlag) of the sweep: every nlag of {1, 15, 16, 17, 64, 100}, every lag0 of {0, 1, 16, 37, n_t - 1}, and ranges
    that run past n_t."""
    return [(0, 1), (0, 15), (1, 16), (16, 17), (37, 64), (0, 100), (n_t - 1, 1), (n_t - 1, 17), (max(0, n_t - 5), 16), (1, 100)]


def reference_mean(x):
    """(m [n_s], d [n_t, n_s]) in long double."""
    xl = x.astype(LD)
    m = xl.sum(axis=0) / LD(x.shape[0])
    return m, xl - m[None, :]


def reference_lagsum(x, d, tau):
    n_t = x.shape[0]
    if tau >= n_t:
        return np.zeros(x.shape[1], dtype=LD)
    return np.sum(d[: n_t - tau] * d[tau:], axis=0)


def mean_bound(x):
    return x.shape[0] * U * np.max(np.abs(x), axis=0)


def lagsum_bound(x, d, tau):
    """float64 [n_s]; 0 for a lag at or past n_t (that sum is exactly 0)."""
    n_t = x.shape[0]
    if tau >= n_t:
        return np.zeros(x.shape[1])
    eta = (LD(n_t) * LD(U) * np.max(np.abs(x), axis=0).astype(LD))[None, :]
    a, b = np.abs(d[: n_t - tau]), np.abs(d[tau:])
    S = np.sum((a + eta) * (b + eta), axis=0)
    return ((S - np.sum(a * b, axis=0)) + LD(n_t) * LD(U) * S).astype(np.float64)


def seg_len(n_t):
    return ((n_t + SEGS - 1) // SEGS + R - 1) // R * R


def segment_mean(x):
    """float64, in the order of chain_mean_kernel: eight sequential segment sums, added in ascending order, / n_t."""
    n_t, ln = x.shape[0], seg_len(x.shape[0])
    tot = None
    for g in range(SEGS):
        acc = np.zeros(x.shape[1])
        for t in range(g * ln, min(g * ln + ln, n_t)):
            acc = acc + x[t]
        tot = acc if tot is None else tot + acc
    return tot / float(n_t)


def segment_lagsum(x, mean, tau):
    """float64, in the order of chain_lagsum_kernel: per segment the products in ascending t (a deviation past the end of the
    chain is 0), the segments added in ascending order.  Plain multiply-add where the kernel has an fma."""
    n_t, ln = x.shape[0], seg_len(x.shape[0])
    d = x - mean[None, :]
    tot = None
    for g in range(SEGS):
        acc = np.zeros(x.shape[1])
        for t in range(g * ln, min(g * ln + ln, n_t)):
            if t + tau < n_t:
                acc = acc + d[t] * d[t + tau]
        tot = acc if tot is None else tot + acc
    return tot
