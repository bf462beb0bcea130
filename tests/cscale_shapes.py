"""Shapes, covariances, second matrices and amplitudes the scaled-covariance tests share (tests/test_cscale_cpu.py,
tests/test_gpu_cscale_kernels.py, tests/test_gpu_cscale.py)."""
import numpy as np

import infl_shapes as IS

# n around the k step of 4, the 16-wide tile, the 32-wide slab and the 64-wide block; S around a row tile and a row block
N_ALL = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257)
S_ALL = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257)
NS_ALL = (1, 2, 5, 16)
S_MAX = 257
MAX_S = 16
KINDS = ("identity", "diag01", "c0", "rank4", "indefinite")
N_ENGINE = (63, 64, 65, 257)   # the SN engines of cf_cscale_eval_device
N_PANTHEON, S_PANTHEON = 1701, 33
CHUNKS = (32, 96, 257)
POSITIONS = (0, 15, 16, 63, 64, 200, 256)

covariance = IS.covariance
residual_rows = IS.residual_rows


def second_matrix(kind, cov, seed=0):
    """C1 of the given kind for the covariance C0 = cov: what ``decompose`` takes (a scalar, a vector or a matrix)."""
    n = cov.shape[0]
    rng = np.random.default_rng(900 + 7 * n + seed)
    if kind == "identity":
        return 1.0
    if kind == "diag01":  # the scatter of a subset: the first half of the data (at least one datum)
        d = np.zeros(n)
        d[:max(1, n // 2)] = 1.0
        return d
    if kind == "c0":
        return cov.copy()
    if kind == "rank4":
        U = 0.05 * rng.standard_normal((n, 4))
        return U @ U.T + np.diag(rng.uniform(0.001, 0.01, n))
    if kind == "indefinite":
        G = 0.02 * rng.standard_normal((n, n))
        B = G + G.T
        B[0, 0] = -abs(B[0, 0]) - 0.01  # at least one direction of each sign for n >= 2
        if n > 1:
            B[-1, -1] = abs(B[-1, -1]) + 0.01
        return B
    raise ValueError(kind)


def amplitudes(info):
    """16 amplitudes spanning (s_min, 0), 0 and up to 1 (or 0.9 s_max): three below zero, zero, the rest geometric above."""
    lo = info["s_min"] if np.isfinite(info["s_min"]) else -0.5
    hi = min(1.0, 0.9 * info["s_max"])
    return np.array([0.9 * lo, 0.5 * lo, 0.1 * lo, 0.0] + list(hi * np.geomspace(1e-3, 1.0, MAX_S - 4)))


def per_row(base, S):
    """[S, 16]: row i takes the 16 amplitudes rotated by i, so that neighbours differ; and the index into base of each entry."""
    idx = (np.arange(MAX_S)[None, :] + np.arange(S)[:, None]) % MAX_S
    return np.ascontiguousarray(base[idx]), idx
