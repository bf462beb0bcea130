"""Shapes, covariances, residual rows, templates and priors the nuisance-marginalisation tests share (tests/test_marg_cpu.py,
tests/test_gpu_marg_kernels.py, tests/test_gpu_marg.py).  The covariances and residual rows are made as ``cscale_shapes`` makes
its own."""
import numpy as np

import cscale_shapes as CS

SLICE = 256                    # CF_MARG_SLICE: the k slice of marg_proj_kernel
# project (CPU): the sizes and widths the issue names
N_CPU = (1, 2, 5, 33, 65, 257)
M_CPU = (1, 2, 3, 16)
PRIORS = ("flat", "gauss", "mixed")
# the kernels: n around the k step of 4, the 16-wide tile, the 64-wide staged tile and the 256-wide slice
N_KERNEL = tuple(dict.fromkeys((1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1)))
M_KERNEL = (1, 2, 3, 15, 16)
S_KERNEL = (1, 15, 16, 17, 63, 65, 257)
S_MAX = 257
POSITIONS = (0, 15, 16, 63, 64, 200, 256)
N_ENGINE = (1, 2, 63, 64, 65, 257)
CHUNKS = (32, 96, 257)
KINDS = ("ones", "ones_mask", "ones_random", "random16", "near_collinear")
NEAR = 1e-4                    # how far the nearly collinear column is from the column of ones

covariance = CS.covariance
residual_rows = CS.residual_rows


def templates(kind, n, seed=0):
    """A [n, m] of one of the named kinds.  "ones_mask" marks the first half of the data (at least one datum)."""
    rng = np.random.default_rng(1300 + 11 * n + seed)
    one = np.ones(n)
    if kind == "ones":
        return one[:, None].copy()
    if kind == "ones_mask":
        mask = np.zeros(n)
        mask[:max(1, n // 2)] = 1.0
        return np.column_stack([one, mask])
    if kind == "ones_random":
        return np.column_stack([one, rng.standard_normal(n)])
    if kind == "random16":
        return rng.standard_normal((n, 16))
    if kind == "near_collinear":
        return np.column_stack([one, one + NEAR * rng.standard_normal(n)])
    if kind == "collinear":  # exactly: project must refuse it under a flat prior
        return np.column_stack([one, 2.0 * one])
    raise ValueError(kind)


def width(n, m, seed=0):
    """A [n, m] for the sweeps over m: a column of ones, then random columns."""
    rng = np.random.default_rng(1700 + 13 * n + m + seed)
    return np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(m - 1)])


def prior(kind, n, m, seed=0):
    """(mu, sigma, box) of kind "flat", "gauss" or "mixed" (flat and Gaussian alternating; every other flat one with a box).
    At most n components can be flat (F needs full column rank on them), so components j >= n are Gaussian whatever the kind;
    so is the second of two columns that coincide on n = 1 datum."""
    rng = np.random.default_rng(1900 + 17 * n + m + seed)
    mu = rng.uniform(-0.3, 0.3, m)
    sigma = rng.uniform(0.05, 0.5, m)
    flat = {"flat": np.ones(m, bool), "gauss": np.zeros(m, bool), "mixed": np.arange(m) % 2 == 0}[kind]
    flat[n:] = False
    sigma = np.where(flat, np.inf, sigma)
    box = [(-1.5 - 0.1 * j, 2.0 + 0.1 * j) if (flat[j] and j % 4 == 0) else None for j in range(m)]
    return mu, sigma, box
