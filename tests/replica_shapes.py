"""Shapes, starts and callables of the replica-ensemble tests (tests/test_replica_cpu.py, tests/test_gpu_replica_kernels.py,
tests/test_gpu_replica.py): the smallest shapes at which the kernels of csrc/cosmofit_replica.hip can still go wrong.

  ndim 1 (the edge), 4, 9 (the run-time-dimension KDE fit);
  w 6 (one triple pair per split: the smallest DE-by-thirds replica), 24, 150 (75 active rows per replica: waves straddle replica
  boundaries);
  R 1, 3, 5 (R = 5 with w = 150 is 375 active rows: past one 256-thread block).
The KDE move needs w / 2 > ndim, so ndim 9 goes with w = 24 and 150 and ndim 4 with w >= 24."""
import numpy as np
import torch

# (R, w, ndim)
SHAPES = [(1, 6, 1), (5, 6, 1), (3, 24, 4), (5, 150, 4), (3, 24, 9), (1, 150, 9)]
MIXED = (("kde", 0.30), ("de", 0.70))
# name -> (moves, de_splits)
MOVE_SETS = {"stretch": ((("stretch", 1.0),), 3), "de3": ((("de", 1.0),), 3), "de2": ((("de", 1.0),), 2),
             "kde": ((("kde", 1.0),), 3), "mixed": (MIXED, 3)}


def starts(R, w, ndim, seed=0, centre=0.0, scale=1.0):
    rng = np.random.default_rng(1000 * seed + 100 * R + 10 * w + ndim)
    return centre + scale * rng.standard_normal((R, w, ndim))


def seeds_for(R, seed=0):
    """Planted seeds: small, above 2^63 and negative ones in turn."""
    pool = [7 + seed, (1 << 63) + 12345 + seed, -3 - seed, 2 ** 40 + seed, 11 + seed]
    return [pool[r % len(pool)] + 1000 * (r // len(pool)) for r in range(R)]


def columnwise_log_prob(ndim):
    """A correlated Gaussian written with elementwise column operations only (no reduction over a row), so a row gets the same
    bits at any position of any batch: log P = -1/2 sum_k ((x_k - 0.1 k) / (1 + 0.25 k))^2 - 0.05 sum_k x_k x_{k-1}."""

    def f(x):
        out = None
        for k in range(ndim):
            z = (x[:, k] - 0.1 * k) * (1.0 / (1.0 + 0.25 * k))
            t = -0.5 * (z * z)
            if k:
                t = t - 0.05 * (x[:, k] * x[:, k - 1])
            out = t if out is None else out + t
        return out

    return f


# ---- the targets of the statistical tests -----------------------------------------------------------------------------------
BOX = np.array([[-10.0, 10.0], [-10.0, 10.0]])
LOG_Z = -2.0 * np.log(20.0)  # a normalised likelihood times the flat prior 1 / 20^2 of BOX (the tails outside are < 1e-20)
GAUSS_SIGMA = (1.0, 0.5)


def gaussian_ll(x):
    s0, s1 = GAUSS_SIGMA
    a, b = x[:, 0] * (1.0 / s0), x[:, 1] * (1.0 / s1)
    return -0.5 * (a * a) - 0.5 * (b * b) - float(np.log(2.0 * np.pi * s0 * s1))


def two_mode_ll(x):
    """0.3 N((4, 0), 0.5^2) + 0.7 N((-4, 0), 0.5^2), normalised."""
    s = 0.5
    y2 = x[:, 1] * x[:, 1]
    a = -0.5 * ((x[:, 0] - 4.0) * (x[:, 0] - 4.0) + y2) * (1.0 / (s * s)) + float(np.log(0.3))
    b = -0.5 * ((x[:, 0] + 4.0) * (x[:, 0] + 4.0) + y2) * (1.0 / (s * s)) + float(np.log(0.7))
    return torch.logaddexp(a, b) - float(np.log(2.0 * np.pi * s * s))


def _ladder(first, n):
    b = np.concatenate([[0.0], np.geomspace(first, 1.0, n)])
    b[-1] = 1.0  # the posterior rung exactly, whatever the rounding of the last power
    return b


def gauss_betas():
    return _ladder(0.01, 7)


def two_mode_betas():
    return _ladder(0.003, 9)
