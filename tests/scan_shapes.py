"""Shapes, covariances, residual rows, bases and candidate families the template-scan tests share (tests/test_scan_cpu.py,
tests/test_gpu_scan_kernels.py, tests/test_gpu_scan.py), and the restatement of every kernel shape, computed once per process
and left unchanged.  The covariances and residual rows are made as ``cscale_shapes`` makes its own."""
import importlib

import numpy as np

import cscale_shapes as CS
import marg_shapes as MS
import scan_reference as SR

TILE = 64                      # CF_SCAN_TILE: the column tile of the row records and the row block of the column sums
# prepare (CPU): the sizes and base widths the issue names
N_CPU = (1, 2, 33, 65, 257)
M0_CPU = (0, 1, 3, 16)
PRIORS = ("flat", "gauss")
# the kernels: (n, K, m0, sign) -- n around the k step of 4, the 16-wide tile, the 32-wide staged tile and the 64-wide block; K
# around the 16-wide MFMA tile and the 64-wide column tile, one, two and five column tiles; every sign; every base width
KERNEL = ((1, 1, 0, 0), (2, 2, 0, 1), (2, 17, 0, 0), (31, 15, 1, 0), (32, 16, 3, -1), (33, 17, 0, 1), (63, 63, 16, 0),
          (64, 64, 1, 0), (65, 65, 3, 1), (31, 64, 0, 0), (63, 1, 0, -1), (64, 2, 1, 1), (33, 129, 1, 0), (65, 257, 0, 0),
          (257, 129, 16, -1), (257, 257, 3, 0), (257, 63, 1, 1), (2, 1, 1, 0), (32, 65, 0, -1))
LARGE = (1701, 4096, 1, 0)     # many k tiles and column tiles; 64 rows
S_KERNEL = (1, 2, 63, 64, 65, 257)
S_MAX, S_LARGE = 257, 64
POSITIONS = (0, 15, 16, 63, 64, 200, 256)
CHUNKS = (32, 96, 257)
N_ENGINE = (63, 65, 257)
EXCUSED_MAX = 0.01             # the share of rows that may be excused from index equality

covariance = CS.covariance
residual_rows = CS.residual_rows


def base(n, m0):
    """(A0 [n, m0], sigma [m0]): a column of ones, then random columns; flat priors on the first min(n - 1, m0) components (so
    that candidates keep a direction of their own), Gaussian ones on the rest."""
    if m0 == 0:
        return None, None
    A0 = MS.width(n, m0)
    rng = np.random.default_rng(2300 + 19 * n + m0)
    sigma = rng.uniform(0.05, 0.5, m0)
    sigma[:min(max(n - 1, 0), m0):2] = np.inf
    if n == 1:
        sigma[:] = rng.uniform(0.05, 0.5, m0)
    return A0, sigma


def candidates(n, K, A0, seed=0):
    """(cand [n, K], sigma [K]): random columns, every fifth a 0/1 mask; candidate 1 (when there are at least three and a base)
    repeats base column 0 with a flat prior (dead when that base column is flat); every fourth has a Gaussian prior."""
    rng = np.random.default_rng(2900 + 23 * n + K + seed)
    A = rng.standard_normal((n, K))
    for k in range(4, K, 5):
        A[:, k] = (rng.uniform(size=n) < 0.4).astype(np.float64)
        if not A[:, k].any():
            A[0, k] = 1.0
    sigma = np.full(K, np.inf)
    sigma[3::4] = rng.uniform(0.2, 2.0, sigma[3::4].size)
    if K >= 3 and A0 is not None:
        A[:, 1] = A0[:, 0]
        sigma[1] = np.inf
    return A, sigma


class KernelCase:
    """One kernel shape: factor, base, candidates, ``scan.prepare``'s result, residual rows and the restatement for them
    (scores for every candidate; for LARGE the scores of a shortlist: the candidates a float64 restatement puts within 1e-6 of a
    row's maximum, plus a spread sample), the tolerances and the restatement's winners."""

    def __init__(self, pkg, shape):
        scan = importlib.import_module(pkg.__name__ + ".scan")
        self.shape = shape
        self.n, self.K, self.m0, self.sign = n, K, m0, sign = shape
        self.S = S_LARGE if shape == LARGE else S_MAX
        self.chol = np.linalg.cholesky(covariance(pkg, n))
        self.A0, self.s0 = base(n, m0)
        self.cand, self.sk = candidates(n, K, self.A0)
        self.prep = scan.prepare(self.chol, self.cand, base=self.A0, base_sigma=self.s0, cand_sigma=self.sk)
        self.rows = residual_rows(self.chol, self.S, seed=n + K)
        args = dict(base=self.A0, base_sigma=self.s0)
        if shape == LARGE:
            f64 = SR.restate(self.chol, self.cand, self.rows, cand_sigma=self.sk, dtype=np.float64, **args)
            stat = np.where(f64["live"][None, :], SR.statistic(f64["s"], sign), -1.0)
            top = stat.max(axis=1, keepdims=True)
            near = (stat >= top * (1.0 - 1e-6)) & (top > 0)   # a row of zeros ties everywhere: its winner is the first live candidate
            cols = np.unique(np.concatenate([np.nonzero(near.any(axis=0))[0], np.arange(0, K, 509), [1, 2, K - 1]]))
            self.live64 = f64["live"]
        else:
            cols = np.arange(K)
        self.cols = cols
        self.ref = SR.restate(self.chol, self.cand[:, cols], self.rows, cand_sigma=self.sk[cols], **args)
        self.scale = SR.scale(self.prep["V"], self.rows)                      # [S]
        self.tol = SR.BAR * self.scale                                        # on a score
        top, k, s_top, gap = SR.best(self.ref["s"], self.ref["live"], sign)
        self.best_ref, self.best_k_ref, self.s_best_ref = top, cols[k], s_top
        self.best_tol = 2.0 * self.tol * np.abs(np.asarray(s_top, dtype=np.float64))
        # near ties: a runner-up within twice the tolerance of the winner, exact ties apart (they go to the smallest k on both sides)
        self.excused = (gap > 0) & (gap <= 2.0 * self.best_tol)


_KERNEL_CASES = {}


def kernel_case(pkg, shape):
    if shape not in _KERNEL_CASES:
        _KERNEL_CASES[shape] = KernelCase(pkg, shape)
    return _KERNEL_CASES[shape]
