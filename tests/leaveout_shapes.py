"""Shapes, groups and host-side helpers the leave-group-out tests share (tests/test_leaveout_cpu.py,
tests/test_gpu_leaveout_kernels.py, tests/test_gpu_leaveout.py)."""
import numpy as np

# group_quad_kernel: n around the tile and the row block; m around the k step of 4, the 16-wide tile and the 64-wide column block
# (257: five column blocks, the last one a single tile); S around a row tile, a wave's rows and a workgroup's 64 rows
N_QUAD = (1, 2, 17, 64, 65, 257)
M_QUAD = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257)
S_QUAD = (1, 2, 15, 16, 17, 257)
S_MAX = 257
M_HOST = (1, 2, 17, 64, 65, 257)          # cf_selftest_group_host
M_BRUTE = (1, 5, 17, 64, 200)             # the restatement against the deleted problem, n = 257
# cf_reweight_device: S around a slice of 2048 rows (4097: three slices), G and ncol at their ends and in between
S_RW = (1, 2, 2047, 2048, 2049, 4097)
G_RW = (1, 3, 33)
NCOL_RW = (1, 4, 16)
GAUSS_CASES = ((0.5, 1.0), (0.0, 1.5), (1.0, 1.3))
GPD_K, GPD_SEEDS, GPD_M = (0.1, 0.5, 0.9), (1, 2, 3), 2000


def quad_groups(n, seed=0):
    """(groups, n_sized): one shuffled group of every size of M_QUAD that fits n (they overlap; the one of size n is the whole
    block), then every datum as a singleton."""
    rng = np.random.default_rng(900 + n + seed)
    sized = [rng.permutation(n)[:m].astype(np.int32) for m in M_QUAD if m <= n]
    return sized + [np.array([i], dtype=np.int32) for i in range(n)], len(sized)


def shuffled_group(n, m, seed):
    return np.random.default_rng(seed).permutation(n)[:m].astype(np.int32)


def reweight_inputs(S, G, ncol, seed=0):
    """(lw [S, G], w0 [S], x [S, ncol], pivot [ncol]): log-weights near -700 with outliers of +-800, -inf entries, NaN and +inf
    entries, rows whose x is NaN, zero base weights."""
    rng = np.random.default_rng(1000 * seed + 7 * S + 3 * G + ncol)
    lw = -700.0 + 3.0 * rng.standard_normal((S, G))
    x = rng.standard_normal((S, ncol)) * np.linspace(0.5, 20.0, ncol)[None, :] + np.linspace(-3.0, 70.0, ncol)[None, :]
    w0 = rng.uniform(0.0, 2.0, S)
    if S >= 16:
        pick = lambda k: rng.choice(S, size=k, replace=False)
        for b in range(G):
            if b % 2:  # the even columns keep many comparable terms in their sums
                lw[pick(2), b] = (800.0, -800.0)
            lw[pick(2), b] = -np.inf
            lw[pick(1), b] = np.nan
            lw[pick(1), b] = np.inf
        quiet = np.nonzero(~(lw == 800.0).any(axis=1))[0]            # the outliers keep their rows
        x[rng.choice(quiet, size=3, replace=False), rng.integers(ncol)] = (np.nan, np.inf, -np.inf)
        zero = rng.choice(quiet, size=3, replace=False)
        w0[zero] = 0.0
        lw[zero[0], :] = 900.0                                  # the largest lw sits on a row of base weight 0: it sets no scale
    ok = np.isfinite(x).all(axis=1)
    pivot = (w0[ok, None] * x[ok]).sum(axis=0) / w0[ok].sum() if w0[ok].sum() > 0 else np.zeros(ncol)
    return lw, w0, x, pivot
