"""Shapes and inputs of the cf_kde_sum_device sweep (tests/test_gpu_kde_kernels.py): the smallest sizes at which tiling, slicing
and the self skip can go wrong.  T and S are the kernel's tile and slice lengths (include/cosmofit.h through _lib)."""
import importlib

import numpy as np

_lib = importlib.import_module("cosmology-model-fit_amd")._lib
T, S = _lib.CF_KDE_TILE, _lib.CF_KDE_SLICE

N = (1, 2, 63, 64, 65, 257, T - 1, T, T + 1, S - 1, S, S + 1, 2 * S + 3)
M = (1, 2, 255, 256, 257, 1025)
NDIM = tuple(range(1, _lib.CF_KDE_MAX_NDIM + 1))
SELF = (-1, 0, 5)


def _cases():
    """Every n with every dimension (104 cases); m, self_offset and weighted walk through their values with periods 6, 3 and 2
    of one running index (3 and 2 coprime, m on the index // 3), so that every m meets every self_offset and both kinds of
    weights.  (n, ndim, m, self_offset, weighted) as asked for; ``fit`` clips m and self_offset to what n allows."""
    out = []
    for i_d, d in enumerate(NDIM):
        for i_n, n in enumerate(N):
            k = i_n + len(N) * i_d
            out.append((n, d, M[(k // 3) % len(M)], SELF[k % len(SELF)], bool(k % 2)))
    return out


CASES = _cases()


def fit(n, m, self_offset):
    """(m, self_offset) the call is made with: with a self_offset the queries ARE samples self_offset .. self_offset + m - 1,
    so both are clipped to n (n = 1 keeps one query at offset 0)."""
    if self_offset < 0:
        return m, self_offset
    off = min(self_offset, n - 1)
    return min(m, n - off), off


def inputs(n, ndim, m, self_offset, weighted, seed):
    """(y [n, ndim], w [n] or None, q [m, ndim]): whitened-scale samples; weights 10^-3 .. 1 with every seventh zero; queries
    a little wider than the samples, or the samples themselves where self_offset >= 0."""
    rng = np.random.default_rng([seed, n, ndim, m])
    y = rng.standard_normal((n, ndim))
    w = None
    if weighted:
        w = 10.0 ** rng.uniform(-3.0, 0.0, n)
        w[3::7] = 0.0
    if self_offset >= 0:
        q = np.ascontiguousarray(y[self_offset: self_offset + m])
    else:
        q = 1.2 * rng.standard_normal((m, ndim))
    return y, w, q
