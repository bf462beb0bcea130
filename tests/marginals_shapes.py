"""Shapes and inputs of the marginals tests (csrc/cosmofit_marginals.hip): the smallest at which the kernels can go wrong.

N: around the 64-lane wave, the 256-thread workgroup and the 4-value group of the index pass, more than one workgroup
(4097 rows), more than one automatic segment (70001 rows).  NDIM: 1, the odd ones, the limit 16.  BINS: 1, 2, 3, the
workload's 100, the limit 128 (a 128 x 128 LDS histogram).

``inputs`` plants into every column of otherwise random rows every edge, both ``nextafter`` neighbours of every edge, NaN and
+-inf (as many of them as the column has rows).  The explicit ranges leave about 10 % of the random rows outside; some
columns have a range as narrow as 1e-9 of its offset, where a multiply alone misplaces values near an edge."""
import numpy as np

N = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 70001)
NDIM = (1, 2, 3, 5, 8, 16)
BINS = (1, 2, 3, 20, 100, 128)

# every size at least twice
CASES = [(n, NDIM[(2 * k + j) % len(NDIM)], BINS[(2 * k + j + k // 3) % len(BINS)]) for k, n in enumerate(N) for j in range(2)]


def ranges(ndim, seed):
    """[ndim, 2] explicit (lo, hi): offsets of either sign, widths from 1e-9 of the offset to 1e3 times it."""
    rng = np.random.default_rng([seed, 1])
    off = rng.choice([-1.0, 1.0], ndim) * 10.0 ** rng.uniform(-2, 3, ndim)
    rel = 10.0 ** rng.choice([-9.0, -6.0, -3.0, 0.0, 3.0], ndim)
    rel[0] = 1e-9 if seed % 2 else rel[0]
    width = np.abs(off) * rel
    lo = off - 0.5 * width
    out = np.stack([lo, lo + width], axis=1)
    assert (out[:, 0] < out[:, 1]).all()
    return out


def specials(edges):
    """Every edge, its two neighbours, NaN and +-inf."""
    return np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [np.nan, np.inf, -np.inf]])


def inputs(n, ndim, bins, seed):
    """(x [n, ndim], lo_hi [ndim, 2]): random rows over the range widened by 5 % on either side, the specials planted at
    random rows of every column."""
    rng = np.random.default_rng([seed, 2])
    lo_hi = ranges(ndim, seed)
    x = np.empty((n, ndim))
    for c in range(ndim):
        lo, hi = lo_hi[c]
        w = hi - lo
        x[:, c] = rng.uniform(lo - 0.05 * w / 0.9, hi + 0.05 * w / 0.9, n)
        sp = rng.permutation(specials(np.linspace(lo, hi, bins + 1)))
        m = min(n, len(sp))
        x[rng.choice(n, m, replace=False), c] = sp[:m]
    return x, lo_hi


def lognormal_weights(n, seed, sigma=3.0, decades=0.0):
    """Log-normal weights with the given sigma (of the natural logarithm); ``decades`` > 0 multiplies each by a power of ten
    drawn uniformly over that many decades, so that 60 gives 60 decades of dynamic range whatever n is.  All finite, > 0."""
    rng = np.random.default_rng([seed, 3])
    w = rng.lognormal(0.0, sigma, n)
    if decades:
        w = w * 10.0 ** rng.uniform(-0.5 * decades, 0.5 * decades, n)
    assert np.isfinite(w).all() and (w > 0).all()
    return w


def all_pairs(ndim):
    return [(a, b) for a in range(ndim) for b in range(a)]
