"""
The numbers behind a corner plot, computed where the chain lives: 1-D and 2-D histograms, contour heights, quantiles.

Every likelihood script of the reference ends in ``plot_corner_and_chains`` (corner_plot.py:6-20: 100 bins, the central
99.99 % range per parameter, Gaussian smoothing with sigma 2, contour levels 0.393 / 0.864, title quantiles 0.159 / 0.5 /
0.841); the nautilus scripts draw a weighted triangle plot and print weighted mean +- std (bao/desi_cmb_des5y.py:169-207).
Drawing stays out of this project; what the drawing needs is a reduction over the largest array the project holds, and that
array is on the GPU already.

* ``histograms``: bin edges as ``np.linspace`` makes them, then csrc/cosmofit_marginals.hip: one pass writes numpy's bin of
  every value as a byte, a second pass builds the histograms from the bytes with integer atomics.  Unweighted counts are
  exact; weighted sums are fixed-point integers (below), so both have the same bits on every run.
* ``corner_data``: ``histograms`` plus what ``corner.corner`` derives from them on the host (80 KB per histogram, not hot):
  scipy's ``gaussian_filter`` restated in numpy, ``corner.hist2d``'s contour heights, ``corner.quantile``'s quantiles.
* ``weighted_mean_std``: getdist's ``mean`` and ``std`` of weighted samples, as the nautilus scripts print them.

Fixed-point weights: a row's weight enters every sum as q = rint(w / w_max * 2^s), s = 62 - ceil(log2 n), so the int64 sum of
n rows is at most 2^62; the histogram is (sum of q) * (w_max / 2^s).  A bin of c rows is off by at most c * w_max * 2^-(s+1).

The inputs are float64 tensors on an MI355X; there is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._args import float64_tensor, on_device, ptr, stream_of
from .chain_stats import percentile

MAX_BINS, MAX_NDIM, MAX_PAIRS = _lib.CF_MARG_MAX_BINS, _lib.CF_MARG_MAX_NDIM, _lib.CF_MARG_MAX_PAIRS


# ---- host side: what corner and scipy do with a histogram -------------------------------------------------------------
def gaussian_smooth(h: np.ndarray, sigma: float) -> np.ndarray:
    """``scipy.ndimage.gaussian_filter(h, sigma)`` with its defaults, in numpy: per axis a correlation with the weights
    exp(-x^2 / (2 sigma^2)), x = -r .. r, r = int(4 sigma + 0.5), normalised by their sum; boundary mode ``reflect``
    (d c b a | a b c d | d c b a: numpy's pad mode ``symmetric``, which like scipy wraps as often as the radius needs)."""
    h = np.asarray(h, dtype=np.float64)
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError("sigma must be > 0")
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    k = np.exp(-0.5 / (sigma * sigma) * x**2)
    k = k / k.sum()
    out = h
    for axis in range(h.ndim):
        n = out.shape[axis]
        pad = [(0, 0)] * out.ndim
        pad[axis] = (r, r)
        p = np.pad(out, pad, mode="symmetric")
        acc = np.zeros_like(out)
        for j in range(2 * r + 1):
            sl = [slice(None)] * out.ndim
            sl[axis] = slice(j, j + n)
            acc += k[j] * p[tuple(sl)]
        out = acc
    return out


def contour_heights(h: np.ndarray, levels: Sequence[float]) -> np.ndarray:
    """``corner.hist2d``'s heights V: flatten, sort descending, sm = cumsum / total, V[i] = the last height with sm <= level
    (the largest height if there is none), then V ascending."""
    flat = np.asarray(h, dtype=np.float64).flatten()
    flat = flat[np.argsort(flat)[::-1]]
    sm = np.cumsum(flat)
    sm /= sm[-1]
    v = np.empty(len(levels))
    for i, v0 in enumerate(levels):
        below = flat[sm <= v0]
        v[i] = below[-1] if below.size else flat[0]
    v.sort()
    return v


def _weighted_quantile(x: torch.Tensor, w: torch.Tensor, q) -> np.ndarray:
    """``corner.quantile(x, q, weights=w)`` for every column of x [n, k]: [len(q), k] numpy.  The sort and the gather of the
    weights run where x lives; the running sum is ``np.cumsum`` on a host copy of the sorted weights, because corner's cdf is a
    sequential float sum and a parallel scan has other bits.  So this path copies 2 n doubles per column to the host (weighted
    samples are nested-sampling posteriors, some 10^5 rows).  cdf = cumsum(w_sorted)[:-1] / its last element, with a leading
    0; the quantile is the linear interpolation of the sorted x at q.  The sort is stable; numpy's argsort in corner is not, so
    among equal x with different weights corner's own result depends on its sort and only then can the bits differ."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if np.any(q < 0.0) or np.any(q > 1.0) or np.isnan(q).any():
        raise ValueError("Quantiles must be between 0 and 1")
    n, k = x.shape
    if n < 2:
        raise ValueError("weighted quantiles need at least two samples")
    out = np.empty((len(q), k))
    for c in range(k):
        xs, order = torch.sort(x[:, c], stable=True)
        sw = w[order].cpu().numpy()
        cdf = np.cumsum(sw)[:-1]
        if not cdf[-1] > 0:
            raise ValueError("weighted quantiles need a weight > 0 below the largest sample of every column "
                             "(corner's cdf is normalised by the sum of all weights but the last)")
        cdf /= cdf[-1]
        cdf = np.append(0, cdf)
        out[:, c] = np.interp(q, cdf, xs.cpu().numpy())
    return out


# ---- argument checks --------------------------------------------------------------------------------------------------
def _samples(samples, what: str) -> torch.Tensor:
    """Shape and type first, the device last: a wrong argument is reported the same with and without a GPU."""
    samples = float64_tensor(samples, what)
    if samples.dim() != 2 or samples.shape[0] < 1 or not 1 <= samples.shape[1] <= MAX_NDIM:
        raise ValueError(f"{what} takes samples [n, k] with n >= 1 and 1 <= k <= {MAX_NDIM}")
    if samples.shape[0] > 2**31 - 1:
        raise ValueError(f"{what} takes at most 2^31 - 1 rows")
    return samples


def _weights(weights, n: int, what: str) -> Tuple[torch.Tensor, float]:
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64:
        raise ValueError(f"{what} takes the weights as a float64 tensor")
    if weights.dim() != 1 or weights.shape[0] != n:
        raise ValueError("weights must be [n], one per sample")
    w = weights.contiguous()
    ok, w_max = torch.stack([(torch.isfinite(w) & (w >= 0)).all().to(torch.float64), w.max()]).cpu().tolist()
    if not ok:
        raise ValueError("weights must be finite and >= 0")
    if not w_max > 0:
        raise ValueError("at least one weight must be > 0")
    return w, float(w_max)


def _device(x: torch.Tensor, w: Optional[torch.Tensor], what: str) -> torch.Tensor:
    x = on_device(x, what)
    if w is not None and w.device != x.device:
        raise ValueError("weights must be on the device of the samples")
    return x.contiguous()


def _bins(bins) -> int:
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must be an integer in 1 .. {MAX_BINS}")
    return int(bins)


def default_pairs(k: int) -> np.ndarray:
    """All (a, b) with a > b in the order corner lays out its lower triangle (row a, column b): (1, 0), (2, 0), (2, 1), ...
    H[p] has the row's parameter a on axis 0; corner's own H (histogram2d(x_b, x_a)) is its transpose."""
    return np.array([(a, b) for a in range(k) for b in range(a)], dtype=np.int32).reshape(-1, 2)


def _pairs(pairs, k: int) -> np.ndarray:
    if pairs is None:
        return default_pairs(k)
    p = np.asarray(pairs)
    if p.size == 0:
        return np.empty((0, 2), dtype=np.int32)
    if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError("pairs must be a list of (a, b) column indices")
    if p.shape[0] > MAX_PAIRS:
        raise ValueError(f"at most {MAX_PAIRS} pairs per call")
    if p.min() < 0 or p.max() >= k:
        raise ValueError(f"pair index out of range (columns are 0 .. {k - 1})")
    return np.ascontiguousarray(p, dtype=np.int32)


def _is_fraction(rng) -> bool:
    return isinstance(rng, (float, int, np.floating, np.integer)) and not isinstance(rng, bool)


def _quantiles(x: torch.Tensor, w: Optional[torch.Tensor], q) -> np.ndarray:
    """``corner.quantile`` per column, [len(q), k] numpy: np.percentile(x, 100 q) without weights (its bits, by
    chain_stats.percentile), corner's weighted definition with them."""
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if w is None:
        return percentile(x, list(100.0 * q)).cpu().numpy()
    return _weighted_quantile(x, w, q)


def _ranges(x: torch.Tensor, rng, w: Optional[torch.Tensor]) -> np.ndarray:
    """[k, 2] (lo, hi) per column.  None: (min, max); per column a (lo, hi) or a fraction r, as ``corner`` accepts (a single
    fraction serves every column): quantile(x, [0.5 - r/2, 0.5 + r/2]), unweighted with np.percentile's bits
    (chain_stats.percentile), weighted by corner's definition."""
    n, k = x.shape
    out = np.empty((k, 2))
    if rng is None:
        out[:, 0], out[:, 1] = x.min(dim=0).values.cpu().numpy(), x.max(dim=0).values.cpu().numpy()
    else:
        if _is_fraction(rng):
            rng = [float(rng)] * k
        rng = list(rng)
        if len(rng) != k:
            raise ValueError("range needs one entry per column")
        fractions = {}
        for c, r in enumerate(rng):
            if np.ndim(r) == 0:
                r = float(r)
                if not 0.0 < r <= 1.0:
                    raise ValueError("a range fraction must be in (0, 1]")
                fractions.setdefault(r, []).append(c)
            else:
                lo, hi = r
                out[c] = float(lo), float(hi)
        for r, cols in fractions.items():
            out[cols] = _quantiles(x[:, cols], w, [0.5 - 0.5 * r, 0.5 + 0.5 * r]).T
    with np.errstate(over="ignore"):
        width = out[:, 1] - out[:, 0]
    if not np.isfinite(out).all() or not (out[:, 0] < out[:, 1]).all():
        raise ValueError("every column needs a finite range with lo < hi (a parameter without dynamic range has no histogram)")
    if not np.isfinite(width).all() or (width < np.finfo(np.float64).tiny).any():
        raise ValueError("the width hi - lo of every range must be a finite normal number")
    return out


# ---- the device passes ------------------------------------------------------------------------------------------------
def histograms(samples: torch.Tensor, bins: int = 100, range=None, weights: Optional[torch.Tensor] = None, pairs=None,
               n_segments: int = 0):
    """(edges [k, bins + 1] numpy, h1 [k, bins], h2 [npairs, bins, bins], pairs [npairs, 2] numpy) of samples [n, k].

    h1[c] is ``np.histogram(x[:, c], bins, range[c])[0]`` and h2[p] is ``np.histogram2d(x[:, a], x[:, b], bins, [range[a],
    range[b]])[0]`` for (a, b) = pairs[p], as device tensors: int64 counts, exactly numpy's; with ``weights`` float64 sums
    within the fixed-point bound of the module's head.  ``pairs`` defaults to ``default_pairs(k)``; ``n_segments`` is the
    launch geometry of the histogram pass (0: chosen by the library) and never changes a bit of the result."""
    n, k = _samples(samples, "histograms").shape
    bins = _bins(bins)
    pr = _pairs(pairs, k)
    w, w_max = (None, 0.0) if weights is None else _weights(weights, n, "histograms")
    x = _device(samples, w, "histograms")
    lo_hi = _ranges(x, range, w)
    edges = np.stack([np.linspace(lo, hi, bins + 1) for lo, hi in lo_hi])
    L, lib = _lib, _lib.lib()
    with torch.cuda.device(x.device):
        stream = stream_of(x.device)
        d_edges = torch.from_numpy(edges).to(x.device)
        idx = torch.empty((n, k), dtype=torch.uint8, device=x.device)
        L.check(lib.cf_marg_bin(x.data_ptr(), n, k, d_edges.data_ptr(), bins, idx.data_ptr(), stream))
        h1 = torch.empty((k, bins), dtype=torch.int64, device=x.device)
        h2 = torch.empty((len(pr), bins, bins), dtype=torch.int64, device=x.device)
        L.check(lib.cf_marg_hist(idx.data_ptr(), None if w is None else w.data_ptr(), w_max, n, k, bins,
                                 ptr(pr), len(pr), h1.data_ptr(), h2.data_ptr() if len(pr) else None,
                                 int(n_segments), stream))
    if w is not None:
        scale = np.ldexp(w_max, -fixed_point_shift(n))
        h1, h2 = h1.to(torch.float64) * scale, h2.to(torch.float64) * scale
    return edges, h1, h2, pr


def fixed_point_shift(n: int) -> int:
    """s = 62 - ceil(log2 n): a weight is quantised to rint(w / w_max * 2^s)."""
    return 62 - (int(n) - 1).bit_length()


def corner_data(samples: torch.Tensor, bins: int = 100, range=0.9999, smooth: Optional[float] = 2.0,
                smooth1d: Optional[float] = 2.0, levels=(0.393, 0.864), quantiles=(0.159, 0.5, 0.841),
                weights: Optional[torch.Tensor] = None) -> dict:
    """What ``corner.corner(samples, bins, range, smooth, smooth1d, levels, quantiles, weights)`` computes before it draws,
    as numpy arrays; the defaults are the arguments of the reference's corner_plot.py:7-20.

    edges [k, bins + 1]; h1 [k, bins] and h2 [npairs, bins, bins] raw; h1_smooth / h2_smooth after the Gaussian filter
    (equal to the raw ones where smooth1d / smooth is None); pairs [npairs, 2] (``default_pairs``); V [npairs, len(levels)],
    the contour heights of h2_smooth, ascending; levels; quantiles [len(quantiles), k] (np.percentile's bits unweighted,
    corner.quantile's definition weighted); q, the quantile levels."""
    n, k = _samples(samples, "corner_data").shape
    bins = _bins(bins)
    w = None if weights is None else _weights(weights, n, "corner_data")[0]
    x = _device(samples, w, "corner_data")
    q = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if _is_fraction(range):  # one sort serves the range and the title quantiles (each quantile has the bits it has alone)
        r = float(range)
        if not 0.0 < r <= 1.0:
            raise ValueError("a range fraction must be in (0, 1]")
        vals = _quantiles(x, w, np.concatenate([[0.5 - 0.5 * r, 0.5 + 0.5 * r], q]))
        range, qv = [tuple(v) for v in vals[:2].T], vals[2:]
    else:
        qv = _quantiles(x, w, q) if q.size else np.empty((0, k))
    edges, h1, h2, pr = histograms(x, bins=bins, range=range, weights=w)
    h1 = h1.cpu().numpy().astype(np.float64)
    h2 = h2.cpu().numpy().astype(np.float64)
    h1s = h1 if smooth1d is None else np.stack([gaussian_smooth(h, smooth1d) for h in h1])
    h2s = h2 if smooth is None or not len(pr) else np.stack([gaussian_smooth(h, smooth) for h in h2])
    levels = np.asarray(levels, dtype=np.float64)
    V = np.stack([contour_heights(h, levels) for h in h2s]).reshape(len(pr), len(levels)) if len(pr) else \
        np.empty((0, len(levels)))
    return dict(edges=edges, h1=h1, h1_smooth=h1s, h2=h2, h2_smooth=h2s, pairs=pr, V=V, levels=levels, quantiles=qv, q=q)


def weighted_mean_std(samples: torch.Tensor, weights: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean [k], std [k]) on the device: sum(w x) / sum(w) and sqrt(sum(w (x - mean)^2) / sum(w)), no ddof: getdist's
    ``mean`` and ``std`` of weighted samples."""
    if not isinstance(samples, torch.Tensor) or samples.dtype != torch.float64 or samples.dim() != 2 or samples.shape[0] < 1:
        raise ValueError("weighted_mean_std takes float64 samples [n, k]")
    w, _ = _weights(weights, samples.shape[0], "weighted_mean_std")
    x = _device(samples, w, "weighted_mean_std")
    tot = w.sum()
    mean = (w[:, None] * x).sum(dim=0) / tot
    var = (w[:, None] * (x - mean) ** 2).sum(dim=0) / tot
    return mean, torch.sqrt(var)
