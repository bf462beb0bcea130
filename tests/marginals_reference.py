"""The judge of the marginals tests: the definitions restated with numpy and scipy, nothing from the package under test.

np.histogram / np.histogram2d for counts, np.linspace for edges, np.percentile and corner's weighted quantile,
scipy.ndimage.gaussian_filter, corner.hist2d's contour heights.  Weighted sums are kept in np.longdouble."""
import numpy as np
from scipy.ndimage import gaussian_filter

LD = np.longdouble
NOT_COUNTED = 255


def edges_of(lo_hi, bins):
    return np.stack([np.linspace(lo, hi, bins + 1) for lo, hi in lo_hi])


def bin_index(x, edges):
    """numpy's bin of every value of one column, NOT_COUNTED where numpy counts nothing: np.histogramdd's own search
    (searchsorted from the right, the last edge moved into the last bin), checked here against np.histogram's counts."""
    nb = len(edges) - 1
    with np.errstate(invalid="ignore"):
        i = np.searchsorted(edges, x, side="right") - 1
        i[x == edges[-1]] = nb - 1
        bad = (i < 0) | (i >= nb) | ~np.isfinite(x)
    out = np.where(bad, NOT_COUNTED, i).astype(np.uint8)
    finite = x[np.isfinite(x)]
    counts = np.histogram(finite, bins=nb, range=(edges[0], edges[-1]))[0]
    assert np.array_equal(np.bincount(out[out != NOT_COUNTED], minlength=nb), counts), "the judge disagrees with np.histogram"
    return out


def bin_indices(x, edges):
    return np.stack([bin_index(x[:, c], edges[c]) for c in range(x.shape[1])], axis=1)


def hist1(x, lo_hi, bins):
    """np.histogram per column; non-finite values are dropped first (numpy refuses a non-finite automatic range only; with
    an explicit range it counts none of them, but it warns on NaN comparisons)."""
    return np.stack([np.histogram(x[np.isfinite(x[:, c]), c], bins=bins, range=tuple(lo_hi[c]))[0] for c in range(x.shape[1])])


def hist2(x, lo_hi, bins, pairs):
    out = np.zeros((len(pairs), bins, bins), dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        ok = np.isfinite(x[:, a]) & np.isfinite(x[:, b])
        h = np.histogram2d(x[ok, a], x[ok, b], bins=bins, range=[tuple(lo_hi[a]), tuple(lo_hi[b])])[0]
        out[p] = h.astype(np.int64)
        assert np.array_equal(out[p], h)
    return out


def weighted_hists(idx, w, bins, pairs):
    """Long-double weighted sums per bin from the judge's own indices, plus the number of rows per bin (for the bound)."""
    n, k = idx.shape
    wl = w.astype(LD)
    h1, c1 = np.zeros((k, bins), dtype=LD), np.zeros((k, bins), dtype=np.int64)
    for c in range(k):
        ok = idx[:, c] != NOT_COUNTED
        np.add.at(h1[c], idx[ok, c], wl[ok])
        np.add.at(c1[c], idx[ok, c], 1)
    h2, c2 = np.zeros((len(pairs), bins * bins), dtype=LD), np.zeros((len(pairs), bins * bins), dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        ok = (idx[:, a] != NOT_COUNTED) & (idx[:, b] != NOT_COUNTED)
        flat = idx[ok, a].astype(np.int64) * bins + idx[ok, b]
        np.add.at(h2[p], flat, wl[ok])
        np.add.at(c2[p], flat, 1)
    return h1, c1, h2.reshape(len(pairs), bins, bins), c2.reshape(len(pairs), bins, bins)


def fixed_point_shift(n):
    """s = 62 - ceil(log2 n)."""
    k = 0
    while (1 << k) < n:
        k += 1
    return 62 - k


def fixed_point_bound(count, ref_sum, w_max, n):
    """count_in_bin * w_max * 2^-(s+1) plus 2 ulp (float64) of the long-double sum."""
    s = fixed_point_shift(n)
    return count.astype(LD) * LD(w_max) * LD(2.0) ** -(s + 1) + 2 * np.spacing(np.abs(ref_sum).astype(np.float64)).astype(LD)


def weighted_quantile(x, q, w):
    """corner.quantile with weights, for one column."""
    q = np.atleast_1d(q)
    idx = np.argsort(x)
    sw = w[idx]
    cdf = np.cumsum(sw)[:-1]
    cdf /= cdf[-1]
    cdf = np.append(0, cdf)
    return np.interp(q, cdf, x[idx])


def quantile(x, q, w=None):
    """corner.quantile: np.percentile(x, 100 q) without weights."""
    q = np.atleast_1d(q)
    if w is None:
        return np.percentile(x, list(100.0 * q))
    return weighted_quantile(x, q, w)


def fraction_ranges(x, r, w=None):
    return np.stack([quantile(x[:, c], [0.5 - 0.5 * r, 0.5 + 0.5 * r], w) for c in range(x.shape[1])])


def smooth(h, sigma):
    return gaussian_filter(np.asarray(h, dtype=np.float64), sigma)


def levels_of(h, levels):
    """corner.hist2d's V."""
    hflat = np.asarray(h, dtype=np.float64).flatten()
    inds = np.argsort(hflat)[::-1]
    hflat = hflat[inds]
    sm = np.cumsum(hflat)
    sm /= sm[-1]
    v = np.empty(len(levels))
    for i, v0 in enumerate(levels):
        try:
            v[i] = hflat[sm <= v0][-1]
        except IndexError:
            v[i] = hflat[0]
    v.sort()
    return v


def weighted_mean_std(x, w):
    xl, wl = x.astype(LD), w.astype(LD)[:, None]
    tot = wl.sum()
    mean = (wl * xl).sum(axis=0) / tot
    return mean, np.sqrt((wl * (xl - mean) ** 2).sum(axis=0) / tot)
