"""CPU: the host half of marginals.py against numpy / scipy / corner's definitions (tests/marginals_reference.py) and its
argument checks.  The last three tests do not touch the package: they keep the prototype of the two rules the kernels of
csrc/cosmofit_marginals.hip implement -- the guess-and-fix-up bin rule and the fixed-point weights with their bound -- checked
in numpy on the inputs and against the judge that tests/test_gpu_marginals_kernels.py then applies to the kernels themselves."""
import importlib

import numpy as np
import pytest
import torch

import marginals_reference as mr
import marginals_shapes as ms
from conftest import PKG_NAME

marginals = importlib.import_module(PKG_NAME + ".marginals")

LD = np.longdouble


@pytest.fixture(scope="module")
def M():
    return marginals


# ---- smoothing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.0, 3.5])
@pytest.mark.parametrize("size", [1, 2, 5, 100])
def test_smoothing_is_scipys_gaussian_filter(M, sigma, size):
    """Relative 1e-14 elementwise on non-negative input.  The bar: per axis at most 29 non-negative terms (radius
    int(4 x 3.5 + 0.5) = 14), so two passes accumulate at most about 60 roundings of 2^-53 = 7e-15 relative, whatever the
    order of the additions; sizes 1, 2 and 5 are smaller than the radius, so the reflection wraps more than once."""
    rng = np.random.default_rng(int(10 * sigma) + size)
    h1 = rng.poisson(30.0, size).astype(np.float64)
    got, want = M.gaussian_smooth(h1, sigma), mr.smooth(h1, sigma)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want))
    for shape in ((size, size), (size, 7), (3, size)):
        h2 = rng.poisson(5.0, shape).astype(np.float64) * rng.uniform(0.0, 2.0, shape)
        got, want = M.gaussian_smooth(h2, sigma), mr.smooth(h2, sigma)
        assert got.shape == want.shape
        assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want)), (sigma, shape)


# ---- levels and quantiles ---------------------------------------------------------------------------------------------
def test_contour_heights_are_corners_bit_for_bit(M):
    rng = np.random.default_rng(5)
    levels = (0.393, 0.864)
    cases = [rng.poisson(3.0, (20, 20)).astype(np.float64),              # tied heights everywhere
             mr.smooth(rng.poisson(3.0, (100, 100)).astype(np.float64), 2.0),
             np.array([[10.0, 0.0], [0.0, 0.0]]),                          # no element qualifies: sm[0] = 1 > both levels
             np.array([[6.0, 3.0], [1.0, 0.0]]),                           # the first level has none (0.6 > 0.393), the second has
             np.full((4, 4), 2.0)]                                         # every height tied
    for h in cases:
        got, want = M.contour_heights(h, levels), mr.levels_of(h, levels)
        np.testing.assert_array_equal(got, want)
        assert got[0] <= got[1]
    np.testing.assert_array_equal(M.contour_heights(cases[2], levels), [10.0, 10.0])
    np.testing.assert_array_equal(M.contour_heights(cases[3], levels), [6.0, 6.0])
    np.testing.assert_array_equal(M.contour_heights(cases[3], (0.95, 0.5)), [3.0, 6.0])  # 3 for 0.95, 6 for 0.5: ascending, whatever the order given


def test_weighted_quantile_is_corners_bit_for_bit(M):
    rng = np.random.default_rng(6)
    q = [0.00005, 0.159, 0.5, 0.841, 0.99995, 0.0, 1.0]
    for n in (2, 3, 1000, 20001):
        x = rng.standard_normal((n, 3)) * [1.0, 1e-6, 50.0] + [0.0, 3.0, -70.0]
        w = ms.lognormal_weights(n, n)
        got = M._weighted_quantile(torch.from_numpy(x), torch.from_numpy(w), q)
        for c in range(3):
            np.testing.assert_array_equal(got[:, c], mr.weighted_quantile(x[:, c], q, w))
    with pytest.raises(ValueError, match="between 0 and 1"):
        M._weighted_quantile(torch.from_numpy(x), torch.from_numpy(w), [1.5])


def test_levels_enclose_their_share_of_a_unit_gaussian(M):
    """2 x 10^5 rows of a 2-D unit Gaussian, 100 bins: V[i] is the height at which the descending running share stops at or
    below level i.  So the bins above V hold at most the level, and the bins at or above V (the tied ones included) miss it
    by less than one bin of height V.  For the smoothed histogram (no ties) that is: the share of the bins >= V is within
    one bin's share below the level."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((200_000, 2))
    h = np.histogram2d(x[:, 0], x[:, 1], bins=100, range=[(-4.5, 4.5), (-4.5, 4.5)])[0]
    levels = np.array([0.393, 0.864])
    for hh in (h, M.gaussian_smooth(h, 2.0)):
        tot = hh.sum()
        v = M.contour_heights(hh, levels)
        for lev, vi in zip(levels[::-1], v):  # V is ascending: the lowest height belongs to the largest share
            above, at_or_above = hh[hh > vi].sum() / tot, hh[hh >= vi].sum() / tot
            assert above <= lev < at_or_above + vi / tot, (lev, above, at_or_above)
    # and they are the 1- and 2-sigma contours of the Gaussian: the share of rows within radius 1 and 2
    r2 = (x**2).sum(axis=1)
    assert abs((r2 <= 1.0).mean() - 0.393) < 5e-3 and abs((r2 <= 4.0).mean() - 0.864) < 5e-3


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_every_entry_point_raises_on_bad_arguments(M):
    x = torch.zeros((10, 3), dtype=torch.float64)
    x[:, 0] = torch.arange(10)
    w = torch.ones(10, dtype=torch.float64)
    for call in (lambda: M.histograms(x), lambda: M.corner_data(x), lambda: M.weighted_mean_std(x, w),
                 lambda: M.histograms(x, weights=w), lambda: M.corner_data(x, weights=w)):
        with pytest.raises(ValueError, match="MI355X"):  # a CPU tensor: there is no fallback
            call()
    with pytest.raises(ValueError, match="MI355X"):
        M.histograms(x.numpy())
    for call in (lambda: M.histograms(x.float()), lambda: M.corner_data(x.float()), lambda: M.weighted_mean_std(x.float(), w),
                 lambda: M.histograms(x, weights=w.float()), lambda: M.weighted_mean_std(x, w.float())):
        with pytest.raises(ValueError, match="float64"):
            call()
    for bad in (-1.0, float("nan"), float("inf")):
        wb = w.clone()
        wb[4] = bad
        for call in (lambda: M.histograms(x, weights=wb), lambda: M.corner_data(x, weights=wb), lambda: M.weighted_mean_std(x, wb)):
            with pytest.raises(ValueError, match="finite and >= 0"):
                call()
    with pytest.raises(ValueError, match="> 0"):
        M.histograms(x, weights=torch.zeros(10, dtype=torch.float64))
    with pytest.raises(ValueError, match="one per sample"):
        M.histograms(x, weights=torch.ones(9, dtype=torch.float64))
    for bins in (0, 129, -3, 2.5, True):
        with pytest.raises(ValueError, match="bins"):
            M.histograms(x, bins=bins)
        with pytest.raises(ValueError, match="bins"):
            M.corner_data(x, bins=bins)
    for pairs in ([(0, 3)], [(-1, 0)], [(1, 0), (3, 3)]):
        with pytest.raises(ValueError, match="pair index out of range"):
            M.histograms(x, pairs=pairs)
    with pytest.raises(ValueError, match="samples"):
        M.histograms(torch.zeros((10, 17), dtype=torch.float64))
    with pytest.raises(ValueError, match="samples"):
        M.histograms(torch.zeros(10, dtype=torch.float64))


def test_default_pairs_are_corners_lower_triangle(M):
    np.testing.assert_array_equal(M.default_pairs(4), [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
    assert M.default_pairs(1).shape == (0, 2)
    assert [M.fixed_point_shift(n) for n in (1, 2, 3, 4, 5, 70001, 2**22, 2**31 - 1)] == [62, 61, 60, 60, 59, 45, 40, 31]
    assert all(M.fixed_point_shift(n) == mr.fixed_point_shift(n) for n in (1, 2, 3, 1000, 4097, 70001, 200_000))


# ---- the kernels' arithmetic, restated --------------------------------------------------------------------------------
def _guess_and_fix_up(x, edges):
    """The prototype of the kernel's rule, in numpy: one multiply, then comparisons with the edges themselves."""
    nb = len(edges) - 1
    lo, hi = edges[0], edges[-1]
    out = np.full(x.shape, mr.NOT_COUNTED, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        ok = (x >= lo) & (x <= hi)
    xv = x[ok]
    g = np.clip(((xv - lo) * (nb / (hi - lo))).astype(np.int64), 0, nb - 1)
    for _ in range(nb):
        down = (g > 0) & (xv < edges[g])
        if not down.any():
            break
        g[down] -= 1
    for _ in range(nb):
        up = (g < nb - 1) & (xv >= edges[np.minimum(g + 1, nb)])
        if not up.any():
            break
        g[up] += 1
    out[ok] = g
    return out


@pytest.mark.parametrize("n,ndim,bins", ms.CASES)
def test_the_bin_rule_is_numpys_on_the_planted_inputs(n, ndim, bins):
    x, lo_hi = ms.inputs(n, ndim, bins, seed=n + ndim + bins)
    edges = mr.edges_of(lo_hi, bins)
    want = mr.bin_indices(x, edges)
    for c in range(ndim):
        np.testing.assert_array_equal(_guess_and_fix_up(x[:, c], edges[c]), want[:, c])
    if n >= 4097:  # every special is in: the edges themselves land as the rule says
        for c in range(ndim):
            for i, e in enumerate(edges[c]):
                assert want[x[:, c] == e, c].tolist() == [min(i, bins - 1)] * int((x[:, c] == e).sum())
            assert (want[~np.isfinite(x[:, c]), c] == mr.NOT_COUNTED).all() and (~np.isfinite(x[:, c])).sum() == 3
        outside = (want == mr.NOT_COUNTED).mean()
        assert 0.05 < outside < 0.15, "the explicit ranges leave about 10 % of the rows outside"


@pytest.mark.parametrize("n,decades", [(1000, 0.0), (70001, 0.0), (200_000, 0.0), (200_000, 60.0), (4097, 60.0)])
def test_fixed_point_weights_stay_within_their_bound(n, decades):
    """The prototype of the fixed-point rule, in numpy: q = rint(w / w_max * 2^s), s = 62 - ceil(log2 n), summed in int64
    and multiplied back by w_max / 2^s: within count_in_bin x w_max x 2^-(s+1) + 2 ulp of the long-double sum.
    Log-normal weights with sigma 3, alone and spread over 60 decades."""
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type"
    rng = np.random.default_rng(n)
    w = ms.lognormal_weights(n, n, decades=decades)
    bins = 100
    which = np.clip((rng.standard_normal(n) * 12 + 50).astype(np.int64), 0, bins - 1)
    s = mr.fixed_point_shift(n)
    w_max = w.max()
    q = np.rint(w / w_max * 2.0**s).astype(np.int64)
    assert int(q.max()) == 2**s and n * 2**s <= 2**62
    acc = np.zeros(bins, dtype=np.int64)
    np.add.at(acc, which, q)
    got = acc.astype(np.float64) * np.ldexp(w_max, -s)
    ref, count = np.zeros(bins, dtype=LD), np.bincount(which, minlength=bins)
    np.add.at(ref, which, w.astype(LD))
    err = np.abs(got.astype(LD) - ref)
    bound = mr.fixed_point_bound(count, ref, w_max, n)
    live = count > 0
    print(f"n={n} decades={decades}: s={s}, largest error / bound {float(np.max(err[live] / bound[live])):.3g}")
    assert np.all(err <= bound)


def test_degenerate_ranges_and_weights_are_refused(M):
    x = torch.zeros((3, 1), dtype=torch.float64)
    for lo_hi in ((-1e308, 1e308), (0.0, 5e-324), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="range"):
            M._ranges(x, [lo_hi], None)
    np.testing.assert_array_equal(M._ranges(x, [(-1.0, 2.0)], None), [[-1.0, 2.0]])
    # corner's cdf is normalised by the sum of all weights but the last sorted one: zero there has no quantile
    xs = torch.tensor([[3.0], [1.0], [2.0]], dtype=torch.float64)
    with pytest.raises(ValueError, match="weight > 0 below the largest sample"):
        M._weighted_quantile(xs, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64), [0.5])
    # equal x with different weights: the stable sort keeps the rows' order
    xt = torch.tensor([[1.0], [1.0], [2.0], [0.0]], dtype=torch.float64)
    wt = np.array([0.1, 0.7, 0.2, 0.4])
    got = M._weighted_quantile(xt, torch.from_numpy(wt), [0.3, 0.6])
    order = np.argsort(xt[:, 0].numpy(), kind="stable")
    cdf = np.append(0, np.cumsum(wt[order])[:-1] / np.cumsum(wt[order])[-2])
    np.testing.assert_array_equal(got[:, 0], np.interp([0.3, 0.6], cdf, xt[:, 0].numpy()[order]))
