"""GPU (-m gpu): the Python layer of tension.py on an MI355X.

* kde_density against scipy.stats.gaussian_kde on a host copy: 1e-10 relative.
* kde_shift against the long-double restatement (tests/kde_reference.py) on the same samples: the unweighted count is exactly
  equal, the weighted ratio within 1e-12, and NO sample is left out of that comparison.  To keep that honest each case first
  asserts on the restatement alone that no sample has |p_{-i} / p(0) - 1| < 1e-9: a sample that close to the threshold could
  fall on either side for rounding alone.  The seeds below were checked for that on the CPU (the closest sample of any case is
  printed); the device sums are good to ~1e-13, four decades inside the margin.
* p_zero and its standard error: 1e-10 of the restatement.  The saturated flag on a chain 12 sigma from zero.
* examples/desi_union3_tension.py run small on real data: plumbing only, no physics value is asserted."""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import kde_reference as kr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble


@pytest.fixture(scope="module")
def tension(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.tension


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cloud(n, d, seed):
    """Samples of a covariance with condition number 3 and a mean a little off zero (scipy whitens in float64; see
    tests/test_tension_cpu.py::_kde_case), weights over a decade."""
    rng = np.random.default_rng([seed, n, d])
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    cov = q @ np.diag(np.linspace(1.0, 3.0, d)) @ q.T
    x = rng.standard_normal((n, d)) @ np.linalg.cholesky(cov).T + 0.8 * rng.standard_normal(d)
    return x, rng.uniform(0.1, 1.0, n), cov


@pytest.mark.parametrize("n", [257, 4097])
@pytest.mark.parametrize("d", [1, 3, 6])
@pytest.mark.parametrize("weighted", [False, True])
def test_kde_density_is_scipys_gaussian_kde(tension, n, d, weighted):
    x, w, cov = _cloud(n, d, 1)
    w = w if weighted else None
    rng = np.random.default_rng(n + d)
    at = x[:150] + 0.1 * rng.standard_normal((150, d))
    worst = 0.0
    for bw in ("silverman", "scott", 0.5, 0.2 * cov):
        got = tension.kde_density(_dev(x), _dev(at), _dev(w), bandwidth=bw).cpu().numpy()
        want = kr.scipy_kde(x, w, bw)(at.T)
        rel = float(np.max(np.abs(got - want) / want))
        worst = max(worst, rel)
        assert rel <= 1e-10, (bw if isinstance(bw, (str, float)) else "matrix", rel)
    print(f"n={n} d={d} weighted={weighted}: largest relative difference from scipy {worst:.3g}")


def test_kde_density_leave_one_out_and_planted_rows(tension):
    x, w, _ = _cloud(300, 2, 2)
    for ww in (None, w):
        got = tension.kde_density(_dev(x), None, _dev(ww), leave_one_out=True).cpu().numpy()
        want = kr.density(x, None, ww, "silverman", leave_one_out=True)
        assert float(np.max(np.abs(got - want) / want)) <= 1e-10
    dx = _dev(x)
    assert torch.equal(tension.kde_density(dx, dx, leave_one_out=True), tension.kde_density(dx, None, leave_one_out=True))
    at = x[:5].copy()
    at[1] = 1.0e4
    at[3, 0] = np.nan
    got = tension.kde_density(dx, _dev(at)).cpu().numpy()
    assert got[1] == 0.0 and np.isnan(got[3]) and np.all(got[[0, 2, 4]] > 0)


# (n, d, weighted, seed): around the slice length of the kernel, and every kind of weights; seeds checked on the CPU
SHIFT_CASES = [(257, 1, False, 1), (1025, 2, True, 1), (2051, 3, False, 1), (2051, 6, True, 1), (1500, 4, False, 2)]


@functools.lru_cache(maxsize=None)
def _shift_reference(n, d, weighted, seed):
    x, w, _ = _cloud(n, d, seed)
    w = w if weighted else None
    return x, w, kr.shift(x, w, "silverman")


@pytest.mark.parametrize("n,d,weighted,seed", SHIFT_CASES)
def test_kde_shift_is_the_restatement(tension, n, d, weighted, seed):
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type"
    x, w, ref = _shift_reference(n, d, weighted, seed)
    margin = float(np.min(np.abs(ref["ratio"] - 1)))
    print(f"n={n} d={d} weighted={weighted}: the closest sample lies {margin:.3g} from the threshold; P = {float(ref['p_exceed']):.6f}")
    assert margin >= 1e-9, "choose another seed: a sample sits on the threshold"
    assert 0 < ref["count"] < n
    r = tension.kde_shift(_dev(x), _dev(w))
    dens = r.densities.cpu().numpy()
    assert dens.shape == (n,) and r.densities.device == DEV
    assert float(np.max(np.abs(dens - ref["densities"]) / ref["densities"])) <= 1e-10
    # every sample on the restatement's side of the threshold: the cap on disagreements is zero
    np.testing.assert_array_equal(dens > r.p_zero, np.asarray(ref["ratio"] > 1))
    if weighted:
        assert r.count is None
        assert abs(r.p_exceed - float(ref["p_exceed"])) <= 1e-12 * float(ref["p_exceed"])
    else:
        assert r.count == ref["count"] and r.p_exceed == ref["count"] / n
    assert abs(r.p_zero - float(ref["p_zero"])) <= 1e-10 * float(ref["p_zero"])
    assert abs(r.p_zero_se - float(ref["p_zero_se"])) <= 1e-10 * float(ref["p_zero_se"])
    assert r.n_eff == pytest.approx(float(ref["n_eff"]), rel=1e-12)
    assert r.n_sigma == pytest.approx(ref["n_sigma"], rel=1e-9) and not r.saturated and not ref["saturated"]
    # the interval: P recomputed at p_zero -+ 2 se on the restatement's densities, widened by the binomial error in quadrature
    wn = np.full(n, 1.0 / n) if w is None else w / w.sum()
    p = float(ref["p_exceed"])
    p_lo = float((wn * np.asarray(ref["densities"] > ref["p_zero"] + 2 * ref["p_zero_se"])).sum())
    p_hi = float((wn * np.asarray(ref["densities"] > ref["p_zero"] - 2 * ref["p_zero_se"])).sum())
    b = math.sqrt(p * (1 - p) / float(ref["n_eff"]))
    assert p_lo <= p <= p_hi
    assert r.p_interval[0] == pytest.approx(max(p - math.hypot(p - p_lo, b), 0.0), abs=1e-9)
    assert r.p_interval[1] == pytest.approx(min(p + math.hypot(p_hi - p, b), 1.0), abs=1e-9)
    assert r.sigma_interval[0] <= r.n_sigma <= r.sigma_interval[1]
    assert r.sigma_interval[0] == pytest.approx(kr.sigma_of(r.p_interval[0]), rel=1e-12)


def test_kde_shift_at_another_point_and_bandwidth(tension):
    x, w, cov = _cloud(600, 2, 3)
    at = np.array([0.4, -0.2])
    for bw in ("scott", 0.4, 0.1 * cov):
        ref = kr.shift(x, w, bw, at=at)
        assert float(np.min(np.abs(ref["ratio"] - 1))) >= 1e-9
        r = tension.kde_shift(_dev(x), _dev(w), bandwidth=bw, at=_dev(at))
        assert abs(r.p_exceed - float(ref["p_exceed"])) <= 1e-12 * float(ref["p_exceed"])
        assert abs(r.p_zero - float(ref["p_zero"])) <= 1e-10 * float(ref["p_zero"])


def test_saturated_on_a_chain_twelve_sigma_from_zero(tension):
    rng = np.random.default_rng(12)
    n = 500
    x = 12.0 + rng.standard_normal((n, 1))
    ref = kr.shift(x)
    assert ref["saturated"] and ref["count"] == n
    r = tension.kde_shift(_dev(x))
    assert r.saturated and r.count == n and r.p_exceed == 1.0
    assert r.n_sigma == pytest.approx(kr.sigma_of(1.0 - 1.0 / n), rel=1e-12) and math.isfinite(r.n_sigma)
    assert r.n_sigma == pytest.approx(ref["n_sigma"], rel=1e-9)
    assert math.isfinite(r.sigma_interval[0]) and math.isfinite(r.sigma_interval[1])
    g = tension.gaussian_shift(_dev(x))
    assert g["n_sigma"] == pytest.approx(float(np.mean(x) / np.std(x, ddof=1)), rel=1e-6)  # one dimension: |mean| / sigma


def test_between_on_pairs_and_a_nested_like_run(tension):
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((400, 5)) + 1.0, 0.7 * rng.standard_normal((300, 3))
    wb = rng.uniform(0.1, 1.0, 300)
    res = tension.between((_dev(a), None), (_dev(b), _dev(wb)), [4, 0], [1, 2], n_shifts=2)
    diff, w = tension.difference_chain(torch.from_numpy(a), torch.from_numpy(b), [4, 0], [1, 2], None, torch.from_numpy(wb), n_shifts=2)
    np.testing.assert_array_equal(res["diff"].cpu().numpy(), diff.numpy())
    np.testing.assert_array_equal(res["weights"].cpu().numpy(), w.numpy())
    ref = kr.shift(diff.numpy(), w.numpy())
    assert float(np.min(np.abs(ref["ratio"] - 1))) >= 1e-9
    assert abs(res["p_exceed"] - float(ref["p_exceed"])) <= 1e-12 * float(ref["p_exceed"])
    assert res["n"] == 600 and res["d"] == 2 and res["kde"].count is None
    assert res["gaussian_n_sigma"] == pytest.approx(tension.gaussian_shift(diff, w)["n_sigma"], rel=1e-9)

    class Run:  # DeviceNestedSampler's surface
        device = DEV

        def posterior(self):
            return b, np.log(wb / wb.sum()), np.zeros(300)

    res2 = tension.between((_dev(a), None), Run(), [4, 0], [1, 2], n_shifts=2)
    assert res2["p_exceed"] == pytest.approx(res["p_exceed"], rel=1e-12)
    plain = tension.between((_dev(a), None), (_dev(b), None), [4, 0], [1, 2], n_shifts=1)
    assert plain["weights"] is None and isinstance(plain["kde"].count, int) and plain["n"] == 300


def test_the_example_runs_small_on_real_data(tension):
    spec = importlib.util.spec_from_file_location("desi_union3_tension", os.path.join(ROOT, "examples", "desi_union3_tension.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    r = ex.run(walkers=64, steps=300, burn=100, thin=10, n_shifts=1)
    a, b = r["chain_bao"], r["chain_sn"]
    assert a.shape == (64 * 20, 2) and b.shape == (64 * 20, 3) and a.is_cuda
    k, g = r["kde"], r["gaussian"]
    vals = [r["p_exceed"], r["n_sigma"], r["gaussian_n_sigma"], k.p_zero, k.p_zero_se, k.n_eff, *k.p_interval, *k.sigma_interval,
            g["chi2"], g["p_value"]]
    assert all(math.isfinite(v) for v in vals), vals
    assert 0.0 <= r["p_exceed"] <= 1.0 and r["n"] == 1280 and r["d"] == 1 and r["weights"] is None
    # the difference chain is the stated pairing of the chains it used, and p_exceed is the restatement's on it
    diff, _ = tension.difference_chain(a, b, [1], [1], n_shifts=1)
    assert torch.equal(diff, r["diff"])
    ref = kr.shift(diff.cpu().numpy())
    margin = float(np.min(np.abs(ref["ratio"] - 1)))
    print(f"example: P = {r['p_exceed']:.4f}, KDE {r['n_sigma']:.2f} sigma, Gaussian {r['gaussian_n_sigma']:.2f} sigma; closest sample "
          f"{margin:.3g} from the threshold")
    if ref["saturated"]:
        assert k.saturated and k.count == ref["count"]
    else:
        assert margin >= 1e-9, "a sample of the example's chain sits on the threshold"
        assert k.count == ref["count"] and r["p_exceed"] == ref["count"] / r["n"]
