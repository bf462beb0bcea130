"""CPU: the tension module's definitions, without a GPU.

* tests/kde_reference.py (the long-double restatement that judges the device code) equals scipy.stats.gaussian_kde.
* The parameter-shift estimator itself is sane: on Gaussian difference chains its leave-one-out estimate lies near the closed
  form, and including the self term is worse.
* difference_chain equals a numpy loop; gaussian_shift, goodness_of_fit_loss and suspiciousness equal their closed forms.
* Every validation error is raised before a device is asked for.

The scatter of the estimator (n = 4096, Silverman bandwidth, exact leave-one-out; RMS deviation of p_exceed from chi^2_d's CDF
at k^2 over 20 seeds [100 .. 119, d, k] of kde_reference.gaussian_chain, measured with the restatement in float64 on the CPU):

    d \\ k        1         2         3
    1        0.0177    0.0048    0.00083
    2        0.0338    0.0174    0.0037
    4        0.0371    0.0603    0.0278

(the issue's 10-seed values for comparison: (1, 2) 0.004, (2, 2) 0.015, (4, 2) 0.046, (4, 3) 0.027).  With the self term
included the same 20 seeds give at d = 4: RMS 0.0436 / 0.0849 / 0.0557 with a mean bias of +0.020 / +0.057 / +0.054.  The test
holds each of 5 fresh seeds [0 .. 4, d, k] within 5 x that RMS."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import stats

import kde_reference as kr

LD = np.longdouble
N_SANITY = 4096
RMS = {(1, 1): 0.0177, (1, 2): 0.0048, (1, 3): 0.00083,
       (2, 1): 0.0338, (2, 2): 0.0174, (2, 3): 0.0037,
       (4, 1): 0.0371, (4, 2): 0.0603, (4, 3): 0.0278}
FRESH_SEEDS = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def tension(pkg):
    return pkg.tension


# ---- the restatement is scipy's gaussian_kde --------------------------------------------------------------------------
def _kde_case(d, seed):
    """Samples of a well-conditioned covariance (scipy whitens in float64: its own error grows with the condition number and
    with the exponent, so the comparison at 1e-12 uses cond < 10 and evaluation points inside the cloud)."""
    rng = np.random.default_rng([seed, d])
    n = 300
    a = rng.standard_normal((d, d))
    q, _ = np.linalg.qr(a)
    cov = q @ np.diag(np.linspace(1.0, 3.0, d)) @ q.T
    x = rng.standard_normal((n, d)) @ np.linalg.cholesky(cov).T + rng.standard_normal(d)
    at = x[:40] + 0.1 * rng.standard_normal((40, d))
    w = rng.uniform(0.1, 1.0, n)
    return x, at, w, 0.3 * cov


@pytest.mark.parametrize("d", [1, 2, 6])
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_is_scipys_gaussian_kde(d, weighted):
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type"
    x, at, w, H = _kde_case(d, 1)
    w = w if weighted else None
    for bw in ("scott", "silverman", 0.37, H):
        ref = kr.density(x, at, w, bw)
        sc = kr.scipy_kde(x, w, bw)(at.T)
        rel = float(np.max(np.abs(ref - sc) / sc))
        print(f"d={d} weighted={weighted} bandwidth={bw if not isinstance(bw, np.ndarray) else 'matrix'}: {rel:.3g}")
        assert rel <= 1e-12
    s = kr.setup(x, w, "silverman")
    k = kr.scipy_kde(x, w, "silverman")
    assert float(s["neff"]) == pytest.approx(k.neff, rel=1e-13) and np.allclose(np.asarray(s["cov"], dtype=float), k.covariance,
                                                                                 rtol=1e-12, atol=0)


def test_leave_one_out_restatement_is_a_kde_of_the_other_samples():
    """Row i of the leave-one-out density = scipy's KDE built from the other samples with the covariance of all."""
    x, _, w, _ = _kde_case(2, 2)
    x, w = x[:40], w[:40]
    s = kr.setup(x, w, "silverman")
    H = np.asarray(s["cov"], dtype=np.float64)
    loo = kr.density(x, None, w, "silverman", leave_one_out=True)
    for i in (0, 17, 39):
        keep = np.arange(40) != i
        sc = kr.scipy_kde(x[keep], w[keep], H)(x[i:i + 1].T)[0]
        assert float(loo[i]) == pytest.approx(sc, rel=1e-12)


# ---- the estimator against the closed form ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sanity_runs():
    """p_exceed of the restatement (float64: the scatter is 1e-2, the arithmetic 1e-15) for the fresh seeds, once."""
    out = {}
    for d, k in RMS:
        for s in FRESH_SEEDS:
            x = kr.gaussian_chain(N_SANITY, d, k, [s, d, k])
            out[d, k, s] = float(kr.shift(x, dtype=np.float64)["p_exceed"])
            if d == 4 and k >= 2:
                out[d, k, s, "self"] = float(kr.shift(x, dtype=np.float64, leave_one_out=False)["p_exceed"])
    return out


@pytest.mark.parametrize("d,k", sorted(RMS))
def test_leave_one_out_estimate_lies_near_the_closed_form(sanity_runs, d, k):
    exact = stats.chi2.cdf(k * k, d)
    for s in FRESH_SEEDS:
        dev = sanity_runs[d, k, s] - exact
        print(f"d={d} k={k} seed={s}: p_exceed {sanity_runs[d, k, s]:.4f} exact {exact:.4f} deviation {dev / RMS[d, k]:+.2f} RMS")
        assert abs(dev) <= 5.0 * RMS[d, k]


def test_including_the_self_term_is_worse_at_d4(sanity_runs):
    """What pins exact leave-one-out: over the ten fresh chains at d = 4, k = 2 and 3, the estimate with the self term is
    further from the closed form (and biased high in every one of them)."""
    loo, with_self = [], []
    for k in (2, 3):
        exact = stats.chi2.cdf(k * k, 4)
        for s in FRESH_SEEDS:
            loo.append(sanity_runs[4, k, s] - exact)
            with_self.append(sanity_runs[4, k, s, "self"] - exact)
            assert sanity_runs[4, k, s, "self"] > sanity_runs[4, k, s]
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    print(f"d=4: RMS deviation leave-one-out {rms(loo):.4f}, with the self term {rms(with_self):.4f}, mean {np.mean(with_self):+.4f}")
    assert rms(with_self) > rms(loo) and np.mean(with_self) > 0


# ---- difference_chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a,n_b,n_shifts", [(50, 50, 4), (37, 101, 3), (101, 37, 1), (5, 9, 5)])
def test_difference_chain_is_the_numpy_loop(tension, n_a, n_b, n_shifts):
    rng = np.random.default_rng(n_a + n_b)
    a, b = rng.standard_normal((n_a, 12)), rng.standard_normal((n_b, 4))
    wa, wb = rng.uniform(0, 1, n_a), rng.uniform(0, 1, n_b)
    ca, cb = [10, 0, 3], [1, -1, 2]
    m = min(n_a, n_b)
    offs = tension.shift_offsets(m, n_shifts)
    assert offs == [((2 * s + 1) * m) // (2 * n_shifts) for s in range(n_shifts)] and len(set(offs)) == n_shifts
    want = np.empty((n_shifts * m, 3))
    want_w = np.empty((3, n_shifts * m))
    for s in range(n_shifts):
        for i in range(m):
            j = (i + offs[s]) % n_b
            want[s * m + i] = a[i, ca] - b[j, cb]
            want_w[:, s * m + i] = wa[i] * wb[j], wa[i], wb[j]
    t = torch.from_numpy
    for k, (xa, xb) in enumerate(((wa, wb), (wa, None), (None, wb), (None, None))):
        diff, w = tension.difference_chain(t(a), t(b), ca, cb, None if xa is None else t(xa), None if xb is None else t(xb),
                                           n_shifts=n_shifts)
        assert diff.dtype == torch.float64 and diff.is_contiguous() and w.shape == (n_shifts * m,)
        np.testing.assert_array_equal(diff.numpy(), want)
        np.testing.assert_array_equal(w.numpy(), want_w[k] if k < 3 else np.ones(n_shifts * m))
    full, _ = tension.difference_chain(t(a[:, :4]), t(b), n_shifts=1)
    np.testing.assert_array_equal(full.numpy(), a[:m, :4] - b[(np.arange(m) + tension.shift_offsets(m, 1)[0]) % n_b])


# ---- closed forms -----------------------------------------------------------------------------------------------------
def test_gaussian_shift_closed_form(tension):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((500, 3)) @ np.array([[1.0, 0.2, 0.0], [0.0, 0.7, 0.1], [0.0, 0.0, 1.5]]) + np.array([0.5, -1.0, 2.0])
    w = rng.uniform(0.2, 1.0, 500)
    for ww in (None, w):
        r = tension.gaussian_shift(torch.from_numpy(x), None if ww is None else torch.from_numpy(ww))
        mean = np.average(x, axis=0, weights=ww)
        cov = np.cov(x.T, aweights=ww, bias=False)
        chi2 = float(mean @ np.linalg.solve(cov, mean))
        assert r["chi2"] == pytest.approx(chi2, rel=1e-12) and r["dof"] == 3
        assert r["p_value"] == pytest.approx(stats.chi2.sf(chi2, 3), rel=1e-10)
        assert r["n_sigma"] == pytest.approx(stats.norm.isf(0.5 * stats.chi2.sf(chi2, 3)), rel=1e-10)
        np.testing.assert_allclose(r["mean"], mean, rtol=1e-13)
        np.testing.assert_allclose(r["cov"], cov, rtol=1e-12)
    # one dimension, mean exactly k sigma away: k sigma
    y = np.array([1.0, 3.0, 1.0, 3.0])  # mean 2, variance 4/3
    r = tension.gaussian_shift(torch.from_numpy(y.reshape(-1, 1)))
    assert r["chi2"] == pytest.approx(3.0, rel=1e-14) and r["n_sigma"] == pytest.approx(np.sqrt(3.0), rel=1e-10)


def test_goodness_of_fit_loss_closed_form(tension, pkg):
    r = tension.goodness_of_fit_loss(10.0, 12.5, 31.5, 1)
    assert r["q_dmap"] == 9.0 and r["n_sigma"] == pytest.approx(3.0) and r["p_value"] == pytest.approx(stats.chi2.sf(9.0, 1))
    r = tension.goodness_of_fit_loss(10.0, 12.0, 30.0, 2)
    assert r["q_dmap"] == 8.0 and r["p_value"] == pytest.approx(np.exp(-4.0), rel=1e-12)  # chi^2_2's tail is exp(-Q / 2)
    assert r["n_sigma"] == pytest.approx(pkg.optimize.sigma_from_delta_chi2(8.0, 2))

    class Fit:  # what optimize.best_fit returns carries .chi2
        def __init__(self, chi2):
            self.chi2 = chi2

    assert tension.goodness_of_fit_loss(Fit(10.0), Fit(12.0), Fit(30.0), 2) == r
    r = tension.goodness_of_fit_loss(10.0, 12.0, 21.0, 3)  # the joint fit lost nothing
    assert r["q_dmap"] == -1.0 and r["p_value"] == 1.0 and r["n_sigma"] == 0.0
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="dof"):
            tension.goodness_of_fit_loss(1.0, 1.0, 3.0, bad)
    with pytest.raises(ValueError, match="finite"):
        tension.goodness_of_fit_loss(float("nan"), 1.0, 3.0, 1)


def test_suspiciousness_closed_form(tension):
    """Hand-made runs: two equally weighted log L values L0 +- s have posterior variance s^2, so d = 2 s^2 per run."""
    def run(log_z, info, s):
        return (log_z, info, np.array([-5.0 - s, -5.0 + s]), np.array([0.5, 0.5]))

    a, b, j = run(-10.0, 2.0, 1.0), run(-12.0, 3.0, np.sqrt(1.5)), run(-25.0, 4.5, 1.0)
    r = tension.suspiciousness(a, b, j)
    assert r["log_r"] == pytest.approx(-3.0) and r["log_i"] == pytest.approx(0.5) and r["log_s"] == pytest.approx(-3.5)
    assert (r["d_a"], r["d_b"], r["d_joint"]) == pytest.approx((2.0, 3.0, 2.0)) and r["d"] == pytest.approx(3.0)
    p = stats.chi2.sf(3.0 + 7.0, 3.0)
    assert r["p_value"] == pytest.approx(p, rel=1e-12) and r["n_sigma"] == pytest.approx(stats.norm.isf(0.5 * p), rel=1e-12)
    # unequal weights: the weighted variance
    w = np.array([1.0, 3.0])
    ll = np.array([-1.0, -3.0])
    r2 = tension.suspiciousness((-10.0, 2.0, ll, w), b, j)
    assert r2["d_a"] == pytest.approx(2.0 * (0.25 * 1.5**2 + 0.75 * 0.5**2))

    class Run:  # the DeviceNestedSampler surface: posterior() -> (points, log_w, log_l), log_z, information
        log_z, information = -10.0, 2.0

        def posterior(self):
            return np.zeros((2, 1)), np.log([0.5, 0.5]), np.array([-6.0, -4.0])

    assert tension.suspiciousness(Run(), b, j) == pytest.approx(r)
    assert np.isnan(tension.suspiciousness(a, a, run(-25.0, 4.5, 2.0))["p_value"])  # d = 2 + 2 - 8 < 0
    for bad in ((1.0, 2.0, ll), "run", (1.0, 2.0, ll, w[:1]), (float("inf"), 2.0, ll, w), (1.0, 2.0, ll, -w)):
        with pytest.raises(ValueError):
            tension.suspiciousness(bad, b, j)


# ---- validation: the same message with and without a GPU --------------------------------------------------------------
def test_validation_errors_need_no_gpu(tension):
    t = torch.from_numpy
    rng = np.random.default_rng(0)
    x = t(rng.standard_normal((50, 3)))
    w = t(rng.uniform(0.1, 1.0, 50))
    nan_x, inf_x = x.clone(), x.clone()
    nan_x[3, 1], inf_x[4, 0] = float("nan"), float("inf")
    for fn in (tension.kde_shift, tension.gaussian_shift, lambda s, weights=None: tension.kde_density(s, x, weights)):
        for bad in (x.numpy(), x.to(torch.float32), x[:, 0], x[:0], t(rng.standard_normal((50, 9))), x[:3], nan_x, inf_x):
            with pytest.raises(ValueError):
                fn(bad)
        neg, zero, nan_w = w.clone(), torch.zeros_like(w), w.clone()
        neg[2], nan_w[5] = -0.1, float("nan")
        for bad in (w.numpy(), w[:10], w.to(torch.float32), neg, zero, nan_w, w.reshape(-1, 1)):
            with pytest.raises(ValueError, match="weights"):
                fn(x, weights=bad)
    for bad in ("botev", 0.0, -1.0, float("nan"), float("inf"), True, np.eye(2), -np.eye(3), np.array([[1.0, 0.5, 0], [0, 1, 0], [0, 0, 1]])):
        with pytest.raises(ValueError, match="bandwidth"):
            tension.kde_shift(x, bandwidth=bad)
        with pytest.raises(ValueError, match="bandwidth"):
            tension.kde_density(x, x, bandwidth=bad)
    for bad in (np.zeros(2), [0.0, float("nan"), 0.0]):
        with pytest.raises(ValueError, match="at"):
            tension.kde_shift(x, at=bad)
    for bad in (None, x.numpy(), x[:, :2], x.to(torch.float32), x[:0]):
        with pytest.raises(ValueError, match="evaluation points"):
            tension.kde_density(x, bad)
    with pytest.raises(ValueError, match="leave_one_out"):
        tension.kde_density(x, x.clone(), leave_one_out=True)
    # difference_chain
    with pytest.raises(ValueError, match="same number"):
        tension.difference_chain(x, x, [0, 1], [0])
    with pytest.raises(ValueError, match="out of range"):
        tension.difference_chain(x, x, [3], [0])
    for bad in (0, 51, 2.0, True):
        with pytest.raises(ValueError, match="n_shifts"):
            tension.difference_chain(x, x, n_shifts=bad)
    with pytest.raises(ValueError, match="finite"):
        tension.difference_chain(nan_x, x)
    with pytest.raises(ValueError, match="weights"):
        tension.difference_chain(x, x, weights_b=w[:10])
    with pytest.raises(TypeError, match="unexpected keyword"):
        tension.between((x, None), (x, None), [0], [0], bins=3)
    with pytest.raises(ValueError, match="ShardedEnsemble"):
        tension.between(x, (x, None), [0], [0])
    # valid arguments: only now the device is asked for, and a CPU tensor is refused without a fallback
    for call in (lambda: tension.kde_shift(x, w), lambda: tension.kde_density(x, x), lambda: tension.kde_density(x, None, leave_one_out=True),
                 lambda: tension.between((x, None), (x, w), [0, 1], [2, 0])):
        with pytest.raises(ValueError, match="MI355X"):
            call()


def test_kernel_entry_validates_before_launching(pkg):
    """cf_kde_sum_device: every argument error is CF_ERR_INVALID with a message, before anything is launched (so this needs no
    GPU; the pointers are never followed)."""
    lib, L = pkg.lib(), pkg._lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    n, m = 8, 4
    ok = dict(y=p, w=None, n=n, d=2, q=p, m=m, off=-1, out=p, sq=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cf_kde_sum_device(a["y"], a["w"], a["n"], a["d"], a["q"], a["m"], a["off"], a["out"], a["sq"], None)

    for kw, word in ((dict(d=0), "ndim"), (dict(d=9), "ndim"), (dict(n=0), "n >= 1"), (dict(m=0), "m >= 1"), (dict(m=-3), "m >= 1"),
                     (dict(y=None), "null"), (dict(q=None), "null"), (dict(out=None), "null"), (dict(off=5), "self_offset"),
                     (dict(off=8), "self_offset"), (dict(off=-2), "self_offset")):
        assert call(**kw) == -1, kw
        with pytest.raises(L.CosmofitError, match="CF_ERR_INVALID.*cf_kde_sum_device.*" + word):
            L.check(call(**kw))
    assert (L.CF_KDE_MAX_NDIM, L.CF_KDE_TILE, L.CF_KDE_SLICE) == (8, 256, 2048)
