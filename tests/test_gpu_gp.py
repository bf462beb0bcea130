"""GPU (-m gpu): ``gp.HubbleGP`` on the real cosmic-chronometer data (tests/golden/ohd_cc.npz, n = 38), end to end: the
type-II maximum through ``optimize.best_fit``, a 64-walker ``ShardedEnsemble`` chain on ``torch_log_prob``, and the bands
marginalised over that chain.  The judge is the long-double restatement (tests/gp_reference.py) and scipy's L-BFGS-B
maximum of it in the same box.  Bars: tests/test_gpu_gp_kernels.py's."""
import numpy as np
import pytest
import torch

import gp_reference as R
import gp_shapes as GS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = R.LD
BAR = 1e-10
N = 38


@pytest.fixture(scope="module")
def hgp(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    g = pkg.gp.HubbleGP(*GS.raw_data(N))
    yield g
    g.close()


@pytest.fixture(scope="module")
def scipy_max():
    """The maximum of the restatement in the default box: (x, log ML in normalised units), the better of two starts."""
    from scipy.optimize import minimize

    z, y, Cm, b = GS.data(N)[:4]
    f = lambda t: -float(R.mll(z, y, Cm, t))
    runs = [minimize(f, x0, method="L-BFGS-B", bounds=b, options=dict(ftol=1e-15, gtol=1e-9, maxiter=500))
            for x0 in (b.mean(axis=1), np.array([1.0, 5.0, 1.2 * b[2, 0], 0.5]))]
    best = min(runs, key=lambda r: r.fun)
    return best.x, -best.fun


@pytest.fixture(scope="module")
def fit(hgp):
    return hgp.fit(n_starts=32, seed=0)


@pytest.fixture(scope="module")
def chain(pkg, hgp, fit):
    """64 walkers, 300 steps, started in a tenth of the box around the fit."""
    b = hgp.bounds
    w = b[:, 1] - b[:, 0]
    lo, hi = np.maximum(b[:, 0] + 1e-3 * w, fit.x - 0.1 * w), np.minimum(b[:, 1] - 1e-3 * w, fit.x + 0.1 * w)
    start = lo + np.random.default_rng(11).uniform(0.0, 1.0, (64, 4)) * (hi - lo)
    ens = pkg.ensemble.ShardedEnsemble(hgp.torch_log_prob(), torch.from_numpy(start).to(DEV), seed=5)
    ens.run_mcmc(300)
    return ens


def test_fit_reaches_the_maximum_scipy_finds(hgp, fit, scipy_max):
    x_ref, f_ref = scipy_max
    got = fit.log_prob + hgp.log_norm  # normalised units
    b = hgp.bounds
    print(f"fit: x = {fit.x}, log ML = {got:.10f} (scipy {f_ref:.10f} at {x_ref}), converged = {fit.best_converged}, "
          f"physical = {hgp.physical(fit.x)}, iterations = {fit.problems.iterations}, likelihood rows = {fit.problems.n_like}")
    assert x_ref[2] == b[2, 0], "scipy's maximum is expected on the lower bound of the length scale"
    assert fit.best_converged
    assert abs(got - f_ref) < 1e-6
    assert 0.0 <= (fit.x[2] - b[2, 0]) / (b[2, 1] - b[2, 0]) < 1e-6
    assert abs(fit.x[3] - x_ref[3]) < 1e-3 * x_ref[3]
    # the value the optimizer reports is the restatement's at that point
    z, y, Cm = GS.data(N)[:3]
    assert abs(got - float(R.mll(z, y, Cm, fit.x))) < BAR * abs(f_ref)
    assert hgp.log_marginal_likelihood(fit.x) == pytest.approx(fit.log_prob, rel=1e-15)


def test_h0_at_the_fit_is_the_restatements(hgp, fit):
    z, y, Cm = GS.data(N)[:3]
    zs = np.array([0.0, 0.5, float(z.max())])
    got = hgp.predict(fit.x, zs, noise=GS.TEST_NOISE)
    ref = R.predict(z, y, Cm, fit.x, zs, GS.TEST_NOISE)
    raw = hgp.predict_normalised(fit.x, zs, noise=GS.TEST_NOISE)[0]
    err = R.scaled_errors(raw, ref, fit.x).astype(np.float64)
    print(f"H0 = {got['mean'][0]:.3f} +- {got['std'][0]:.3f} km/s/Mpc, q0 = {got['q'][0]:.4f}; max scaled err {err.max():.2e}")
    assert err.max() < BAR
    s, mu = LD(hgp.h_std), LD(hgp.h_mean)
    assert abs(LD(got["mean"][0]) - (ref[0, 0] * s + mu)) < BAR * abs(ref[0, 0] * s + mu)
    assert abs(LD(got["std"][0]) - np.sqrt(ref[0, 1]) * s) < 1e-9 * np.sqrt(ref[0, 1]) * s
    assert np.allclose(got["q"], -1 + (1 + zs) * got["dmean"] / got["mean"], rtol=1e-15)


def test_chain_stays_in_the_box_moves_and_replays_bit_for_bit(hgp, chain):
    x = chain.get_chain(flat=True)
    lp = chain.get_log_prob(flat=True)
    assert x.shape == (300 * 64, 4) and lp.shape == (300 * 64,)
    xs, lps = x.cpu().numpy(), lp.cpu().numpy()
    b = hgp.bounds
    assert np.isfinite(lps).all() and (xs > b[:, 0]).all() and (xs < b[:, 1]).all()
    acc = chain.acceptance_fraction()
    print(f"chain: acceptance fraction {acc:.3f}, mean theta {xs[64 * 100:].mean(axis=0)}")
    assert 0.1 < acc < 0.9
    replay = hgp.log_marginal_likelihood(np.ascontiguousarray(xs))
    assert np.array_equal(replay.view(np.int64), np.ascontiguousarray(lps).view(np.int64))
    assert hgp.info()["failed_factorizations"] == 0


@pytest.mark.parametrize("weighted", (False, True))
def test_marginal_band_is_the_restatements_mixture(hgp, chain, weighted):
    z, y, Cm = GS.data(N)[:3]
    samples = chain.get_chain(flat=True)[-256:].contiguous()  # the last four steps of all walkers
    th = samples.cpu().numpy()
    zs = np.concatenate([[0.0, float(z[3]), -0.05, float(z.max()) + 0.2], np.linspace(0.1, 1.9, 8)])
    w = np.random.default_rng(2).uniform(0.0, 1.0, 256) if weighted else None
    got = hgp.marginal_predict(samples, zs, weights=None if w is None else torch.from_numpy(w).to(DEV), noise=GS.TEST_NOISE,
                               max_bytes=100 * zs.size * 40)  # three chunks
    ref = R.mixture(np.array([R.predict(z, y, Cm, t, zs, GS.TEST_NOISE) for t in th]), w)
    s, mu = LD(hgp.h_std), LD(hgp.h_mean)
    sf2, ell = th[:, 1].astype(LD), th[:, 2].astype(LD)
    # the smallest scale any sample has: the strictest reading of the per-row bars
    scales = [np.max(np.abs(ref[:, 0] * s + mu)), np.min(sf2) * s * s, np.max(np.abs(ref[:, 2])) * s, np.min(sf2 / ell**2) * s * s,
              np.min(sf2 / ell) * s * s]
    pairs = [(got["mean"], ref[:, 0] * s + mu), (got["std"] ** 2, ref[:, 1] * s * s), (got["dmean"], ref[:, 2] * s),
             (got["dstd"] ** 2, ref[:, 3] * s * s), (got["cov_fd"], ref[:, 4] * s * s)]
    errs = [float(np.max(np.abs(np.asarray(a, dtype=LD) - r)) / sc) for (a, r), sc in zip(pairs, scales)]
    print(f"marginal band (weighted={weighted}): scaled errs {['%.1e' % e for e in errs]}; H0 = {got['H0'][0]:.3f} +- {got['H0'][1]:.3f}")
    assert max(errs) < BAR
    assert got["H0"] == (got["mean"][0], got["std"][0])
    assert np.allclose(got["q"], -1 + (1 + zs) * got["dmean"] / got["mean"], rtol=1e-15)


def test_log_prob_callable_outlives_its_maker_and_refuses_a_closed_gp(pkg):
    import gc

    def make():
        g = pkg.gp.HubbleGP(*GS.raw_data(N))
        return g.torch_log_prob(), g

    f, g = make()
    th = torch.from_numpy(GS.thetas(N, 5)).to(DEV)
    want = g.log_marginal_likelihood(GS.thetas(N, 5))
    del g
    gc.collect()
    assert np.array_equal(f(th).cpu().numpy().view(np.int64), want.view(np.int64))  # the callable alone keeps the GP alive
    with pytest.raises(ValueError, match="on the GP's GPU"):
        f(th.cpu())
    keep = pkg.gp.HubbleGP(*GS.raw_data(N))
    f2 = keep.torch_log_prob()
    keep.close()
    with pytest.raises(pkg.CosmofitError, match="has been closed"):
        f2(th)
    with pytest.raises(pkg.CosmofitError, match="has been closed"):
        keep.marginal_predict(th, [0.0])
