"""GPU (-m gpu): marginals.py end to end (histograms, corner_data, weighted_mean_std) and the sampler methods built on it,
against the numpy / scipy / corner restatement of tests/marginals_reference.py."""
import numpy as np
import pytest
import torch
from scipy import stats

import marginals_reference as mr
import marginals_shapes as ms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
LEVELS = (0.393, 0.864)
QUANTILES = (0.159, 0.5, 0.841)


@pytest.fixture(scope="module")
def M(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.marginals


@pytest.fixture(scope="module")
def sample():
    """50 000 rows of a correlated 4-column Gaussian with offsets, log-normal weights; the reference parts computed once."""
    rng = np.random.default_rng(2024)
    a = rng.standard_normal((4, 4))
    cov = a @ a.T + 0.5 * np.eye(4)
    x = rng.multivariate_normal([0.3, -19.3, 70.0, 1e-3], cov * np.outer([0.02, 0.1, 1.5, 1e-4], [0.02, 0.1, 1.5, 1e-4]), 50_000)
    w = ms.lognormal_weights(len(x), 5)
    return dict(x=x, w=w, dx=torch.from_numpy(x).to(DEV), dw=torch.from_numpy(w).to(DEV))


def _check_corner_data(got, x, w, bins, r, smooth, smooth1d):
    k = x.shape[1]
    lo_hi = mr.fraction_ranges(x, r, w)
    edges = mr.edges_of(lo_hi, bins)
    np.testing.assert_array_equal(got["edges"], edges)
    pairs = [(a, b) for a in range(k) for b in range(a)]
    np.testing.assert_array_equal(got["pairs"], np.array(pairs).reshape(-1, 2))
    if w is None:
        np.testing.assert_array_equal(got["h1"], mr.hist1(x, lo_hi, bins))
        np.testing.assert_array_equal(got["h2"], mr.hist2(x, lo_hi, bins, pairs))
    else:
        idx = mr.bin_indices(x, edges)
        r1, c1, r2, c2 = mr.weighted_hists(idx, w, bins, pairs)
        for g, ref, cnt in ((got["h1"], r1, c1), (got["h2"], r2, c2)):
            assert np.all(np.abs(g.astype(LD) - ref) <= mr.fixed_point_bound(cnt, ref, w.max(), len(x)))
            assert np.all(g[cnt == 0] == 0.0)
    # the host half, given the histograms: scipy's filter within 1e-14 (derived in tests/test_marginals_cpu.py), corner's V
    for name, sigma in (("h1", smooth1d), ("h2", smooth)):
        for h, hs in zip(got[name], got[name + "_smooth"]):
            want = h if sigma is None else mr.smooth(h, sigma)
            assert np.all(np.abs(hs - want) <= 1e-14 * np.abs(want))
    assert got["V"].shape == (len(pairs), len(LEVELS))
    for p in range(len(pairs)):
        np.testing.assert_array_equal(got["V"][p], mr.levels_of(got["h2_smooth"][p], LEVELS))
    want_q = np.stack([mr.quantile(x[:, c], QUANTILES, w) for c in range(k)], axis=1)
    np.testing.assert_array_equal(got["quantiles"], want_q)


@pytest.mark.parametrize("weighted", [False, True])
def test_corner_data_against_the_restatement(M, sample, weighted):
    x, w = sample["x"], sample["w"] if weighted else None
    got = M.corner_data(sample["dx"], weights=sample["dw"] if weighted else None)  # the reference's corner_plot.py arguments
    assert got["h2"].shape == (6, 100, 100) and got["h1"].shape == (4, 100)
    _check_corner_data(got, x, w, 100, 0.9999, 2.0, 2.0)
    got = M.corner_data(sample["dx"], bins=37, range=0.95, smooth=None, smooth1d=1.0, weights=sample["dw"] if weighted else None)
    _check_corner_data(got, x, w, 37, 0.95, None, 1.0)
    np.testing.assert_array_equal(got["h2"], got["h2_smooth"])


@pytest.mark.parametrize("weighted", [False, True])
def test_histograms_with_explicit_ranges_and_pairs(M, sample, weighted):
    x = sample["x"]
    lo_hi = np.stack([np.percentile(x, 5, axis=0), np.percentile(x, 95, axis=0)], axis=1)  # about 10 % of the rows outside
    pairs = [(0, 3), (3, 0), (2, 1)]
    rng = [tuple(lo_hi[0]), 0.9, tuple(lo_hi[2]), 0.5]  # corner's mixture: a (lo, hi) or a fraction per column
    dw, w = (sample["dw"], sample["w"]) if weighted else (None, None)
    edges, h1, h2, pr = M.histograms(sample["dx"], bins=128, range=rng, weights=dw, pairs=pairs)
    fr = {c: mr.quantile(x[:, c], [0.5 - 0.5 * r, 0.5 + 0.5 * r], w) for c, r in ((1, 0.9), (3, 0.5))}
    want_lo_hi = np.stack([lo_hi[0], fr[1], lo_hi[2], fr[3]])
    np.testing.assert_array_equal(edges, mr.edges_of(want_lo_hi, 128))
    np.testing.assert_array_equal(pr, pairs)
    assert h1.device == sample["dx"].device and h2.shape == (3, 128, 128)
    if not weighted:
        assert h1.dtype == torch.int64
        np.testing.assert_array_equal(h1.cpu().numpy(), mr.hist1(x, want_lo_hi, 128))
        np.testing.assert_array_equal(h2.cpu().numpy(), mr.hist2(x, want_lo_hi, 128, pairs))
    else:
        assert h1.dtype == torch.float64
        r1, c1, r2, c2 = mr.weighted_hists(mr.bin_indices(x, edges), w, 128, pairs)
        for g, ref, cnt in ((h1.cpu().numpy(), r1, c1), (h2.cpu().numpy(), r2, c2)):
            assert np.all(np.abs(g.astype(LD) - ref) <= mr.fixed_point_bound(cnt, ref, w.max(), len(x)))
    np.testing.assert_array_equal(h2[1].cpu().numpy(), h2[0].cpu().numpy().T)
    for nseg in (1, 7):  # the launch geometry never changes a bit
        _, g1, g2, _ = M.histograms(sample["dx"], bins=128, range=rng, weights=dw, pairs=pairs, n_segments=nseg)
        assert torch.equal(g1, h1) and torch.equal(g2, h2)
    # no range: (min, max) of every column, every row counted
    edges, h1, _, _ = M.histograms(sample["dx"], bins=10)
    np.testing.assert_array_equal(edges, mr.edges_of(np.stack([x.min(axis=0), x.max(axis=0)], axis=1), 10))
    assert h1.sum(dim=1).tolist() == [len(x)] * 4


def test_weighted_mean_and_std(M, sample):
    """Relative 1e-13 against long double: the sums have 50 000 terms of one sign (mean: offsets far from 0; variance:
    squares), so pairwise device sums lose a few ulp of 1.1e-16 each."""
    mean, std = M.weighted_mean_std(sample["dx"], sample["dw"])
    assert mean.device == sample["dx"].device and mean.shape == std.shape == (4,)
    rm, rs = mr.weighted_mean_std(sample["x"], sample["w"])
    assert np.all(np.abs(mean.cpu().numpy().astype(LD) - rm) <= 1e-13 * np.abs(rm))
    assert np.all(np.abs(std.cpu().numpy().astype(LD) - rs) <= 1e-13 * np.abs(rs))


def test_a_strided_view_equals_its_contiguous_copy(M, sample):
    chain = sample["dx"][:48_000].reshape(300, 160, 4)
    views = [chain[20::3].flatten(0, 1),                                                       # discard 20, thin 3
             torch.cat([sample["dx"], sample["dx"]], dim=1)[:, 2:6],                                 # columns of a wider tensor
             sample["dx"][::2]]                                                                     # every other row
    assert not views[1].is_contiguous() and not views[2].is_contiguous()
    for v in views:
        a, b = M.corner_data(v), M.corner_data(v.contiguous().clone())
        assert set(a) == set(b)
        for key in a:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    w = sample["dw"][::2]
    a, b = M.corner_data(views[2], weights=w), M.corner_data(views[2].contiguous(), weights=w.contiguous())
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_ensemble_marginals_and_mean_path(pkg, M):
    E = pkg.ensemble
    mu = torch.tensor([0.3, -19.3, 70.0], dtype=torch.float64, device=DEV)
    sd = torch.tensor([0.02, 0.1, 1.5], dtype=torch.float64, device=DEV)

    def log_prob(theta):
        return -0.5 * (((theta - mu) / sd) ** 2).sum(dim=1)

    start = mu + sd * torch.from_numpy(np.random.default_rng(1).standard_normal((64, 3))).to(DEV)
    ens = E.ShardedEnsemble(log_prob, start, seed=3)
    ens.run_mcmc(60)
    chain = ens.get_chain()
    assert chain.shape == (60, 64, 3)
    got = ens.marginals(discard=10, thin=2, bins=20)
    flat = ens.get_chain(discard=10, thin=2, flat=True)
    assert flat.shape == (25 * 64, 3)
    want = M.corner_data(flat, bins=20)
    assert set(got) == set(want)
    for key in got:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    _check_corner_data(got, flat.cpu().numpy(), None, 20, 0.9999, 2.0, 2.0)
    assert torch.equal(ens.mean_path(), chain.mean(dim=1)) and ens.mean_path().shape == (60, 3)
    assert torch.equal(ens.mean_path(discard=15), chain[15:].mean(dim=1))
    np.testing.assert_allclose(ens.mean_path().cpu().numpy(), chain.cpu().numpy().mean(axis=1), rtol=1e-14)


def test_nested_sampler_marginals_and_mean_std(pkg, M):
    nested = pkg.nested
    mu, cov = np.array([0.3, 0.6]), np.array([[0.01, 0.003], [0.003, 0.02]])
    mu_t = torch.tensor(mu, dtype=torch.float64, device=DEV)
    prec = torch.tensor(np.linalg.inv(cov), dtype=torch.float64, device=DEV)

    def loglike(theta):
        d = theta - mu_t
        return -0.5 * ((d @ prec) * d).sum(1)

    p = nested.Prior()
    p.add_parameter("a", dist=(0.0, 1.0))
    p.add_parameter("b", dist=stats.norm(0.5, 0.2))
    s = nested.DeviceNestedSampler(p, loglike, n_live=400, seed=7)
    assert s.run() is True
    pts, log_w, _ = s.posterior()
    w = np.exp(log_w)
    got = s.marginals(bins=30)
    _check_corner_data(got, pts, w, 30, 0.9999, 2.0, 2.0)
    mean, std = s.mean_std()
    assert mean.is_cuda and std.is_cuda
    rm, rs = mr.weighted_mean_std(pts, w)
    assert np.all(np.abs(mean.cpu().numpy().astype(LD) - rm) <= 1e-13 * np.abs(rm))
    assert np.all(np.abs(std.cpu().numpy().astype(LD) - rs) <= 1e-13 * np.abs(rs))


def test_one_column_has_no_pairs(M, sample):
    got = M.corner_data(sample["dx"][:, 2:3], bins=50)
    assert got["h2"].shape == got["h2_smooth"].shape == (0, 50, 50) and got["V"].shape == (0, 2) and got["pairs"].shape == (0, 2)
    _check_corner_data(got, sample["x"][:, 2:3], None, 50, 0.9999, 2.0, 2.0)
