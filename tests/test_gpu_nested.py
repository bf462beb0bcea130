"""GPU (-m gpu): the device-resident nested sampler (nested.py, csrc/cosmofit_nested.hip).

* The kernels against the numpy restatement (tests/nested_reference.py): the prior draw, the transform (Phi^-1 against
  scipy.special.ndtri) and one full iteration -- bit for bit on uniform priors, within 1e-13 with normal dimensions -- with
  the walk counters.
* Evidence against closed forms: a correlated 5-D Gaussian in a box, normal priors times a Gaussian likelihood, two
  separated modes; a 10-seed calibration of log Z against its stated error.
* sn/union3_1.py on the real-data fixture through the engine against a trapezoid quadrature of the same GPU log-likelihood,
  and against the reference's published log Z.
* Determinism: the same seed gives the same bits.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy import special, stats

import nested_reference as ref
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def nested(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.nested


def _gauss(mu, cov):
    """torch log-density of N(mu, cov) on the rows of theta."""
    mu_t = torch.tensor(mu, dtype=torch.float64, device=DEV)
    prec = torch.tensor(np.linalg.inv(cov), dtype=torch.float64, device=DEV)
    c = -0.5 * np.linalg.slogdet(2 * np.pi * np.asarray(cov))[1]

    def f(theta):
        x = theta - mu_t
        return -0.5 * ((x @ prec) * x).sum(1) + c

    return f


def _weighted_moments(points, log_w):
    w = np.exp(log_w)
    mean = w @ points / w.sum()
    x = points - mean
    return mean, (w[:, None] * x).T @ x / w.sum()


# ---- 1. kernels against the restatement ------------------------------------------------------------------------------
def test_transform_and_prior_draw_against_the_restatement(pkg, nested):
    L = pkg._lib
    p = nested.Prior()
    p.add_parameter("a", dist=(-1, 1))
    p.add_parameter("b", dist=stats.norm(0.0, 1.0))
    p.add_parameter("c", dist=(0.1, 0.7))
    p.add_parameter("d", dist=stats.norm(147.05, 0.3))
    u = np.concatenate([np.random.default_rng(3).uniform(size=(20000, 4)),
                        np.repeat(np.array([1e-9, 1 - 1e-9, 0.5, 1e-3, 1 - 1e-3])[:, None], 4, axis=1)])
    u[:2000, 1] = np.geomspace(1e-9, 0.5, 2000)
    u[2000:4000, 1] = 1.0 - np.geomspace(1e-9, 0.5, 2000)
    du = torch.from_numpy(u).to(DEV)
    th = torch.empty_like(du)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    L.check(L.lib().cf_ns_transform(C.byref(p.c_struct()), du.data_ptr(), u.shape[0], th.data_ptr(), stream))
    got = th.cpu().numpy()
    want = p.unit_to_physical(u)
    np.testing.assert_array_equal(got[:, [0, 2]], want[:, [0, 2]])  # uniform: the same bits
    np.testing.assert_allclose(got[:, 1], special.ndtri(u[:, 1]), rtol=0, atol=1e-13)  # Phi^-1 in standard units
    np.testing.assert_allclose(got[:, 3], want[:, 3], rtol=1e-13, atol=0)
    # the prior draw: u bit for bit, theta = T(u)
    n = 3001
    pu, pth = torch.empty((n, 4), dtype=torch.float64, device=DEV), torch.empty((n, 4), dtype=torch.float64, device=DEV)
    L.check(L.lib().cf_ns_prior_draw(C.byref(p.c_struct()), n, nested.ns_key(11, 0, 0), pu.data_ptr(), pth.data_ptr(), stream))
    ru, rth = ref.prior_draw(nested, p, n, 11)
    np.testing.assert_array_equal(pu.cpu().numpy(), ru)
    assert np.all((ru > 0) & (ru < 1))
    np.testing.assert_array_equal(pth.cpu().numpy()[:, [0, 2]], rth[:, [0, 2]])
    np.testing.assert_allclose(pth.cpu().numpy()[:, [1, 3]], rth[:, [1, 3]], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("normal_dims", [False, True])
def test_one_iteration_against_the_restatement(nested, normal_dims):
    """prior draw + one iteration (deaths with ties at L*, walk start, n_walk DE steps, fill) of the sampler's kernels against
    tests/nested_reference.py; bit for bit with uniform priors, within 1e-13 with normal dimensions; counters equal."""
    p = nested.Prior()
    p.add_parameter("a", dist=(-2, 2))
    p.add_parameter("b", dist=stats.norm(0.3, 0.5) if normal_dims else (-1, 3))
    p.add_parameter("c", dist=(0, 10))
    mu, sig = [0.2, 0.4, 6.0], [0.3, 0.4, 1.5]

    def loglike(theta):
        # elementwise torch ops only (a row gets the same bits in any batch); integer levels make ties at L*, and a strip
        # of dimension a is non-finite
        v = torch.zeros(theta.shape[0], dtype=torch.float64, device=theta.device)
        for k in range(3):
            v = v - 0.5 * ((theta[:, k] - mu[k]) / sig[k]) ** 2
        v = torch.floor(v)
        return torch.where((theta[:, 0] > 1.2) & (theta[:, 0] < 1.3), torch.full_like(v, math.nan), v)

    n, k, n_walk, seed = 1000, 500, 7, 5
    s = nested.DeviceNestedSampler(p, loglike, n_live=n, n_batch=k, n_walk=n_walk, seed=seed)
    s._start()
    u0, th0, l0 = s._live_u.cpu().numpy(), s._live_th.cpu().numpy(), s._live_l.cpu().numpy()
    ru, _ = ref.prior_draw(nested, p, n, seed)
    np.testing.assert_array_equal(u0, ru)
    sorted_l, order = torch.sort(s._live_l, stable=True)
    s._iterate(sorted_l, order, sorted_l.cpu().numpy())
    want = ref.iteration(nested, p, lambda t: loglike(torch.from_numpy(np.ascontiguousarray(t)).to(DEV)).cpu().numpy(),
                         u0, th0, l0, seed=seed, it=1, n_batch=k, n_walk=n_walk, gamma=s.gamma, sigma=s.sigma)
    assert want["m"] > k  # ties at L* died together
    c = s.walk_counts()
    assert [c["accepted"], c["out_of_cube"], c["nonfinite"]] == want["counts"].tolist()
    assert c["proposed"] == want["m"] * n_walk and min(want["counts"]) > 0
    np.testing.assert_array_equal(s._dead_l[0], want["dead_l"])
    np.testing.assert_array_equal(s._dead_th[0].cpu().numpy(), want["dead_th"])
    np.testing.assert_array_equal(s._live_u.cpu().numpy(), want["u"])
    if normal_dims:
        np.testing.assert_allclose(s._live_th.cpu().numpy(), want["th"], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(s._live_l.cpu().numpy(), want["logl"], rtol=1e-13, atol=0)
    else:
        np.testing.assert_array_equal(s._live_th.cpu().numpy(), want["th"])
        np.testing.assert_array_equal(s._live_l.cpu().numpy(), want["logl"])


# ---- 2. evidence against closed forms --------------------------------------------------------------------------------
def _check_gaussian_posterior(s, mean_true, cov_true):
    pts, lw, _ = s.posterior()
    mean, cov = _weighted_moments(pts, lw)
    sd = np.sqrt(np.diag(cov_true))
    assert np.all(np.abs(mean - mean_true) < 5 * sd / math.sqrt(s.n_eff)), (mean, mean_true)
    np.testing.assert_allclose(np.diag(cov), np.diag(cov_true), rtol=0.1)
    assert np.all(np.abs(cov - cov_true) <= 0.1 * np.outer(sd, sd)), (cov, cov_true)


def test_evidence_of_a_correlated_gaussian_in_a_box(nested):
    d = 5
    rng = np.random.default_rng(8)
    sd = np.array([0.5, 1.0, 0.3, 0.8, 0.6])
    a = rng.normal(size=(d, d))
    s_ = a @ a.T + d * np.eye(d)
    cov = s_ / np.sqrt(np.outer(np.diag(s_), np.diag(s_))) * np.outer(sd, sd)  # a well-conditioned correlation
    mu = np.array([0.5, -1.0, 1.5, 0.0, 2.0])
    p = nested.Prior()
    for k in range(d):
        p.add_parameter(f"x{k}", dist=(-5.0, 5.0))
    s = nested.DeviceNestedSampler(p, _gauss(mu, cov), n_live=2000, seed=1)
    assert s.run() is True
    truth = -d * math.log(10.0)
    assert abs(s.log_z - truth) < 4 * s.log_z_err, (s.log_z, truth, s.log_z_err)
    _check_gaussian_posterior(s, mu, cov)


def test_evidence_of_normal_priors_times_a_gaussian(nested):
    mu_pi, sd_pi = np.array([1.0, -2.0]), np.array([1.5, 0.8])
    c_pi = np.diag(sd_pi**2)
    mu_l = np.array([1.8, -1.5])
    c_l = np.array([[0.25, 0.1], [0.1, 0.36]])
    # a third dimension with a uniform prior on (0, 4) and a normalised Gaussian likelihood well inside it
    cov3 = np.zeros((3, 3))
    cov3[:2, :2], cov3[2, 2] = c_l, 0.2**2
    p = nested.Prior()
    p.add_parameter("a", dist=stats.norm(mu_pi[0], sd_pi[0]))
    p.add_parameter("b", dist=stats.norm(loc=mu_pi[1], scale=sd_pi[1]))
    p.add_parameter("c", dist=(0.0, 4.0))
    s = nested.DeviceNestedSampler(p, _gauss(np.r_[mu_l, 2.0], cov3), n_live=2000, seed=2)
    assert s.run() is True
    truth = stats.multivariate_normal(mu_pi, c_l + c_pi).logpdf(mu_l) - math.log(4.0)
    assert abs(s.log_z - truth) < 4 * s.log_z_err, (s.log_z, truth, s.log_z_err)
    post = np.linalg.inv(np.linalg.inv(c_l) + np.linalg.inv(c_pi))
    mean = post @ (np.linalg.solve(c_l, mu_l) + np.linalg.solve(c_pi, mu_pi))
    cov_true = np.zeros((3, 3))
    cov_true[:2, :2], cov_true[2, 2] = post, 0.2**2
    _check_gaussian_posterior(s, np.r_[mean, 2.0], cov_true)


def test_two_separated_modes_keep_their_weight(nested):
    d, w = 3, 0.03
    g1, g2 = _gauss(np.full(d, 0.25), w**2 * np.eye(d)), _gauss(np.full(d, 0.75), w**2 * np.eye(d))

    def loglike(theta):
        return torch.logaddexp(g1(theta), g2(theta)) - math.log(2.0)

    p = nested.Prior()
    for k in range(d):
        p.add_parameter(f"x{k}", dist=(0.0, 1.0))
    s = nested.DeviceNestedSampler(p, loglike, n_live=2000, seed=3)
    assert s.run() is True
    assert abs(s.log_z) < 4 * s.log_z_err, (s.log_z, s.log_z_err)  # a normalised mixture in the unit box
    pts, lw, _ = s.posterior()
    frac = np.exp(lw)[pts[:, 0] < 0.5].sum() / np.exp(lw).sum()
    assert abs(frac - 0.5) < 0.1, frac


# ---- 3. calibration -------------------------------------------------------------------------------------------------
def test_calibration_of_log_z_against_its_error(nested):
    """10 seeds of a 3-D Gaussian at n_live = 500: the scatter of log Z is within [0.5, 2] x the mean log_z_err and the bias
    below 3 err / sqrt(10) (what a walk too short to decorrelate would fail)."""
    mu, sd = np.array([0.4, 0.55, 0.6]), np.array([0.05, 0.08, 0.03])
    cov = np.diag(sd**2)
    cov[0, 1] = cov[1, 0] = 0.5 * sd[0] * sd[1]
    truth = 0.0  # the box (0, 1)^3 holds the Gaussian's mass to 1e-9
    p = nested.Prior()
    for k in range(3):
        p.add_parameter(f"x{k}", dist=(0.0, 1.0))
    zs, errs = [], []
    for seed in range(10):
        s = nested.DeviceNestedSampler(p, _gauss(mu, cov), n_live=500, seed=100 + seed)
        assert s.run() is True
        zs.append(s.log_z)
        errs.append(s.log_z_err)
    zs, err = np.array(zs), float(np.mean(errs))
    assert 0.5 * err <= zs.std(ddof=1) <= 2.0 * err, (zs, err)
    assert abs(zs.mean() - truth) < 3 * err / math.sqrt(10), (zs.mean(), truth, err)


# ---- 4. union3 against the integral ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def union3(pkg, nested):
    g = golden("sn_union3_1")
    box = pkg.likelihoods.SnUnion3.PRIOR_BOX
    lk = pkg.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    yield lk, box
    lk.engine.close()


def _trapezoid(lo, hi, n):
    w = np.full(n, (hi - lo) / (n - 1))
    w[[0, -1]] *= 0.5
    return np.linspace(lo, hi, n), w


def test_union3_log_evidence_against_a_grid_quadrature(pkg, nested, union3):
    lk, box = union3
    f = lk.engine.torch_log_prob(pkg.CF_OUT_LOGL)
    p = nested.Prior()
    p.add_parameter("dM", dist=(-1, +1))
    p.add_parameter("om", dist=(0.1, 0.7))
    p.add_parameter("v", dist=(-9, 9))
    s = nested.DeviceNestedSampler(p, f, n_live=7000, seed=42)
    assert s.run() is True
    # the same GPU log-likelihood on a 201 x 301 x 181 trapezoid grid over the whole box, 65536 rows per call
    axes = [_trapezoid(lo, hi, n) for (lo, hi), n in zip(box, (201, 301, 181))]
    x = [torch.from_numpy(a[0]).to(DEV) for a in axes]
    lw = [torch.from_numpy(np.log(a[1])).to(DEV) for a in axes]
    grid = torch.stack(torch.meshgrid(*x, indexing="ij"), -1).reshape(-1, 3)
    lt = (lw[0][:, None, None] + lw[1][None, :, None] + lw[2][None, None, :]).reshape(-1)
    lt = lt + torch.cat([f(grid[i:i + 65536].contiguous()) for i in range(0, grid.shape[0], 65536)])
    log_z_grid = float(torch.logsumexp(lt, 0)) - float(np.sum(np.log(box[:, 1] - box[:, 0])))
    wg = torch.exp(lt - torch.logsumexp(lt, 0))
    mean_g = (wg[:, None] * grid).sum(0)
    sd_g = torch.sqrt((wg[:, None] * (grid - mean_g) ** 2).sum(0)).cpu().numpy()
    mean_g = mean_g.cpu().numpy()
    assert abs(s.log_z - log_z_grid) < max(4 * s.log_z_err, 0.05), (s.log_z, log_z_grid, s.log_z_err)
    pts, lwp, _ = s.posterior()
    mean, cov = _weighted_moments(pts, lwp)
    assert np.all(np.abs(mean - mean_g) < 5 * sd_g / math.sqrt(s.n_eff)), (mean, mean_g)
    np.testing.assert_allclose(np.sqrt(np.diag(cov)), sd_g, rtol=0.1)
    # the reference publishes -20.5 (sn/union3_1.py:162, one decimal); a miss of this check alone is a question about the
    # fixture, not about the sampler
    assert abs(s.log_z - (-20.5)) <= 0.1, (s.log_z, log_z_grid)


# ---- 5. determinism -------------------------------------------------------------------------------------------------
def test_same_seed_same_bits(nested):
    p = nested.Prior()
    p.add_parameter("a", dist=(0.0, 1.0))
    p.add_parameter("b", dist=stats.norm(0.5, 0.2))
    f = _gauss([0.3, 0.6], [[0.01, 0.003], [0.003, 0.02]])
    runs = []
    for seed in (7, 7, 8):
        s = nested.DeviceNestedSampler(p, f, n_live=400, seed=seed)
        assert s.run() is True
        runs.append((s.posterior(), s.log_z, s.n_iterations, s.walk_counts()))
    (a, za, ia, ca), (b, zb, ib, cb), (c, zc, _, _) = runs
    assert za == zb and ia == ib and ca == cb
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert zc != za and not np.array_equal(c[0][: len(a[0])], a[0][: len(c[0])])
