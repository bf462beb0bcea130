"""GPU (-m gpu): the replica ensembles as a user runs them -- tempered runs whose answers are known in closed form, and R-hat.

Seeds are fixed, so every run is deterministic.  A bar is 5 standard errors, the standard error being the scatter of the C = 8
independent ladders' estimates over sqrt(8): it comes from the run, it is not tuned.  Every test also caps that standard error,
so a noisy run cannot hide a failure.  The caps of ln Z (0.05) and of the mode fraction (0.02) are three to five times what a numpy
rehearsal of these runs gave (0.007-0.018 and 0.004-0.006).  The caps of the moments allow an integrated autocorrelation time of
100 steps, a quarter of the 400 kept ones (the stretch move in two dimensions has about 10): 8 ladders x 400 steps x 32 walkers /
100 = 1024 effective samples, so se(mean) <= sigma / 32 and se(variance) <= sd(x^2) / 32, with sd(x^2) = sqrt(2) sigma^2 for a
Gaussian and sqrt(4 a^4 / 45) = 29.8 for the uniform law on (-a, a), a = 10.  A sampler slower than that has not converged in
the run and the test should say so."""
import numpy as np
import pytest
import torch

import replica_shapes as rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K, C, W = 5.0, 8, 32


@pytest.fixture(scope="module")
def RP(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.replicas


def _se(per):
    per = np.asarray(per, dtype=np.float64)
    return float(per.mean()), float(per.std(ddof=1) / np.sqrt(len(per)))


def _within(name, per, want, cap):
    mean, se = _se(per)
    print(f"{name}: {mean:.5f} +- {se:.5f} (want {want:.5f}, deviation {abs(mean - want) / se:.2f} se, cap {cap:.4f})")
    assert se <= cap, f"{name}: standard error {se:.4g} above its cap {cap:.4g}"
    assert abs(mean - want) <= K * se, f"{name}: {mean:.6g} is {abs(mean - want) / se:.1f} standard errors from {want:.6g}"


def _rung(ens, t, discard):
    """The stored samples of rung t of every ladder: [C, n * w, ndim]."""
    v = ens.get_chain(discard=discard)[:, [c * ens.T + t for c in range(ens.C)]]
    return v.permute(1, 0, 2, 3).reshape(ens.C, -1, ens.ndim).cpu().numpy()


# ---- a Gaussian in a box ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss_run(RP):
    betas = rs.gauss_betas()
    x = torch.from_numpy(rs.starts(C * len(betas), W, 2, seed=11)).to(DEV)
    ens = RP.ReplicaEnsemble(rs.gaussian_ll, x, seed=101, betas=betas, bounds=rs.BOX)
    ens.run_mcmc(600)
    torch.cuda.synchronize()
    return ens


def test_gaussian_stepping_stone_finds_the_closed_form_evidence(gauss_run):
    got = gauss_run.log_evidence(discard=200)
    assert got["log_z"] == pytest.approx(got["per_ladder"].mean()) and got["log_z_err"] == pytest.approx(_se(got["per_ladder"])[1])
    _within("ln Z (stepping stone)", got["per_ladder"], rs.LOG_Z, 0.05)


def test_gaussian_ti_lies_within_its_own_discretisation_error(gauss_run):
    """The trapezoid rule on this ladder is biased (about -0.3): the test only holds TI to the error it reports."""
    got = gauss_run.log_evidence(discard=200, method="ti")
    print(f"ln Z (TI): {got['log_z']:.5f} +- {got['log_z_err']:.5f}, discretisation {got['discretisation_err']:.5f}, want {rs.LOG_Z:.5f}")
    assert got["log_z_err"] <= 0.05
    assert abs(got["log_z"] - rs.LOG_Z) <= got["discretisation_err"] + K * got["log_z_err"]


def test_gaussian_rungs_have_the_moments_of_their_laws(gauss_run):
    cold, hot = _rung(gauss_run, gauss_run.T - 1, 200), _rung(gauss_run, 0, 200)
    for k, sigma in enumerate(rs.GAUSS_SIGMA):
        _within(f"beta = 1 mean[{k}]", cold[:, :, k].mean(axis=1), 0.0, sigma / 32)
        _within(f"beta = 1 var[{k}]", cold[:, :, k].var(axis=1), sigma ** 2, np.sqrt(2.0) * sigma ** 2 / 32)
        _within(f"beta = 0 mean[{k}]", hot[:, :, k].mean(axis=1), 0.0, np.sqrt(100.0 / 3.0) / 32)
        _within(f"beta = 0 var[{k}]", hot[:, :, k].var(axis=1), 100.0 / 3.0, np.sqrt(4.0e4 / 45.0) / 32)
    sf = gauss_run.swap_fraction()
    assert sf.shape == (C, gauss_run.T - 1) and bool(((sf > 0) & (sf < 1)).all())


# ---- two modes --------------------------------------------------------------------------------------------------------------
def _two_mode_starts(T):
    rng = np.random.default_rng(12)
    return torch.from_numpy(np.array([4.0, 0.0]) + rng.uniform(-0.1, 0.1, (C * T, W, 2))).to(DEV)


@pytest.fixture(scope="module")
def two_mode_run(RP):
    betas = rs.two_mode_betas()
    ens = RP.ReplicaEnsemble(rs.two_mode_ll, _two_mode_starts(len(betas)), seed=202, betas=betas, bounds=rs.BOX)
    ens.run_mcmc(1500)
    torch.cuda.synchronize()
    return ens


def test_without_tempering_no_walker_leaves_its_mode(RP):
    x = _two_mode_starts(len(rs.two_mode_betas()))
    ens = RP.ReplicaEnsemble(rs.two_mode_ll, x, seed=202)
    ens.run_mcmc(1500)
    assert float((ens.cold_chain(discard=500, flat=True)[:, 0] < 0).double().mean()) == 0.0


def test_the_ladder_finds_the_other_mode_with_its_weight(two_mode_run):
    cold = _rung(two_mode_run, two_mode_run.T - 1, 500)
    _within("fraction of beta = 1 samples with x < 0", (cold[:, :, 0] < 0).mean(axis=1), 0.7, 0.02)
    sf = two_mode_run.swap_fraction()
    print("swap fractions per pair of rungs (mean over ladders):", np.round(sf.mean(dim=0).cpu().numpy(), 3))
    assert bool(((sf > 0) & (sf < 1)).all())


def test_two_mode_stepping_stone_finds_the_closed_form_evidence(two_mode_run):
    _within("ln Z (stepping stone, two modes)", two_mode_run.log_evidence(discard=500)["per_ladder"], rs.LOG_Z, 0.05)


# ---- R-hat ------------------------------------------------------------------------------------------------------------------
def test_rhat_is_gelman_rubin_of_independent_chains_and_sees_two_groups(pkg, RP):
    rng = np.random.default_rng(13)
    x = rng.uniform(-0.1, 0.1, (8, W, 2))
    x[:4, :, 0] += 4.0
    x[4:, :, 0] -= 4.0
    ens = RP.ReplicaEnsemble(rs.two_mode_ll, torch.from_numpy(x).to(DEV), seed=303)
    ens.run_mcmc(200)
    got = ens.rhat(discard=50)
    chain = ens.get_chain(discard=50)  # [n, R, w, ndim]
    want = pkg.chain_stats.gelman_rubin(chain.permute(1, 0, 2, 3).reshape(8, 150 * W, 2).contiguous())
    assert torch.equal(got, want)
    print("R-hat of four replicas in each mode:", got.cpu().numpy())
    assert float(got[0]) > 2.0  # the two-group closed form is about 8; the bar only separates it from 1
    one_mode = RP.ReplicaEnsemble(rs.two_mode_ll, torch.from_numpy(x[:4]).to(DEV), seed=303)
    one_mode.run_mcmc(200)
    assert float(one_mode.rhat(discard=50).max()) < 1.2
    # a tempered run's R-hat is that of its beta = 1 rungs
    betas = [0.0, 0.1, 1.0]
    t = RP.ReplicaEnsemble(rs.gaussian_ll, torch.from_numpy(rs.starts(6, W, 2, seed=14)).to(DEV), seed=4, betas=betas, bounds=rs.BOX)
    t.run_mcmc(40)
    cold = t.get_chain(discard=10)[:, [2, 5]]
    assert torch.equal(t.rhat(discard=10), pkg.chain_stats.gelman_rubin(cold.permute(1, 0, 2, 3).reshape(2, 30 * W, 2).contiguous()))
    assert torch.equal(t.cold_chain(discard=10), cold)
