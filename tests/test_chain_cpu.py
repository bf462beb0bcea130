"""CPU: emcee's results interface of the ensemble (run_mcmc / get_chain / get_log_prob) with the tensor statement of the
moves, its rank-count invariance under gloo, and the numpy restatements the GPU chain-statistics tests compare against."""
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import chain_gloo_worker as cw
import chain_reference as ref
from conftest import golden

REF_MOVES = (("kde", 0.30), ("de", 0.70))  # sn/pantheon.py:114-117


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _twin_states(W, moves, n):
    """Positions / log P after each of n step() calls of an ensemble with the same seed, stacked [n, W, ...]."""
    twin = cw.make_ensemble(W, moves)
    xs, lps = [], []
    for _ in range(n):
        twin.step()
        x, lp = twin.full_state()
        xs.append(x.clone())
        lps.append(lp.clone())
    return torch.stack(xs), torch.stack(lps)


def test_no_results_before_a_run():
    ens = cw.make_ensemble(24, REF_MOVES)
    assert ens.iteration == 0
    with pytest.raises(AttributeError):
        ens.get_chain()
    with pytest.raises(AttributeError):
        ens.get_log_prob(flat=True)
    ens.run(2)  # plain steps record nothing
    with pytest.raises(AttributeError):
        ens.get_chain()


@pytest.mark.parametrize("thin_by", [1, 3])
@pytest.mark.parametrize("moves", [REF_MOVES, (("stretch", 1.0),)])
def test_recorded_chain_is_the_stacked_end_of_step_states(thin_by, moves):
    """run_mcmc stores every thin_by-th end-of-step state; get_chain / get_log_prob slice it as emcee does
    ([discard + thin - 1 :: thin]; flat = step-major, walker-minor); two calls append."""
    W, n1, n2 = 30, 7, 5
    ens = cw.make_ensemble(W, moves)
    ens.run_mcmc(n1, thin_by=thin_by)
    ens.run_mcmc(n2, thin_by=thin_by)
    assert ens.iteration == n1 + n2 and ens.step_count == (n1 + n2) * thin_by
    xs, lps = _twin_states(W, moves, (n1 + n2) * thin_by)
    xs, lps = xs[thin_by - 1::thin_by], lps[thin_by - 1::thin_by]
    assert torch.equal(ens.get_chain(), xs) and torch.equal(ens.get_log_prob(), lps)
    for discard, thin in ((0, 1), (3, 1), (2, 2), (1, 4), (11, 1), (12, 1), (40, 3)):
        want = xs[discard + thin - 1::thin]
        got = ens.get_chain(discard=discard, thin=thin)
        assert torch.equal(got, want)
        flat = ens.get_chain(discard=discard, thin=thin, flat=True)
        assert flat.shape == (want.shape[0] * W, 3) and torch.equal(flat, want.reshape(-1, 3))
        assert torch.equal(ens.get_log_prob(discard=discard, thin=thin, flat=True), lps[discard + thin - 1::thin].reshape(-1))
    x, lp = ens.full_state()
    assert torch.equal(x, xs[-1]) and torch.equal(lp, lps[-1])


def test_per_walker_acceptance_needs_the_kernels():
    ens = cw.make_ensemble(24, REF_MOVES)
    ens.run_mcmc(3)
    with pytest.raises(NotImplementedError):
        ens.walker_acceptance_fraction()


def test_device_statistics_refuse_cpu_tensors(pkg):
    cs = pkg.chain_stats
    x = torch.zeros((10, 4, 2), dtype=torch.float64)
    for fn in (cs.integrated_time, cs.gelman_rubin):
        with pytest.raises(ValueError, match="no CPU implementation"):
            fn(x)
    with pytest.raises(ValueError, match="no CPU implementation"):
        cs.percentile(x[:, 0], 50)


@pytest.mark.parametrize("world,W,thin_by", [(2, 48, 1), (3, 50, 2)])
def test_sharded_get_chain_is_bit_identical_for_any_number_of_ranks(tmp_path, world, W, thin_by):
    """Every rank records only its slice; get_chain returns the full chain on every rank (3 ranks: ragged shards)."""
    one = cw.record(cw.make_ensemble(W, REF_MOVES), 6, thin_by)
    path = str(tmp_path / "chain")
    mp.spawn(cw.worker, args=(world, _free_port(), W, 6, thin_by, REF_MOVES, path), nprocs=world, join=True)
    rows = []
    for r in range(world):
        got = torch.load(f"{path}.{r}")
        rows.append(got["local_rows"])
        assert got["iteration"] == one["iteration"] == 6
        for k in ("chain", "logp", "flat"):
            assert torch.equal(got[k], one[k]), f"rank {r}: {k}"
    assert sum(rows) == W and max(rows) < W


@pytest.mark.parametrize("rho", [0.5, 0.9])
def test_numpy_integrated_time_on_ar1_chains(rho):
    """The restatement of emcee's estimator lands near the AR(1) chain's known tau = (1 + rho) / (1 - rho)."""
    want = (1 + rho) / (1 - rho)
    x = ref.ar1_chain(6000, 24, 2, rho, seed=5)
    tau, window, taus, short = ref.integrated_time(x)
    assert not short
    assert np.all(np.abs(tau / want - 1) < 0.1), (tau, want)
    for d in range(2):  # the window is the first lag at which lag >= c tau
        assert window[d] >= 5 * taus[window[d], d] and np.all(np.arange(window[d]) < 5 * taus[: window[d], d])
    _, _, _, short = ref.integrated_time(x[:120])  # 50 tau > 120 steps for both
    assert short


def test_numpy_gelman_rubin_matches_the_reference_fixture():
    g = golden("gelman_rubin")
    chains = ref.gelman_rubin_input(int(g["seed"]), tuple(int(v) for v in g["shape"]))
    got = ref.gelman_rubin(chains)
    assert np.allclose(got, g["rhat"], rtol=0, atol=1e-12)
    assert np.all(g["rhat"] > 1.005)
