"""GPU (-m gpu): the recorded chain and emcee's diagnostics on the device.

* The fused recording (cf_ens_accept_record) stores exactly the end-of-step states that step() + copies of x / log P give
  on a twin ensemble, for every move (stretch, DE on three splits, KDE, the reference mixture), and leaves the chain itself
  bit-identical to a run that does not record.
* integrated_time from the direct lag-sum kernels against the numpy FFT restatement of emcee's estimator
  (tests/chain_reference.py): same window, tau within 1e-10 relative, same AutocorrError cases, NaN for a frozen walker,
  same bits on a second call.
* gelman_rubin against the reference's recorded output; percentile bit for bit against np.percentile.
* Sharded natively: 2 and 3 rank processes on one GPU give the one-rank chain and tau bit for bit.
"""
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import chain_reference as ref
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "chain_rank_worker.py")
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def need_gpu(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")


@pytest.fixture(scope="module")
def pantheon(pkg, need_gpu):
    syn = pkg.synthetic.pantheon_like(n_sn=300, seed=3)
    lk = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    yield lk
    lk.engine.close()


def _start(pkg, W, seed=1):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(pkg.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * rng.standard_normal((W, 4))).to(DEV)


MOVES = {"stretch": (("stretch", 1.0),), "de": (("de", 1.0),), "kde": (("kde", 1.0),), "ref": (("kde", 0.30), ("de", 0.70))}


@pytest.mark.parametrize("thin_by", [1, 3])
@pytest.mark.parametrize("W", [150, 4096])
@pytest.mark.parametrize("moves", ["stretch", "de", "kde", "ref"])
def test_fused_recording_equals_stepped_copies(pkg, pantheon, moves, W, thin_by):
    E = pkg.ensemble
    nsteps = 6
    lp = pantheon.engine.torch_log_prob()
    rec = E.ShardedEnsemble(lp, _start(pkg, W), seed=9, moves=MOVES[moves])
    twin = E.ShardedEnsemble(lp, _start(pkg, W), seed=9, moves=MOVES[moves])
    assert isinstance(rec.impl, E.NativeMoves) and rec.de_splits == 3
    rec.run_mcmc(nsteps, thin_by=thin_by)
    xs, lps = [], []
    for _ in range(nsteps * thin_by):
        twin.step()  # cf_ens_accept: no recording
        x, l = twin.full_state()
        xs.append(x.clone())
        lps.append(l.clone())
    xs, lps = torch.stack(xs)[thin_by - 1::thin_by], torch.stack(lps)[thin_by - 1::thin_by]
    assert rec.iteration == nsteps
    assert torch.equal(rec.get_chain(), xs), "recorded positions differ from the stepped copies"
    assert torch.equal(rec.get_log_prob(), lps), "recorded log P differs from the stepped copies"
    assert torch.equal(rec.get_chain(discard=1, thin=2, flat=True), xs[2::2].reshape(-1, 4))
    x, l = rec.full_state()
    assert torch.equal(x, twin.x) and torch.equal(l, twin.logp), "recording changed the chain"
    assert rec.n_accepted == twin.n_accepted
    counts = rec._walker_acc
    assert int(counts.sum()) == rec.n_accepted > 0
    frac = rec.walker_acceptance_fraction()
    assert frac.shape == (W,) and frac.device == x.device
    assert torch.equal(frac, counts.to(torch.float64) / (nsteps * thin_by))
    assert float(frac.mean()) == pytest.approx(rec.acceptance_fraction(), rel=1e-12)


def _device_vs_numpy(pkg, x_host, c=5):
    tau_d, win_d = pkg.chain_stats.autocorr_window_search(torch.from_numpy(x_host).to(DEV), c)
    tau_h, win_h, taus_h, _ = ref.integrated_time(x_host, c=c)
    return tau_d, win_d, tau_h, win_h, taus_h


def test_integrated_time_on_an_ar1_chain(pkg, need_gpu):
    """[2500, 4096, 4] AR(1) chain (tau ~ 32): the device's windows and taus are the FFT restatement's."""
    x = ref.ar1_chain(2500, 4096, 4, 0.94, seed=3)
    tau_d, win_d, tau_h, win_h, taus_h = _device_vs_numpy(pkg, x)
    assert ref.window_margin(taus_h, win_h) > 1e-9, "fixture too close to a window boundary"
    assert np.array_equal(win_d, win_h)
    assert np.all(np.abs(tau_d / tau_h - 1) < 1e-10), (tau_d, tau_h)
    assert np.all(np.abs(tau_d / (1.94 / 0.06) - 1) < 0.15)
    xd = torch.from_numpy(x).to(DEV)
    t1 = pkg.chain_stats.integrated_time(xd)
    t2 = pkg.chain_stats.integrated_time(xd)
    assert np.array_equal(t1, t2) and np.array_equal(t1, tau_d), "two calls must give the same bits"
    # too short for tol = 50: raised, or warned with quiet, in the restatement's cases
    short = xd[:1000]
    _, _, _, too_short = ref.integrated_time(x[:1000])
    assert too_short
    with pytest.raises(pkg.chain_stats.AutocorrError) as ei:
        pkg.chain_stats.integrated_time(short)
    assert ei.value.tau.shape == (4,)
    with pytest.warns(UserWarning):
        tq = pkg.chain_stats.integrated_time(short, quiet=True)
    assert np.array_equal(tq, ei.value.tau)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pkg.chain_stats.integrated_time(short, tol=10)  # 10 tau < 1000: no error, no warning


def test_integrated_time_on_a_recorded_pantheon_chain(pkg, pantheon):
    E = pkg.ensemble
    ens = E.ShardedEnsemble(pantheon.engine.torch_log_prob(), _start(pkg, 256), seed=2, moves=E.REFERENCE_MOVES)
    ens.run(100)
    ens.run_mcmc(600)
    chain = ens.get_chain()
    x = chain.cpu().numpy()
    tau_d, win_d = pkg.chain_stats.autocorr_window_search(chain)
    tau_h, win_h, taus_h, too_short = ref.integrated_time(x)
    assert ref.window_margin(taus_h, win_h) > 1e-9, "fixture too close to a window boundary"
    assert np.array_equal(win_d, win_h)
    assert np.all(np.abs(tau_d / tau_h - 1) < 1e-10), (tau_d, tau_h)
    if too_short:
        with pytest.raises(pkg.chain_stats.AutocorrError):
            ens.get_autocorr_time()
    else:
        assert np.array_equal(ens.get_autocorr_time(), tau_d)
    assert np.array_equal(ens.get_autocorr_time(discard=100, thin=2, quiet=True),
                          2 * pkg.chain_stats.integrated_time(chain[101::2], quiet=True))


def test_frozen_walker_gives_nan_as_emcee(pkg, need_gpu):
    x = ref.ar1_chain(400, 32, 3, 0.6, seed=8)
    x[:, 5, 1] = 0.25  # walker 5 never moves in dimension 1
    with np.errstate(invalid="ignore", divide="ignore"):
        tau_d, win_d, tau_h, win_h, _ = _device_vs_numpy(pkg, x)
    assert np.isnan(tau_h[1]) and np.isnan(tau_d[1])
    assert win_d[1] == win_h[1] == 399
    ok = [0, 2]
    assert np.array_equal(win_d[ok], win_h[ok]) and np.all(np.abs(tau_d[ok] / tau_h[ok] - 1) < 1e-10)
    assert np.isnan(pkg.chain_stats.integrated_time(torch.from_numpy(x).to(DEV), tol=1)[1])


def test_gelman_rubin_matches_the_reference(pkg, need_gpu):
    g = golden("gelman_rubin")
    chains = ref.gelman_rubin_input(int(g["seed"]), tuple(int(v) for v in g["shape"]))
    got = pkg.chain_stats.gelman_rubin(torch.from_numpy(chains).to(DEV))
    assert got.is_cuda
    assert np.allclose(got.cpu().numpy(), g["rhat"], rtol=0, atol=1e-12)
    x = np.random.default_rng(4).standard_normal((50, 20, 3))
    assert np.allclose(pkg.chain_stats.gelman_rubin(torch.from_numpy(x).to(DEV)).cpu().numpy(), ref.gelman_rubin(x),
                       rtol=0, atol=1e-12)


@pytest.mark.parametrize("n", [1, 3, 5, 101, 4096 * 7 + 1])
def test_percentile_has_numpys_bits(pkg, need_gpu, n):
    rng = np.random.default_rng(n)
    s = rng.standard_normal((n, 4)) * np.array([0.02, 1.0, 0.03, 0.3]) + pkg.synthetic.THETA_TRUE
    s[: n // 3, 3] = np.round(s[: n // 3, 3], 1)  # ties
    sd = torch.from_numpy(s).to(DEV)
    # 12.5 with n = 5 and 25 with n = 3 put the virtual index at k + 0.5 (the branch of _lerp at t >= 0.5)
    for q in ([15.9, 50, 84.1], [0, 100], [12.5, 25, 37.5, 62.5, 75], 50, 0, 100, [99.99, 0.01]):
        got = pkg.chain_stats.percentile(sd, q).cpu().numpy()
        want = np.percentile(s, q, axis=0)
        assert got.shape == want.shape and np.array_equal(got, want), (n, q)
    assert np.array_equal(pkg.chain_stats.percentile(sd[:, 2], [15.9, 84.1]).cpu().numpy(), np.percentile(s[:, 2], [15.9, 84.1]))
    with pytest.raises(ValueError):
        pkg.chain_stats.percentile(sd, 101)


def test_ensemble_summaries_are_the_reference_calls(pkg, pantheon):
    E = pkg.ensemble
    ens = E.ShardedEnsemble(pantheon.engine.torch_log_prob(), _start(pkg, 150), seed=4, moves=E.REFERENCE_MOVES)
    ens.run_mcmc(60)
    chain = ens.get_chain(discard=10).cpu().numpy()
    assert np.allclose(ens.gelman_rubin(discard=10).cpu().numpy(), ref.gelman_rubin(chain), rtol=0, atol=1e-12)
    flat = ens.get_chain(discard=10, thin=2, flat=True).cpu().numpy()
    assert np.array_equal(ens.percentile([15.9, 50, 84.1], discard=10, thin=2).cpu().numpy(),
                          np.percentile(flat, [15.9, 50, 84.1], axis=0))


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _run(tmp_path, world, walkers, steps, thin_by):
    out = str(tmp_path / f"chain_w{world}.npz")
    port = _free_port()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    procs = [subprocess.Popen([sys.executable, WORKER, "--rank", str(r), "--world", str(world), "--port", str(port), "--walkers",
                               str(walkers), "--steps", str(steps), "--thin-by", str(thin_by), "--out", out],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    fails = []
    for r, p in enumerate(procs):
        try:
            so, se = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
            fails.append(f"rank {r} timed out\n{se[-1500:]}")
            continue
        if p.returncode != 0:
            fails.append(f"rank {r} exit {p.returncode}\n{se[-1500:]}")
    assert not fails, "\n".join(fails)
    return np.load(out)


def test_sharded_recording_is_bit_identical_to_one_rank(tmp_path, need_gpu):
    """2 ranks (equal shards) and 3 ranks (ragged shards 22 / 21 / 21): get_chain, get_log_prob, get_autocorr_time and the
    per-walker acceptance equal the one-rank run bit for bit."""
    walkers, steps, thin_by = 64, 40, 2
    one = _run(tmp_path, 1, walkers, steps, thin_by)
    assert one["chain"].shape == (steps, walkers, 4) and np.all(np.isfinite(one["logp"]))
    for world in (2, 3):
        got = _run(tmp_path, world, walkers, steps, thin_by)
        assert int(got["local_rows"]) < walkers
        for k in ("chain", "logp", "tau", "frac"):
            assert np.array_equal(got[k], one[k], equal_nan=True), f"world {world}: {k} differs from one rank"
