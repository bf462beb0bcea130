"""GPU (-m gpu): ``evidence.bridge`` end to end.

* The three closed-form targets of tests/bridge_reference.py as torch objectives on the device, fed the host-drawn iid samples
  of the CPU test: the same two conditions (|ln Z - closed form| <= 5 x the reported error, reported error <= 0.02), ln Z within
  1e-9 of the long-double restatement fed the same samples and key, and the objective rows spent.
* The Union3 22-bin likelihood through the engine: ``ShardedEnsemble.log_evidence`` of a 64-walker x 2000-step chain, both
  methods, against ``DeviceNestedSampler.log_z`` on the same engine and box: |difference| <= 5 sqrt(err_bridge^2 +
  (1.2 err_nested)^2) with both errors below 0.1 (1.2: the measured scatter ratio of nested.py's header).  The seeds below were
  fixed before the first GPU run.
* The example script, run small, for plumbing only.
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

import bridge_reference as BR
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ENSEMBLE_SEED, START_SEED, NESTED_SEED, BRIDGE_SEED = 9, 3, 42, 1


@pytest.fixture(scope="module")
def E(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.evidence


def _inside(th):
    return ((th > 0.0) & (th < 1.0)).all(dim=1)


def torch_objective(name):
    ninf = float("-inf")
    if name == "expwall":
        a = torch.from_numpy(BR.EXP_A).to(DEV)
        return lambda th: torch.where(_inside(th), -(th * a).sum(dim=1), ninf)
    if name == "halfwall":
        m, s = torch.from_numpy(BR.HALF_M).to(DEV), torch.from_numpy(BR.HALF_S).to(DEV)
        return lambda th: torch.where(_inside(th), -0.5 * (((th - m) / s) ** 2).sum(dim=1), ninf)
    mu, prec = torch.from_numpy(BR.GAUSS_MEAN).to(DEV), torch.from_numpy(BR.GAUSS_PREC).to(DEV)

    def gauss(th):
        c = th - mu
        return torch.where(_inside(th), -0.5 * ((c @ prec) * c).sum(dim=1), ninf)

    return gauss


@pytest.mark.parametrize("method", ["normal", "warp3"])
@pytest.mark.parametrize("name", sorted(BR.TARGETS))
def test_closed_form_objectives_on_the_device(E, name, method):
    t = BR.TARGETS[name]
    d = t["ndim"]
    f = torch_objective(name)
    for seed in BR.SEEDS:
        th, lp = BR.target_samples(name, seed)
        r = E.bridge(f, th, np.zeros(d), np.ones(d), log_probs=lp, method=method, seed=seed)
        ref = BR.target_bridge(name, seed, method)
        ratio = abs(r.log_z - t["log_z"]) / r.log_z_err
        print(f"{name} {method} seed {seed}: ln Z = {r.log_z:.6f} +- {r.log_z_err:.4f} (closed form {t['log_z']:.6f}, ratio {ratio:.2f}); "
              f"device - restatement = {r.log_z - ref['log_z']:.2e} (bar 1e-9), error {r.log_z_err - ref['log_z_err']:.2e}; "
              f"{r.n_iter} iterations")
        assert r.status == E.CONVERGED and r.converged and r.method == method
        assert ratio <= 5.0 and r.log_z_err <= 0.02
        assert abs(r.log_z - ref["log_z"]) <= 1e-9 and abs(r.log_z_err - ref["log_z_err"]) <= 1e-9
        assert (r.n_fit, r.n_iter_rows, r.n_draws, r.n_eff, r.tau_f, r.tau_reliable) == (2048, 2048, 2048, 2048.0, 1.0, True)
        assert r.n_like == (2048 if method == "normal" else 3 * 2048) == ref["n_like"]
        assert r.l1.is_cuda and r.l1.shape == (2048,) and r.l2.shape == (2048,) and r.f2.shape == (2048,)
        assert r.mean.shape == (d,) and np.allclose(r.chol, np.asarray(ref["chol"], dtype=np.float64), rtol=1e-10, atol=1e-13)


def test_options_of_bridge(E):
    """Without log_probs the N1 rows are evaluated; the objective is called with at most `chunk` rows and chunking changes no
    bit; n_draws and n_eff do what they say; a flat tensor on the device is used where it is; a NaN from the objective at a
    draw is status NONFINITE; a sample outside the box is a ValueError."""
    th, lp = BR.target_samples("expwall", 2)
    lo, hi = np.zeros(3), np.ones(3)
    f = torch_objective("expwall")
    base = E.bridge(f, th, lo, hi, log_probs=lp, seed=2)
    rows = []

    def counted(x):
        assert x.is_cuda and x.dtype == torch.float64 and x.is_contiguous()
        rows.append(x.shape[0])
        return f(x)

    r = E.bridge(counted, torch.from_numpy(th).to(DEV), lo, hi, seed=2, chunk=500)
    assert max(rows) <= 500 and sum(rows) == r.n_like == 4096 and rows.count(500) == 8
    assert abs(r.log_z - base.log_z) <= 1e-12 and torch.equal(r.l2, base.l2)
    few = E.bridge(f, th, lo, hi, log_probs=lp, seed=2, n_draws=1000, n_eff=512.0, method="warp3")
    ref = BR.bridge(BR.TARGETS["expwall"]["logp"], th, lo, hi, log_probs=lp, seed=2, n_draws=1000, n_eff=512.0, method="warp3")
    assert (few.n_draws, few.n_eff, few.tau_f, few.n_like) == (1000, 512.0, 4.0, 2048 + 2000)
    assert abs(few.log_z - ref["log_z"]) <= 1e-9 and abs(few.log_z_err - ref["log_z_err"]) <= 1e-9
    assert few.log_z_err > base.log_z_err
    other = E.bridge(f, th, lo, hi, log_probs=lp, seed=3)
    assert other.log_z != base.log_z and abs(other.log_z - base.log_z) <= 5 * np.hypot(other.log_z_err, base.log_z_err)
    nan = E.bridge(lambda x: torch.where(x[:, 0] > 0.5, torch.full_like(x[:, 0], float("nan")), f(x)), th, lo, hi, log_probs=lp, seed=2)
    assert nan.status == E.NONFINITE and np.isnan(nan.log_z) and np.isnan(nan.log_z_err)
    out = th.copy()
    out[3000, 1] = 1.0
    with pytest.raises(ValueError, match="strictly inside"):
        E.bridge(f, out, lo, hi, log_probs=lp)
    bad_lp = lp.copy()
    bad_lp[3000] = -np.inf
    with pytest.raises(ValueError, match="finite log posterior"):
        E.bridge(f, th, lo, hi, log_probs=bad_lp)
    flat = th.copy()
    flat[:, 2] = 0.25
    with pytest.raises(ValueError, match="column 2"):
        E.bridge(f, flat, lo, hi)


# ---- the engine against nested sampling --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def union3(pkg, E):
    g = golden("sn_union3_1")
    box = pkg.likelihoods.SnUnion3.PRIOR_BOX
    lk = pkg.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    rng = np.random.default_rng(START_SEED)
    start = np.array([0.0, 0.3, -3.0]) + np.array([0.02, 0.02, 1.0]) * rng.standard_normal((64, 3))
    ens = pkg.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(DEV), seed=ENSEMBLE_SEED,
                                       moves=pkg.ensemble.REFERENCE_MOVES)
    ens.run_mcmc(2000)
    prior = pkg.nested.Prior()
    for k, key in enumerate(("dM", "om", "v")):
        prior.add_parameter(key, dist=(float(box[k, 0]), float(box[k, 1])))
    ns = pkg.nested.DeviceNestedSampler(prior, lk.engine.torch_log_prob(pkg.CF_OUT_LOGL), n_live=2000, seed=NESTED_SEED)
    assert ns.run() is True
    yield ens, ns, box
    lk.engine.close()


@pytest.mark.parametrize("method", ["normal", "warp3"])
def test_union3_chain_against_nested_sampling(E, union3, method):
    ens, ns, box = union3
    r = ens.log_evidence(discard=400, method=method, seed=BRIDGE_SEED)
    bar = 5.0 * np.hypot(r.log_z_err, 1.2 * ns.log_z_err)
    print(f"union3 {method}: bridge ln Z = {r.log_z:.4f} +- {r.log_z_err:.4f} ({r.n_iter} iterations, n_eff {r.n_eff:.0f} of "
          f"{r.n_iter_rows}, tau_f {r.tau_f:.1f}, reliable {r.tau_reliable}); nested ln Z = {ns.log_z:.4f} +- {ns.log_z_err:.4f}; "
          f"difference {r.log_z - ns.log_z:+.4f} (bar {bar:.4f})")
    assert r.status == E.CONVERGED
    assert (r.n_fit, r.n_iter_rows, r.n_draws) == (800 * 64, 800 * 64, 800 * 64)
    assert r.n_like == (800 * 64 if method == "normal" else 3 * 800 * 64)
    assert 1.0 <= r.n_eff <= r.n_iter_rows and r.tau_f >= 1.0
    assert r.log_z_err < 0.1 and ns.log_z_err < 0.1
    assert abs(r.log_z - ns.log_z) <= bar


def test_log_evidence_needs_the_box(pkg, union3):
    ens, _, box = union3
    free = pkg.ensemble.ShardedEnsemble(lambda th: ens.log_prob_fn(th), ens.x.clone(), seed=1)
    free.run_mcmc(40)
    with pytest.raises(ValueError, match="needs the box"):
        free.log_evidence()
    with pytest.raises(ValueError, match=r"\[3, 2\]"):
        free.log_evidence(bounds=box[:2])
    r = free.log_evidence(bounds=box, n_draws=256)
    assert r.n_fit == 20 * 64 and r.n_draws == 256 and np.isfinite(r.log_z)


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_example_runs_small(E, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        ex = importlib.import_module("union3_bridge_evidence")
    finally:
        sys.path.pop(0)
    res = ex.main(["--walkers", "32", "--steps", "300", "--discard", "100", "--n-live", "200"])
    text = capsys.readouterr().out
    assert "ln B (step against v = 0)" in text and "2.57 sigma" in text and text.count("bridge (") == 6
    for name in ("step", "v = 0"):
        for m in E.METHODS:
            assert np.isfinite(res[name][m].log_z) and np.isfinite(res[name][m].log_z_err)
        assert np.isfinite(res[name]["laplace"]) and np.isfinite(res[name]["nested"][0])
