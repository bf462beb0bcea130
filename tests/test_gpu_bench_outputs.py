"""GPU (-m gpu): a plain `bench.py` run (no --full) times its K steps and prints the headline only, and `--dump-outputs` writes what
the last timed step computed: the per-walker log-probabilities of the seeded workload, the values the library returns for the same
walkers in-process and the CPU oracle reproduces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(pkg, tmp_path):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    W, n_sn, steps = 512, 300, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--walkers-per-gpu", str(W), "--n-sn", str(n_sn), "--precondition-ms", "0", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:800]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "evals/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(W * 1e3 / d["ms_per_step"], rel=1e-9)
    assert not {"roofline", "kernels_ms", "from_idle", "host_visible", "cpu_baseline", "device_ids"} & set(d), \
        "a plain run measures the headline only (the rest is --full)"

    assert os.listdir(tmp_path / "out") == ["log_prob.npy"]
    got = np.load(tmp_path / "out" / "log_prob.npy")
    assert got.dtype == np.float64 and got.shape == (W,) and np.all(np.isfinite(got))
    syn = pkg.synthetic.pantheon_like(n_sn=n_sn, seed=0)
    theta = pkg.synthetic.walkers(pkg.sn_pantheon.bounds, W, seed=0)
    lk = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    assert np.array_equal(got, lk.log_probs_vectorized(theta)), "the dump is not what the library returns for the same walkers"

    from oracle import oracle_c, oracle_np as onp

    ref = oracle_c.COracle(onp.Likelihood(
        ndim=4, z_max=lk.z_max, offset=onp.Slot(0), H0=onp.Slot(1), Om=onp.Slot(2), v=onp.Slot(3),
        z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"],
        bounds=pkg.sn_pantheon.bounds, gauss=[pkg.sn_pantheon.H0_PRIOR])).logp(theta)
    assert np.max(np.abs(got - ref) / np.abs(ref)) < 1e-10
