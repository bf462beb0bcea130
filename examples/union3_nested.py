#!/usr/bin/env python3
"""sn/union3_1.py (flat LCDM with the velocity step, real data of the golden fixture) under the device nested sampler.

The script's nautilus run -- ``Prior`` with dM (-1, 1), om (0.1, 0.7), v (-9, 9); ``Sampler(prior, log_likelihood,
n_live=7_000, seed=42)``; ``run``; ``posterior``; ``log_z`` -- on ``nested.DeviceNestedSampler``, printed beside the block
the reference publishes (sn/union3_1.py:155-168) and the Laplace value of tools/union3_evidence.py.

    python examples/union3_nested.py
"""
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")

PUBLISHED = {"dM": "0.004 ± 0.023", "om": "0.299 +0.025 -0.028", "v": "-3.07 ± 1.20 (x 100 km/s)", "chi2_map": 22.15,
             "log_z": -20.5}


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    nested = amd.nested

    prior = nested.Prior()
    prior.add_parameter("dM", dist=(-1, +1))  # mag
    prior.add_parameter("om", dist=(0.1, 0.7))
    prior.add_parameter("v", dist=(-9, 9))  # x 100 km/s
    sampler = nested.DeviceNestedSampler(prior, lk.engine.torch_log_prob(amd.CF_OUT_LOGL), n_live=7_000, seed=42)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sampler.run(verbose=True)
    wall = time.perf_counter() - t0
    samples, log_w, log_l = sampler.posterior()

    w = np.exp(log_w)
    mean = w @ samples
    std = np.sqrt(w @ (samples - mean) ** 2)
    print(f"\nrun(): {wall:.2f} s, {sampler.n_like} likelihood evaluations, {sampler.n_iterations} iterations, "
          f"walk acceptance {sampler.acceptance:.3f}, n_eff {sampler.n_eff:.0f}")
    print(f"{'':10s}{'device nested sampler':>28s}   reference (nautilus, sn/union3_1.py:155-168)")
    for k, key in enumerate(prior.keys):
        print(f"{key:10s}{mean[k]:>16.5f} ± {std[k]:.5f}   {PUBLISHED[key]}")
    print(f"{'v_km_s':10s}{100 * mean[2]:>16.1f} ± {100 * std[2]:.1f}   -307 ± 120")
    print(f"{'χ2 (MAP)':10s}{-2 * np.max(log_l):>16.2f}            {PUBLISHED['chi2_map']}")
    print(f"{'Log Z':10s}{sampler.log_z:>16.3f} ± {sampler.log_z_err:.3f}   {PUBLISHED['log_z']}")

    # the Laplace approximation at the MAP (tools/union3_evidence.py), for contrast
    rng = np.random.default_rng(3)
    start = np.array([0.0, 0.3, -3.0]) + np.array([0.02, 0.02, 1.0]) * rng.standard_normal((2048, 3))
    ens = amd.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to("cuda:0"), seed=9,
                                       moves=amd.ensemble.REFERENCE_MOVES)
    ens.run(400)
    lap = amd.laplace.log_evidence(ens.x.cpu().numpy(), ens.logp.cpu().numpy(), lk.log_probs_vectorized, box)
    print(f"{'Laplace':10s}{float(np.ravel(lap)[0]):>16.3f}            (Gaussian approximation at the MAP)")
    lk.engine.close()


if __name__ == "__main__":
    main()
