#!/usr/bin/env python3
"""
The device counterpart of the reference's Pantheon+ fit (sn/pantheon.py:100-164, without the plots): burn-in, run_mcmc with
the reference's move mixture (KDEMove 30 % + DEMove 70 %), then emcee's results interface -- Gelman-Rubin, autocorrelation
time, acceptance, effective samples, the 15.9 / 50 / 84.1 % labels, chi^2 at the median and the Laplace log-evidence.
The chain stays on the GPU; only the summaries (and the flat chain handed to the evidence's optimiser) reach the host.

    python examples/pantheon_device_fit.py [--walkers 150] [--burn 500] [--steps 2500] [--n-sn 1701]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=150)
    ap.add_argument("--burn", type=int, default=500)
    ap.add_argument("--steps", type=int, default=2500)
    ap.add_argument("--n-sn", type=int, default=1701)
    args = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    dev = torch.device("cuda:0")
    syn = amd.synthetic.pantheon_like(n_sn=args.n_sn, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    bounds = lk.bounds
    rng = np.random.default_rng(42)
    initial_pos = rng.uniform(bounds[:, 0], bounds[:, 1], size=(args.walkers, len(bounds)))  # sn/pantheon.py:112
    ens = amd.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(initial_pos).to(dev), seed=42,
                                       moves=amd.ensemble.REFERENCE_MOVES)
    t0 = time.perf_counter()
    ens.run_mcmc(args.burn + args.steps)
    torch.cuda.synchronize()
    t_run = time.perf_counter() - t0

    burn_in, n_walkers, n_dim = args.burn, args.walkers, len(bounds)
    samples = ens.get_chain(discard=burn_in, flat=True)
    log_probs = ens.get_log_prob(discard=burn_in, flat=True)
    print(f"{n_walkers} walkers x {args.burn + args.steps} steps on the device: {t_run:.2f} s")
    print("Gelman-Rubin", ens.gelman_rubin(discard=burn_in).cpu().numpy())
    try:
        tau = ens.get_autocorr_time()
        print("Autocorrelation time", tau)
        print("Acceptance fraction", float(ens.walker_acceptance_fraction().mean()))
        print("effective samples", n_walkers * args.steps * n_dim / np.max(tau))
    except amd.chain_stats.AutocorrError:
        print("Autocorrelation time", "Not available")

    pct = ens.percentile([15.9, 50, 84.1], discard=burn_in).cpu().numpy()
    (M0_16, M0_50, M0_84), (H0_16, H0_50, H0_84), (Om_16, Om_50, Om_84), (v_16, v_50, v_84) = pct.T
    best_fit = pct[1]
    print("M0", f"{M0_50:.3f} +{M0_84-M0_50:.3f}/-{M0_50-M0_16:.3f}")
    print("H0", f"{H0_50:.2f} +{H0_84-H0_50:.2f}/-{H0_50-H0_16:.2f} km/s/Mpc")
    print("Ωm", f"{Om_50:.3f} +{Om_84-Om_50:.3f}/-{Om_50-Om_16:.3f}")
    print("v", f"{v_50:.3f} +{v_84-v_50:.3f}/-{v_50-v_16:.3f} x 100 km/s")
    print("Chi squared", float(np.asarray(lk.chi_squared(best_fit)).ravel()[0]))
    log_evd = amd.laplace.log_evidence(samples.cpu().numpy(), log_probs.cpu().numpy(), lk.log_probs_vectorized, bounds)
    print("Log evidence", log_evd)
    lk.engine.close()


if __name__ == "__main__":
    main()
