#!/usr/bin/env python3
"""
ohd/cc_gp.py on the device: a model-independent H(z) from the 38 cosmic chronometers.

The script's 5000 Adam steps become one ``HubbleGP.fit()`` (the type-II maximum in the box), and where the script stops at
that point estimate, a 64-walker chain over the four hyperparameters gives the band of H(z), H0 = H(0) and q(z) marginalised
over them (``HubbleGP.marginal_predict``).  Saved to an .npz: z*, the H band at the fit and marginalised, q(z), H0 +- sigma
and the hyperparameter summary.  No plotting.

    python examples/cc_gp_reconstruction.py [--steps 1500] [--burn 500] [--out cc_gp_reconstruction.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--burn", type=int, default=500)
    ap.add_argument("--out", default="cc_gp_reconstruction.npz")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    amd = importlib.import_module("cosmology-model-fit_amd")
    d = np.load(os.path.join(ROOT, "tests", "golden", "ohd_cc.npz"))
    g = amd.gp.HubbleGP(d["cc_z"], d["cc_h"], d["cc_cov"])
    fit = g.fit()
    mean, out_scale, length, noise_scale = g.physical(fit.x)
    print(f"type-II maximum: log ML = {fit.log_prob:.4f} | mean {mean:.2f} | output scale {out_scale:.1f} | "
          f"length scale {length:.4f} | noise scale {noise_scale:.4f}")

    z_star = np.linspace(0.0, float(np.max(d["cc_z"])), 100)  # cc_gp.py:75
    at_fit = g.predict(fit.x, z_star, noise=1e-4)             # cc_gp.py:76
    print(f"H0 at the fit: {at_fit['mean'][0]:.1f} +- {at_fit['std'][0]:.1f} km/s/Mpc")

    b = g.bounds
    w = b[:, 1] - b[:, 0]
    lo, hi = np.maximum(b[:, 0] + 1e-3 * w, fit.x - 0.1 * w), np.minimum(b[:, 1] - 1e-3 * w, fit.x + 0.1 * w)
    start = lo + np.random.default_rng(1).uniform(0.0, 1.0, (args.walkers, 4)) * (hi - lo)
    ens = amd.ensemble.ShardedEnsemble(g.torch_log_prob(), torch.from_numpy(start).to(dev), seed=7)
    ens.run_mcmc(args.steps)
    samples = ens.get_chain(discard=args.burn, flat=True)
    pct = g.physical(ens.percentile([15.9, 50.0, 84.1], discard=args.burn).cpu().numpy())
    band = g.marginal_predict(samples, z_star, noise=1e-4)
    print(f"{samples.shape[0]} samples, acceptance {ens.acceptance_fraction():.2f}")
    for name, col in zip(amd.gp.NAMES, pct.T):
        print(f"  {name}: {col[1]:.4g} +{col[2] - col[1]:.3g} -{col[1] - col[0]:.3g}")
    print(f"H0 marginalised over the hyperparameters: {band['H0'][0]:.1f} +- {band['H0'][1]:.1f} km/s/Mpc")
    np.savez(args.out, z=z_star, fit_theta=fit.x, fit_physical=g.physical(fit.x), fit_log_ml=fit.log_prob,
             H_fit=at_fit["mean"], H_fit_std=at_fit["std"], q_fit=at_fit["q"],
             H=band["mean"], H_std=band["std"], dH=band["dmean"], dH_std=band["dstd"], q=band["q"], H0=np.array(band["H0"]),
             hyper_percentiles=pct, hyper_names=np.array(amd.gp.NAMES))
    print(f"saved z, H +- H_std (1 sigma; 2 sigma is twice that), q, H0 and the hyperparameter summary to {args.out}")
    g.close()


if __name__ == "__main__":
    main()
