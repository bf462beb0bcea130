#!/usr/bin/env python3
"""
A posterior-predictive D_V / r_d band for bao/desi.py, from a device-resident chain.

bao/desi.py (DESI BAO alone, theta = (h, Om, w0), thawing dark energy, r_d = 147.09 Mpc; the data of the golden fixture) on
the device sampler, then ``derived.bands``: D_V(z) / r_d of EVERY stored sample on the 200 redshifts of
``plot_bao_predictions`` (bao/plot_predictions.py:23), reduced to the 16 / 50 / 84 % envelope on the device -- where the
script draws the single curve of its best fit (bao/desi.py:204-211).  The band and the best-fit curve are saved to an .npz.

    python examples/desi_dv_band.py [--walkers 512] [--steps 600] [--burn 200] [--out desi_dv_band.npz]
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
    ap.add_argument("--walkers", type=int, default=512)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--burn", type=int, default=200)
    ap.add_argument("--out", default="desi_dv_band.npz")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    amd = importlib.import_module("cosmology-model-fit_amd")
    g = np.load(os.path.join(ROOT, "tests", "golden", "bao_desi.npz"))
    lk = amd.likelihoods.DesiBao(g["bao_z"], g["bao_val"], g["bao_qty"], g["bao_inv_cov"])
    start = np.array([0.68, 0.31, -0.85]) + np.array([0.01, 0.01, 0.05]) * np.random.default_rng(1).standard_normal((args.walkers, 3))
    ens = amd.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(dev), seed=7,
                                       moves=amd.ensemble.REFERENCE_MOVES)
    ens.run_mcmc(args.steps)
    samples = ens.get_chain(discard=args.burn, flat=True)
    best_fit = ens.percentile(50, discard=args.burn).cpu().numpy()
    z = np.linspace(0, float(np.max(g["bao_z"])), 200)
    band = amd.derived.bands(lk.engine, samples, z, "DV_rd")
    curve = lk.bao_theory(z, 0, best_fit)
    np.savez(args.out, best_fit=best_fit, best_fit_curve=curve, **band)
    k = [50, 100, 199]
    print(f"{samples.shape[0]} samples; best fit (h, Om, w0) = {best_fit}")
    for i in k:
        lo, med, hi = band["bands"][:, i]
        print(f"  z = {z[i]:.3f}: D_V / r_d = {med:.4f} +{hi - med:.4f} -{med - lo:.4f}   (best-fit curve {curve[i]:.4f})")
    print(f"saved z, q, bands [3, 200], mean, std, best_fit_curve to {args.out}")
    lk.engine.close()


if __name__ == "__main__":
    main()
