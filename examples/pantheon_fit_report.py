#!/usr/bin/env python3
"""
The report block every script of the reference ends with, for every sample of a device-resident chain.

A short ensemble chain on the Pantheon+-shaped flat-LambdaCDM likelihood (the reference's move mixture, sn/pantheon.py:114-117),
then ``ens.fit_report(discard=...)``: the lines sn/pantheon.py:171-183 prints -- R-squared, RMSD, skewness and kurtosis of the
residuals, degrees of freedom, chi squared -- evaluated at the median of the chain as the script does, each with the 15.9 / 50 /
84.1 percentiles it takes over the posterior; and, for the residual plot (sn/plotting.py:46-71), the posterior mean and scatter
of every supernova's residual, its sqrt(C_ii), and the fraction of the posterior in which it lies beyond 2 and 3 sigma.  The
residual rows never leave the device; the arrays of the plot are saved to an .npz.

    python examples/pantheon_fit_report.py [--walkers 1024] [--steps 400] [--burn 100] [--out pantheon_fit_report.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--out", default="pantheon_fit_report.npz")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    amd = importlib.import_module("cosmology-model-fit_amd")
    syn = amd.synthetic.pantheon_like(n_sn=args.n_sn, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    rng = np.random.default_rng(1)
    start = amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * rng.standard_normal((args.walkers, 4))
    ens = amd.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(dev), seed=7,
                                       moves=amd.ensemble.REFERENCE_MOVES)
    ens.run_mcmc(args.steps)
    rep = ens.fit_report(discard=args.burn, thresholds=(2.0, 3.0))  # centre: the median, sn/pantheon.py:150
    s, d = rep["summary"], rep["datum"]

    def line(key, name, scale=1.0, fmt=".3f"):
        lo, med, hi = scale * s["posterior"][name]
        print(f"{key}: {scale * s['at_center'][name]:{fmt}}   (over the posterior {med:{fmt}} +{hi - med:{fmt}} -{med - lo:{fmt}})")

    print(f"{args.walkers} walkers x {args.steps} steps, {args.burn} discarded: {rep['stats'].shape[0]} samples, "
          f"{d['sigma'].size} supernovae")
    for c, n in enumerate(("M", "H0", "Om", "v")):
        print(f"{n}: {s['center'][c]:.4f}")
    line("R-squared (%)", "r2", 100.0, ".2f")
    line("RMSD (mag)", "rmsd")
    line("Skewness of residuals", "skew")
    line("kurtosis of residuals", "kurtosis")
    print("Degs of freedom:", s["dof"])
    print(f"Chi squared: {s['chi2']:.2f}")
    line("normal fit of the residuals, mean", "mean", fmt=".4f")
    line("normal fit of the residuals, std", "std", fmt=".4f")
    often = d["exceed"][1] > 0.5
    print(f"beyond 3 sigma in most of the posterior: {int(often.sum())} supernovae"
          + (f" (z = {', '.join(f'{z:.4f}' for z in d['z'][often][:8])}{' ...' if often.sum() > 8 else ''})" if often.any() else ""))
    np.savez(args.out, z=d["z"], sigma=d["sigma"], residual_mean=d["mean"], residual_std=d["std"], pull_mean=d["pull_mean"],
             thresholds=d["thresholds"], exceed=d["exceed"], n_used=d["n_used"], n_skipped=d["n_skipped"], center=s["center"],
             columns=np.array(rep["columns"]), stats_q=np.array([s["posterior"][c] for c in rep["columns"][:-1]]))
    print(f"saved the residual-plot arrays to {args.out}")
    lk.engine.close()


if __name__ == "__main__":
    main()
