#!/usr/bin/env python3
"""
cmb/cmb.py on the device sampler: the chain, its emcee blobs, the ``addDerived`` columns and the eight-parameter triangle,
without copying the chain to the host.

The script's run -- 200 walkers drawn uniformly in the box, KDEMove 15 % + DEMove 85 %, blobs (100 theta*, r*, D_M*, z*)
recorded beside the chain (cmb/cmb.py:45-63,80-93) -- on ``ensemble.ShardedEnsemble(..., blobs=spec)``; then what its
post-fit block does (:104-150): ``get_chain`` and ``get_blobs`` side by side, omega_m, Omega_m, z_drag, r_drag, z_eq added
(``derived.columns``), the printed 16 / 50 / 84 % values, and the numbers behind ``g.triangle_plot(params=[thetastar, H0,
omegam, DAstar, rstar, zstar, zdrag, rdrag])`` (``marginals.corner_data``) saved to an .npz.

    python examples/cmb_derived_triangle.py [--walkers 200] [--steps 3500] [--burn 500] [--out cmb_triangle.npz]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOBS = ["theta_star100", "rs_star", "DM_star", "z_star"]          # cmb/cmb.py:62-63 (D_M* in Mpc here, Gpc there)
DERIVED = ["omh2", "Om", "z_drag", "r_drag", "z_eq"]               # :118-138
TRIANGLE = ["theta_star100", "H0", "Om", "DM_star", "rs_star", "z_star", "z_drag", "r_drag"]  # :142


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=200)
    ap.add_argument("--steps", type=int, default=3500)
    ap.add_argument("--burn", type=int, default=500)
    ap.add_argument("--out", default="cmb_triangle.npz")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    amd = importlib.import_module("cosmology-model-fit_amd")
    D, M = amd.derived, amd.marginals
    lk = amd.likelihoods.CmbOnly()
    comp = lk.comp
    blobs = D.Spec(lk.engine, BLOBS)
    start = np.random.default_rng(42).uniform(lk.bounds[:, 0], lk.bounds[:, 1], (args.walkers, 3))  # :84-85
    ens = amd.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(dev), seed=42,
                                       moves=(("kde", 0.15), ("de", 0.85)), blobs=blobs)
    ens.run_mcmc(args.steps)
    chain = ens.get_chain(discard=args.burn, flat=True)                       # [n, 3]: H0, ombh2, omch2
    blob = ens.get_blobs(discard=args.burn, flat=True)                        # [n, 4]
    extra = D.columns(D.Spec(lk.engine, DERIVED, comp=comp), chain)           # [n, 5]
    table = torch.cat([chain, blob, extra], dim=1)
    names = ["H0", "obh2", "och2"] + BLOBS + DERIVED
    pct = amd.chain_stats.percentile(table, [15.9, 50.0, 84.1]).cpu().numpy()
    print(f"{args.walkers} walkers x {args.steps} steps, {args.burn} discarded, acceptance {ens.acceptance_fraction():.3f}")
    for j, n in enumerate(names):
        lo, med, hi = pct[:, j]
        print(f"  {n:14s} {med:.6g} +{hi - med:.3g} -{med - lo:.3g}")
    tri = table[:, [names.index(n) for n in TRIANGLE]].contiguous()
    m = M.corner_data(tri)
    np.savez(args.out, names=np.array(TRIANGLE), percentiles=pct, percentile_names=np.array(names), **m)
    print(f"saved the triangle of {TRIANGLE} ({sorted(m)}) to {args.out}")
    lk.engine.close()


if __name__ == "__main__":
    main()
