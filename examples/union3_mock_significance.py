#!/usr/bin/env python3
"""sn/union3_1.py (flat LCDM with the velocity step, real data of the golden fixture): the significance of the step, calibrated
by simulation, and the goodness of fit of chi^2_min (mocks.py).

The reference quotes sqrt(28.76 - 22.15) = 2.57 sigma (sn/union3_1.py:145,161): Wilks' theorem for one extra parameter.  Here
the same Delta chi^2 is placed in the distribution of Delta chi^2 over mock data sets drawn from the v = 0 best fit with the
data's own covariance, each fitted with and without the step on the device; the chi^2_min of the mocks gives the p-value of the
chi^2_min the script prints beside its DOF.

    python examples/union3_mock_significance.py [--mocks 4096]
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mocks", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX  # dM (-1, 1), om (0.1, 0.7), v (-9, 9) x 100 km/s
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    opt, M = amd.optimize, amd.mocks
    f = lk.engine.torch_log_prob(amd.CF_OUT_LOGL)  # log L = -chi^2 / 2

    fit = opt.best_fit(f, box, n_starts=32, seed=0)
    lcdm = opt.best_fit(f, box, n_starts=32, seed=0, fixed={2: 0.0})  # the null: v = 0
    observed = lcdm.chi2 - fit.chi2
    print(f"observed   chi2 (v free) = {fit.chi2:.3f}   chi2 (v = 0) = {lcdm.chi2:.3f}   Delta chi2 = {observed:.3f}   "
          f"(reference: 22.15, 28.76, sn/union3_1.py:145,161)")

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mocks = M.MockSet.draw(lk.engine, lcdm.x, a.mocks, seed=a.seed)  # data = model(v = 0 best fit) + noise of the covariance
    res = mocks.delta_chi2({2: 0.0}, n_starts=4, seed=a.seed)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0

    sig = M.significance(observed, res["delta_chi2"], k=1)
    dof = g["z_cmb"].size - 3
    gof = M.goodness_of_fit(fit.chi2, res["chi2_full"], dof=dof)
    lo, hi = sig["sigma_interval"]
    print(f"{a.mocks} mocks of the null, {res['n_like']} likelihood rows, {wall * 1e3:.0f} ms; mocks with Delta chi2 < -{res['tol']:g} "
          f"(optimizer failures): {res['n_below']}")
    print(f"mock Delta chi2: median {np.median(res['delta_chi2']):.3f}, 95 % {np.quantile(res['delta_chi2'], 0.95):.3f}   "
          f"(chi2 with one degree of freedom: 0.455, 3.841)")
    print(f"significance of the step   Wilks: {sig['wilks_sigma']:.2f} sigma (p = {sig['wilks_p']:.2e})   "
          f"calibrated: {sig['sigma']:.2f} sigma [{lo:.2f}, {hi:.2f}] (p = {sig['p']:.2e}, {sig['n_exceed']} of {sig['n_mocks']} mocks at "
          f"or above the observed value)")
    print(f"goodness of fit   chi2_min = {fit.chi2:.2f} for DOF = {dof}: Wilks p = {gof['wilks_p']:.3f}   "
          f"mocks p = {gof['p']:.3f} [{gof['p_interval'][0]:.3f}, {gof['p_interval'][1]:.3f}]")
    lk.engine.close()


if __name__ == "__main__":
    main()
