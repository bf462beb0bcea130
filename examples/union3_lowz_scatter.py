#!/usr/bin/env python3
"""Does the velocity step of sn/union3_1.py survive a free extra scatter of the low-z bins?  (real data of the golden fixture)

The reference reads its 2.57 sigma as "systematics in the standardisation of supernovae": the step sits where the low-z sample
ends.  The competing explanation is an error model that is wrong in the same place.  Here the covariance becomes
``C0 + sigma^2 diag(z <= 0.2)`` with ``sigma`` (an extra scatter in magnitudes, ``power = 2``) sampled beside (dM, om, v) --
``covscale.ScaledCovariance``: one diagonalisation on the host, no new Cholesky factor per likelihood call.

Printed: the significance of ``v`` from the two best fits with the covariance as published and with the extra scatter free
(a likelihood ratio; the second includes the log-determinant), the best-fit scatter, and from a device-resident ensemble the
posterior of the scatter and of ``v`` with and without it.

    python examples/union3_lowz_scatter.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")

Z_TURN = 0.2        # sn/union3_1.py
SIGMA_MAX = 0.3     # mag: the upper end of the flat prior of the extra scatter
WALKERS, STEPS, BURN = 64, 1500, 500


def _chain(log_prob, box, seed):
    start = torch.from_numpy(amd.synthetic.walkers(box, WALKERS, seed=seed)).to("cuda:0")
    ens = amd.ensemble.ShardedEnsemble(log_prob, start, seed=seed, moves=(("stretch", 1.0),))
    ens.run_mcmc(STEPS)
    return ens.get_chain(discard=BURN, flat=True).cpu().numpy()


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = np.asarray(amd.likelihoods.SnUnion3.PRIOR_BOX, dtype=np.float64)
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    opt = amd.optimize
    lowz = (g["z_cmb"] <= Z_TURN).astype(np.float64)
    print(f"{int(lowz.sum())} of {lowz.size} bins at z <= {Z_TURN} get the extra scatter")

    f0 = lk.engine.torch_log_prob(amd.CF_OUT_LOGL)
    free0 = opt.best_fit(f0, box, n_starts=32, seed=0)
    null0 = opt.best_fit(f0, box, n_starts=32, seed=0, fixed={2: 0.0})
    d0 = null0.chi2 - free0.chi2
    print(f"covariance as published:  -2 ln L (v = 0) - (v free) = {d0:.3f}  ({opt.sigma_from_delta_chi2(d0, 1):.2f} sigma), "
          f"v = {free0.x[2]:.3f}")

    with amd.covscale.ScaledCovariance(lk.engine, lowz, (0.0, SIGMA_MAX ** 2), power=2) as sc:
        box1 = np.vstack([box, [sc.p_bounds]])
        f1 = sc.torch_log_prob(amd.CF_OUT_LOGL)
        free1 = opt.best_fit(f1, box1, n_starts=32, seed=0)
        null1 = opt.best_fit(f1, box1, n_starts=32, seed=0, fixed={2: 0.0})
        d1 = null1.chi2 - free1.chi2
        print(f"extra low-z scatter free: -2 ln L (v = 0) - (v free) = {d1:.3f}  ({opt.sigma_from_delta_chi2(max(d1, 0.0), 1):.2f} sigma), "
              f"v = {free1.x[2]:.3f}, scatter = {free1.x[3]:.4f} mag (v free) / {null1.x[3]:.4f} mag (v = 0)")
        gain = free0.chi2 - free1.chi2
        print(f"what the scatter itself buys with v free: -2 Delta ln L = {gain:.3f} for one parameter on the boundary of its prior")

        with_s = _chain(sc.torch_log_prob(), box1, seed=3)
        without = _chain(lk.engine.torch_log_prob(), box, seed=3)
        q = np.percentile(with_s[:, 3], [50, 68, 95])
        print(f"\nposterior of the extra scatter (flat prior on [0, {SIGMA_MAX}] mag, {with_s.shape[0]} samples): "
              f"median {q[0]:.3f}, 68 % below {q[1]:.3f}, 95 % below {q[2]:.3f} mag")
        for name, ch in (("as published", without), ("scatter free", with_s)):
            lo, med, hi = np.percentile(ch[:, 2], [16, 50, 84])
            sd = ch[:, 2].std()
            print(f"v, {name:>13s}: {med:.3f} +{hi - med:.3f} -{med - lo:.3f}  (mean / std = {ch[:, 2].mean() / sd:.2f})")
    lk.engine.close()


if __name__ == "__main__":
    main()
