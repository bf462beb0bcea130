#!/usr/bin/env python3
"""Which of the 22 Union3 bins carry the Delta chi^2 of the velocity step (sn/union3_1.py, real data of the golden fixture).

The reference credits the preference for a velocity step to supernovae on either side of ``z_turn``.  Here the best fit with
``v`` free and the best fit with ``v = 0`` (``optimize.best_fit``), then ``influence.attribution``: ``delta_i = contrib_i(v = 0) -
contrib_i(v free)`` with ``contrib_i = r_i (C^-1 r)_i``, an exact additive split of the Delta chi^2 over the bins, listed against
redshift with its running sum; and under each model the bins whose leave-one-out z-scores (datum i against its prediction from
the 21 others) are largest.

    python examples/union3_step_attribution.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")

Z_TURN = 0.2  # sn/union3_1.py


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    opt, infl = amd.optimize, amd.influence
    f = lk.engine.torch_log_prob(amd.CF_OUT_LOGL)
    free = opt.best_fit(f, box, n_starts=32, seed=0)
    null = opt.best_fit(f, box, n_starts=32, seed=0, fixed={2: 0.0})
    dchi2 = null.chi2 - free.chi2
    print(f"chi2 (v free) = {free.chi2:.3f} at (dM, om, v) = {np.round(free.x, 4)}")
    print(f"chi2 (v = 0)  = {null.chi2:.3f} at (dM, om, v) = {np.round(null.x, 4)}")
    print(f"Delta chi^2   = {dchi2:.3f}  ({opt.sigma_from_delta_chi2(dchi2, 1):.2f} sigma for one parameter)")

    att = infl.attribution(lk.engine, null.x, free.x)
    print(f"\n{'bin':>3s} {'z':>8s} {'delta_i':>10s} {'running sum':>12s}")
    turned = False
    for k, (i, z, c) in enumerate(zip(att["order"], att["redshift"], att["cumulative"])):
        if z > Z_TURN and not turned:
            print(f"    ---- z_turn = {Z_TURN} ----")
            turned = True
        print(f"{i:3d} {z:8.4f} {att['delta'][i]:10.4f} {c:12.4f}")
    print(f"sum of delta_i = {att['delta'].sum():.6f}; chi2(v = 0) - chi2(v free) of the block = {att['total']:.6f}")

    sigma, loo_sigma = lk.engine.resid_sigma("sn"), lk.engine.precision("sn").loo_sigma()
    for name, fit in (("v free", free), ("v = 0", null)):
        r = infl.rows(lk.engine, fit.x, want=("z", "loo"))
        z, loo = r["z"][0].cpu().numpy(), r["loo"][0].cpu().numpy()
        top = np.argsort(-np.abs(z))[:5]
        print(f"\nlargest leave-one-out z-scores, {name} (chi2 without the first of them: "
              f"{float(r['sample']['chi2'][0] - r['sample']['max_drop'][0]):.3f}):")
        print(f"{'bin':>3s} {'z':>8s} {'z-score':>8s} {'loo resid':>10s} {'1/sqrt(K_ii)':>13s} {'sqrt(C_ii)':>11s}")
        for i in top:
            print(f"{i:3d} {g['z_cmb'][i]:8.4f} {z[i]:8.3f} {loo[i]:10.4f} {loo_sigma[i]:13.4f} {sigma[i]:11.4f}")
    lk.engine.close()


if __name__ == "__main__":
    main()
