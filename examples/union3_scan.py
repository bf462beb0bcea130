#!/usr/bin/env python3
"""Which redshift step or window do the 22 Union3 bins prefer, and how significant is it after the search?

sn/union3_1.py quotes 2.57 sigma (Wilks) for a velocity step placed at z_turn = 0.2.  Here the question is asked of a whole
family on top of the fit without a step: every magnitude step (21 thresholds between the bins) and every window of consecutive
bins (253), each tried one at a time with the offset and the first-order refit of (dM, Omega_m) in the base
(``scan.TemplateScan``).  The winner, its local significance and the look-elsewhere-corrected p-value from null draws pushed
through the same kernel are printed beside the script's number.  A magnitude step is the linear stand-in of the script's
velocity step: the exact ``z_cosmo`` correction is not linear in v.

Then a hemisphere + cap scan on the directions of the Pantheon+ dipole fixture.  ITS COVARIANCE IS SYNTHETIC (the 20 MB matrix
is not stored with the fixture), so its numbers illustrate the calls, not the sky.

    python examples/union3_scan.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")


def _describe(c):
    if c["kind"] == "step":
        return f"step at z > {c['z_t']:.4f}"
    if c["kind"] == "window":
        return f"window {c['lo']:.4f} <= z < {c['hi']:.4f} ({c['bins']} bins)"
    if c["kind"] == "hemisphere":
        return "hemisphere about (%.3f, %.3f, %.3f)" % c["centre"]
    if c["kind"] == "cap":
        return "cap of %.0f deg about (%.3f, %.3f, %.3f)" % ((c["radius_deg"],) + c["centre"])
    return str(c)


def _print(sig, what):
    lo, hi = sig["p_interval"]
    print(f"{what}: {_describe(sig['candidate'])}")
    print(f"  amplitude {sig['alpha_hat']:+.4f} +- {sig['alpha_err']:.4f} mag, Delta chi^2 = {sig['best']:.3f}: {sig['local_sigma']:.2f} sigma local")
    print(f"  p_global = {sig['p_global']:.2e} [{lo:.2e}, {hi:.2e}] from {sig['n_draws']} null draws ({sig['n_exceed']} at or above): "
          f"{sig['sigma_global']:.2f} sigma; effective number of trials {sig['n_trials']:.1f}")


def union3():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    null = amd.optimize.best_fit(lk.engine.torch_log_prob(amd.CF_OUT_LOGL), box, n_starts=32, seed=0, fixed={2: 0.0})
    print(f"sn/union3_1.py without a step: chi2 = {null.chi2:.3f} at (dM, om, v) = {np.round(null.x, 4)}")
    Cd, z = amd.scan.Candidates, np.asarray(g["z_cmb"])
    zs = np.sort(z)
    edges = np.concatenate([[zs[0] * 0.99], 0.5 * (zs[1:] + zs[:-1]), [zs[-1] * 1.01]])
    family = Cd.stack(Cd.steps(z), Cd.windows(z, edges))
    with amd.scan.TemplateScan(lk.engine, family, base=np.ones(z.size), base_jacobian=null.x, jacobian_free=(0, 1)) as ts:
        print(f"{ts.K} candidates, {int(ts.info['live'].sum())} of them not spanned by the base "
              f"(offset + d r / d (dM, om): {ts.base.shape[1]} independent columns)")
        sig = ts.significance(null.x, n_draws=100000, seed=0)
        _print(sig, "best of every step and window")
        print("  sn/union3_1.py: 2.57 sigma (Wilks, one fixed alternative: the velocity step at z_turn = 0.2)")
        s = ts.map(null.x)[0]
        order = np.argsort(-np.where(ts.info["live"], s * s, -1.0))[:5]
        print("  the five largest Delta chi^2:")
        for k in order:
            print(f"    {s[k] ** 2:7.3f}  {_describe(ts.table[k])}")
    lk.engine.close()


def sky():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_pantheon_dipole_xyz.npz"))
    n = g["z_cmb"].size
    rng = np.random.default_rng(0)
    A = 0.01 * rng.standard_normal((n, 40))
    chol = np.linalg.cholesky(np.diag(np.asarray(g["sigma"]) ** 2) + A @ A.T)  # SYNTHETIC: diag(sigma^2) + a rank-40 term
    lk = amd.sn_pantheon.PantheonLikelihood(g["z_cmb"], g["z_hel"], g["obs"], chol=chol)
    theta = amd.optimize.best_fit(lk.engine.torch_log_prob(amd.CF_OUT_LOGL), amd.sn_pantheon.bounds, n_starts=8, seed=0).x
    Cd = amd.scan.Candidates
    centres = Cd.fibonacci_sphere(192)
    family = Cd.stack(Cd.hemispheres(g["dirs"], centres), Cd.caps(g["dirs"], centres, [20.0, 40.0, 60.0]))
    with amd.scan.TemplateScan(lk.engine, family, base=np.ones(n), base_jacobian=theta) as ts:
        print(f"\nPantheon+ directions, SYNTHETIC covariance: {ts.K} hemispheres and caps, {int(ts.info['live'].sum())} live")
        _print(ts.significance(theta, n_draws=20000, seed=0), "best sky patch")
    print("  (a dipole c_i (n_i . d) needs no scan: three columns of nuisance.LinearNuisance cover every direction)")
    lk.engine.close()


if __name__ == "__main__":
    union3()
    sky()
