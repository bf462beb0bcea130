#!/usr/bin/env python3
"""What happens if you drop them: each of the 22 Union3 bins (sn/union3_1.py) and each DESI tracer (bao/desi.py) left out in turn,
from ONE device chain per data set and one pass over it -- no new engine, no new factor and no new sampling run per cut.

Per group: q at the best fit with its p-value (m degrees of freedom; Wilks-grade, the parameters were fitted with the group in),
the posterior mean of q, the shift of Omega_m and of the velocity step (w0 for DESI) in units of the full posterior's sigma when
the group is removed, the effective sample size of the reweighted chain and the Pareto tail index khat (>= 0.7: do not trust the
reweighted numbers, run the reduced data), next to ``influence.attribution``'s split of the step's Delta chi^2 over the same bins.
Then the check nobody should take on faith: the device ensemble run again on the engine REBUILT without one middle bin, printed
next to the reweighted answer, with both chains' effective sizes.

    python examples/union3_leaveout.py
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")
DEV = torch.device("cuda:0")


def sample(lk, box, n_walkers=64, n_steps=3000, seed=1):
    """A device ensemble on the mirror's log-probability, started around its best fit: (flat chain after burn-in, best fit, tau)."""
    fit = amd.optimize.best_fit(lk.engine.torch_log_prob(amd.CF_OUT_LOGL), box, n_starts=32, seed=0)
    rng = np.random.default_rng(seed)
    start = np.clip(fit.x[None, :] + 1e-3 * (box[:, 1] - box[:, 0])[None, :] * rng.standard_normal((n_walkers, box.shape[0])),
                    box[:, 0] + 1e-9, box[:, 1] - 1e-9)
    ens = amd.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(DEV), seed=seed)
    ens.run_mcmc(n_steps)
    tau = float(np.max(np.asarray(ens.get_autocorr_time(quiet=True)))) if hasattr(ens, "get_autocorr_time") else float("nan")
    return ens, fit, tau


def table(out, cols, labels, redshift, extra=None):
    head = f"{'group':>12s} {'z':>7s} {'m':>3s} {'q_ref':>8s} {'p_ref':>7s} {'<q>':>8s} " + " ".join(f"{'d' + c + '/s':>9s}" for c in labels) + \
           f" {'ESS':>9s} {'khat':>6s} {'ok':>3s}" + ("" if extra is None else f" {extra[0]:>10s}")
    print(head)
    for b, name in enumerate(out["names"]):
        line = f"{name:>12s} {redshift[b]:7.3f} {out['dof'][b]:3d} {out['q_ref'][b]:8.3f} {out['p_ref'][b]:7.3f} {out['q_mean'][b]:8.3f} " + \
               " ".join(f"{out['shift_sigma'][b, c]:9.3f}" for c in cols) + \
               f" {out['ess'][b]:9.0f} {out['khat'][b]:6.2f} {'yes' if out['reliable'][b] else 'NO':>3s}"
        print(line + ("" if extra is None else f" {extra[1][b]:10.4f}"))


def main():
    LO, infl = amd.leaveout, amd.influence
    # ---- sn/union3_1.py: the 22 bins --------------------------------------------------------------------------------------------
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    ens, fit, tau = sample(lk, box)
    null = amd.optimize.best_fit(lk.engine.torch_log_prob(amd.CF_OUT_LOGL), box, n_starts=32, seed=0, fixed={2: 0.0})
    att = infl.attribution(lk.engine, null.x, fit.x)
    groups, names = LO.groups_from_labels(np.arange(g["z_cmb"].size))
    out = ens.leave_group_out(discard=500, groups=groups, names=[f"bin{n}" for n in names], theta_ref=fit.x)
    n_rows = out["q"].shape[0]
    print(f"sn/union3_1.py: {n_rows} chain rows (tau ~ {tau:.0f} steps), chi2_min = {fit.chi2:.3f} at (dM, om, v) = {np.round(fit.x, 4)}")
    print(f"full posterior: om = {out['mean_full'][1]:.4f} +- {out['std_full'][1]:.4f}, v = {out['mean_full'][2]:.3f} +- {out['std_full'][2]:.3f}")
    table(out, (1, 2), ("om", "v"), g["z_cmb"], ("delta_i", att["delta"]))
    print("delta_i: influence.attribution's share of the step's Delta chi^2 = %.3f carried by the bin" % att["total"])

    # the direct answer for one middle bin: the same sampler on the engine rebuilt without it
    drop = int(np.argsort(g["z_cmb"])[g["z_cmb"].size // 2])
    keep = np.setdiff1d(np.arange(g["z_cmb"].size), [drop])
    assert drop != int(np.argmax(g["z_cmb"]))  # the top redshift sets the integration grid: keep it
    sub = amd.likelihoods.SnUnion3(g["z_cmb"][keep], g["z_hel"][keep], g["obs"][keep], g["cov"][np.ix_(keep, keep)],
                                   H0=float(g["H0"]), bounds=box)
    ens_sub, _, tau_sub = sample(sub, box, seed=2)
    direct = ens_sub.get_chain(discard=500, flat=True)
    mean_d, std_d = direct.mean(dim=0).cpu().numpy(), direct.std(dim=0).cpu().numpy()
    print(f"\nwithout bin{drop} (z = {g['z_cmb'][drop]:.3f}):           om                 v")
    print(f"  reweighted full chain : {out['mean'][drop, 1]:.4f} +- {out['std'][drop, 1]:.4f}   {out['mean'][drop, 2]:.3f} +- {out['std'][drop, 2]:.3f}"
          f"   (importance ESS {out['ess'][drop]:.0f} of {n_rows} rows, khat {out['khat'][drop]:.2f}; chain tau ~ {tau:.0f})")
    print(f"  direct run, rebuilt   : {mean_d[1]:.4f} +- {std_d[1]:.4f}   {mean_d[2]:.3f} +- {std_d[2]:.3f}"
          f"   ({direct.shape[0]} rows, tau ~ {tau_sub:.0f}: about {direct.shape[0] / max(tau_sub, 1.0):.0f} independent)")
    lk.engine.close()
    sub.engine.close()

    # ---- bao/desi.py: the tracers ---------------------------------------------------------------------------------------------
    d = np.load(os.path.join(ROOT, "tests", "golden", "bao_desi.npz"))
    bao = amd.likelihoods.DesiBao(d["bao_z"], d["bao_val"], d["bao_qty"], d["bao_inv_cov"])
    ens, fit, tau = sample(bao, bao.bounds)
    groups, names = LO.groups_from_labels(np.asarray(d["bao_z"]))
    out = ens.leave_group_out(discard=500, groups=groups, block="bao", names=[f"z={n}" for n in names], theta_ref=fit.x)
    print(f"\nbao/desi.py: {out['q'].shape[0]} chain rows (tau ~ {tau:.0f}), chi2_min = {fit.chi2:.3f} at (h, om, w0) = {np.round(fit.x, 4)}")
    print(f"full posterior: om = {out['mean_full'][1]:.4f} +- {out['std_full'][1]:.4f}, w0 = {out['mean_full'][2]:.3f} +- {out['std_full'][2]:.3f}")
    table(out, (1, 2), ("om", "w0"), [float(n) for n in names])
    bao.engine.close()


if __name__ == "__main__":
    main()
