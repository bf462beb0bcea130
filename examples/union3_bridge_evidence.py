#!/usr/bin/env python3
"""sn/union3_1.py (real data of the golden fixture): ln Z of the velocity-step model and of v = 0, four ways.

The reference ends its emcee fits with ``log_evidence(samples, log_probs, log_probability, bounds)``, a Gaussian integral around
the MAP.  Here the same chain gives ln Z by bridge sampling (``ShardedEnsemble.log_evidence``, both methods) with an error
bar, beside ``laplace.log_evidence`` on that chain and a ``DeviceNestedSampler`` run of the same likelihood and box, and the
Bayes factor of the step beside the 2.57 sigma (Delta chi^2 = 6.61 for one parameter) the scripts quote.

    python examples/union3_bridge_evidence.py [--walkers 64] [--steps 3000] [--discard 500] [--n-live 2000]
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
amd = importlib.import_module("cosmology-model-fit_amd")

QUOTED_SIGMA, QUOTED_DELTA_CHI2 = 2.57, 6.61
START = np.array([0.0, 0.3, -3.0])
SPREAD = np.array([0.02, 0.02, 1.0])


def engines(g):
    """(name, engine, box) of the step model (dM, Om, v) and of v = 0 (dM, Om) on the same data and box."""
    lk_mod = amd.likelihoods
    box = lk_mod.SnUnion3.PRIOR_BOX
    step = lk_mod.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box).engine
    flat = amd.LikelihoodEngine(
        ndim=2, z_max=float(np.max(g["z_cmb"]) + 0.1), n_grid=lk_mod.N_GRID, fde=amd.CF_FDE_LCDM,
        params=dict(offset=amd.Param(0), H0=amd.Param(fixed=float(g["H0"])), Om=amd.Param(1), v=amd.Param(fixed=0.0)),
        sn=dict(z_cmb=g["z_cmb"], z_hel=g["z_hel"], obs=g["obs"], chol=np.linalg.cholesky(g["cov"]), z_turn=0.2), bounds=box[:2])
    return [("step", step, box), ("v = 0", flat, box[:2])]


def evidences(name, eng, box, a):
    d = box.shape[0]
    rng = np.random.default_rng(3)
    start = START[:d] + SPREAD[:d] * rng.standard_normal((a.walkers, d))
    ens = amd.ensemble.ShardedEnsemble(eng.torch_log_prob(), torch.from_numpy(start).to("cuda:0"), seed=9,
                                       moves=amd.ensemble.REFERENCE_MOVES)
    ens.run_mcmc(a.steps)
    out = {m: ens.log_evidence(discard=a.discard, method=m, seed=1) for m in amd.evidence.METHODS}
    flat, logp = ens.get_chain(discard=a.discard, flat=True), ens.get_log_prob(discard=a.discard, flat=True)
    out["laplace"] = float(np.ravel(amd.laplace.log_evidence(flat.cpu().numpy(), logp.cpu().numpy(), eng.log_probability, box))[0])
    prior = amd.nested.Prior()
    for k in range(d):
        prior.add_parameter(("dM", "om", "v")[k], dist=(float(box[k, 0]), float(box[k, 1])))
    ns = amd.nested.DeviceNestedSampler(prior, eng.torch_log_prob(amd.CF_OUT_LOGL), n_live=a.n_live, seed=42)
    ns.run()
    out["nested"] = (ns.log_z, ns.log_z_err)
    print(f"\n{name}: {a.walkers} walkers x {a.steps} steps, {a.discard} discarded")
    for m in amd.evidence.METHODS:
        r = out[m]
        print(f"  bridge ({m:6s})  ln Z = {r.log_z:9.4f} +- {r.log_z_err:.4f}   {amd.evidence.STATUS_NAMES[r.status]} in {r.n_iter} "
              f"iterations, n_eff {r.n_eff:.0f} of {r.n_iter_rows}, {r.n_like} objective rows"
              + ("" if r.tau_reliable else "  (chain shorter than 50 tau)"))
    print(f"  Laplace          ln Z = {out['laplace']:9.4f}")
    print(f"  nested sampling  ln Z = {out['nested'][0]:9.4f} +- {out['nested'][1]:.4f}")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--discard", type=int, default=500)
    ap.add_argument("--n-live", type=int, default=2000)
    a = ap.parse_args(argv)
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    res = {}
    for name, eng, box in engines(g):
        res[name] = evidences(name, eng, box, a)
        eng.close()
    print("\nln B (step against v = 0):")
    for m in amd.evidence.METHODS:
        d, e = amd.evidence.log_bayes_factor(res["step"][m], res["v = 0"][m])
        print(f"  bridge ({m:6s})  {d:8.4f} +- {e:.4f}")
    print(f"  Laplace          {res['step']['laplace'] - res['v = 0']['laplace']:8.4f}")
    (zs, es), (z0, e0) = res["step"]["nested"], res["v = 0"]["nested"]
    print(f"  nested sampling  {zs - z0:8.4f} +- {float(np.hypot(es, e0)):.4f}")
    print(f"  the scripts quote {QUOTED_SIGMA} sigma for the step (Delta chi^2 = {QUOTED_DELTA_CHI2}, one parameter): a likelihood ratio "
          f"of exp({QUOTED_DELTA_CHI2 / 2:.2f}) at the best fit, before the prior volume of v is paid for")
    return res


if __name__ == "__main__":
    main()
