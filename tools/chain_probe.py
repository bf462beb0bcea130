#!/usr/bin/env python3
"""Cost of the recorded chain and of emcee's diagnostics on the device; prints one JSON line.

* step time of the 4096-walker Pantheon+-shaped ensemble (reference move mixture) with and without recording, A/B
  interleaved in one process: ALTS alternations of STEPS steps each way, medians;
* integrated_time / gelman_rubin / percentile on a [2500, 4096, 4] AR(1) chain (tau ~ 32), device-synchronised wall time,
  median of REPS calls after one warm-up call;
* the numpy FFT restatement of emcee's integrated_time (tests/chain_reference.py) on the host copy of that chain, once.

    python tools/chain_probe.py [--alts 5] [--steps 200] [--reps 5] [--skip-numpy]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alts", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--skip-numpy", action="store_true")
    a = ap.parse_args()

    import chain_reference as ref

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("chain_probe needs an MI355X")
    dev = torch.device("cuda:0")
    W = a.walkers
    syn = amd.synthetic.pantheon_like(n_sn=1701, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    start = amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * np.random.default_rng(1).standard_normal((W, 4))
    f = lk.engine.torch_log_prob()
    plain = amd.ensemble.ShardedEnsemble(f, torch.from_numpy(start).to(dev), seed=3, moves=amd.ensemble.REFERENCE_MOVES)
    rec = amd.ensemble.ShardedEnsemble(f, torch.from_numpy(start).to(dev), seed=3, moves=amd.ensemble.REFERENCE_MOVES)
    plain.run(20)
    rec.run_mcmc(20)
    ms_plain, ms_rec = [], []
    for _ in range(a.alts):
        dt, _ = _timed(lambda: plain.run(a.steps))
        ms_plain.append(dt / a.steps * 1e3)
        dt, _ = _timed(lambda: rec.run_mcmc(a.steps))
        ms_rec.append(dt / a.steps * 1e3)
    same = bool(torch.equal(plain.x, rec.x) and torch.equal(plain.logp, rec.logp))

    x_host = ref.ar1_chain(2500, 4096, 4, 0.94, seed=3)
    x = torch.from_numpy(x_host).to(dev)
    cs = amd.chain_stats
    stats = {}
    for name, fn in (("integrated_time", lambda: cs.integrated_time(x)), ("gelman_rubin", lambda: cs.gelman_rubin(x)),
                     ("percentile", lambda: cs.percentile(x.reshape(-1, 4), [15.9, 50, 84.1]))):
        fn()
        stats[name] = float(np.median([_timed(fn)[0] for _ in range(a.reps)]) * 1e3)
    tau = cs.integrated_time(x)
    out = {
        "probe": "chain_probe", "walkers": W, "moves": "reference (KDE 0.30 + DE 0.70)", "n_sn": 1701,
        "step_ms_plain_median": float(np.median(ms_plain)), "step_ms_record_median": float(np.median(ms_rec)),
        "step_ms_plain": ms_plain, "step_ms_record": ms_rec, "alternations": a.alts, "steps_per_leg": a.steps,
        "record_overhead_frac": float(np.median(ms_rec) / np.median(ms_plain) - 1.0), "same_chain_bits": same,
        "stats_chain": [2500, 4096, 4], "stats_ms_median": stats, "reps": a.reps, "tau_device": tau.tolist(),
    }
    if not a.skip_numpy:
        t0 = time.perf_counter()
        tau_h, _, _, _ = ref.integrated_time(x_host)
        out["numpy_integrated_time_s"] = time.perf_counter() - t0
        out["tau_numpy"] = tau_h.tolist()
        out["tau_max_rel_diff"] = float(np.max(np.abs(tau / tau_h - 1)))
    print(json.dumps(out))
    lk.engine.close()


if __name__ == "__main__":
    main()
