#!/usr/bin/env python3
"""Where the time of ``evidence.bridge`` goes on a chain of production size; writes one JSON file.

Shape: the Pantheon+-shaped synthetic likelihood (sn/pantheon.py, 1701 SNe, 4 parameters) and a chain [2500, 4096, 4] of draws
around the truth with its log posterior recorded by the engine, as a sampler would hold it.  ``bridge`` runs with both methods.
HIP events on torch's current stream bracket every call of the objective (``cf_eval_device`` on exactly the rows the estimator
asks for, so the objective's time IS the cf_eval_device time of the same rows in the same run) and every call of the four
``cf_bridge_*`` entry points; two more bracket the whole call.  Recorded per method: the time in the objective, in each
kernel, their shares of the call, the solve's iterations and ``log_z_err``.  The probe records the outcome whatever it is.

    python tools/bridge_probe.py --out profiles/r17_bridge_probe.json
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

KERNELS = ("cf_bridge_forward", "cf_bridge_points", "cf_bridge_draw", "cf_bridge_solve")


class Timed:
    """Event pairs around calls, summed per name after a synchronise."""

    def __init__(self):
        self.pairs = []

    def wrap(self, name, fn):
        def timed(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(*args)
            b.record()
            self.pairs.append((name, a, b))
            return out

        return timed

    def totals(self):
        torch.cuda.synchronize()
        ms, calls = {}, {}
        for name, a, b in self.pairs:
            ms[name] = ms.get(name, 0.0) + a.elapsed_time(b)
            calls[name] = calls.get(name, 0) + 1
        self.pairs = []
        return ms, calls


class TimedLib:
    """The library with its cf_bridge_* entry points bracketed by events."""

    def __init__(self, lib, timed):
        self._lib = lib
        self._fns = {k: timed.wrap(k, getattr(lib, k)) for k in KERNELS}

    def __getattr__(self, name):
        return self._fns.get(name) or getattr(self._lib, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_bridge_probe.json"))
    ap.add_argument("--steps", type=int, default=2500)
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--n-sn", type=int, default=1701)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("bridge_probe needs an MI355X")
    ev, dev = amd.evidence, torch.device("cuda:0")
    syn = amd.synthetic.pantheon_like(n_sn=a.n_sn, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    eng = lk.engine
    f = eng.torch_log_prob()
    box = np.asarray(amd.sn_pantheon.bounds, dtype=np.float64)
    rng = np.random.default_rng(1)
    n = a.steps * a.walkers
    theta = amd.synthetic.THETA_TRUE + np.array([0.01, 0.3, 0.01, 0.1]) * rng.standard_normal((n, 4))
    chain = torch.from_numpy(theta).to(dev).reshape(a.steps, a.walkers, 4)
    log_probs = torch.cat([f(chain[t0:t0 + 16].reshape(-1, 4)) for t0 in range(0, a.steps, 16)]).reshape(a.steps, a.walkers)

    timed = Timed()
    objective = timed.wrap("objective", f)
    real = ev._require_gpu

    def require():
        L, lib = real()
        return L, TimedLib(lib, timed)

    ev._require_gpu = require
    out = {"probe": "bridge_probe", "n_sn": a.n_sn, "chain": [a.steps, a.walkers, 4], "info": eng.info()["gcn_arch"], "methods": {}}
    try:
        ev.bridge(objective, chain[:64], box[:, 0], box[:, 1], log_probs=log_probs[:64])  # warm-up
        timed.totals()
        for method in ev.METHODS:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = ev.bridge(objective, chain, box[:, 0], box[:, 1], log_probs=log_probs, method=method)
            t1.record()
            ms, calls = timed.totals()
            call_ms = t0.elapsed_time(t1)
            kernels = {k: ms.get(k, 0.0) for k in KERNELS}
            k_ms = sum(kernels.values())
            out["methods"][method] = {
                "call_ms": call_ms, "objective_ms": ms.get("objective", 0.0), "objective_calls": calls.get("objective", 0),
                "objective_rows": r.n_like, "bridge_kernels_ms": kernels, "bridge_kernels_total_ms": k_ms,
                "bridge_kernels_share_of_call": k_ms / call_ms, "objective_share_of_call": ms.get("objective", 0.0) / call_ms,
                "bridge_kernels_over_cf_eval_device_same_rows": k_ms / ms["objective"] if ms.get("objective") else None,
                "solve_iterations": r.n_iter, "status": ev.STATUS_NAMES[r.status], "log_z": r.log_z, "log_z_err": r.log_z_err,
                "n_iter_rows": r.n_iter_rows, "n_draws": r.n_draws, "n_eff": r.n_eff, "tau_f": r.tau_f, "tau_reliable": r.tau_reliable}
    finally:
        ev._require_gpu = real
        eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
