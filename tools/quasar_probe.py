#!/usr/bin/env python3
"""Cost of the quasar Hubble-diagram likelihoods (quasars.py, csrc/cosmofit_quasar.hip); writes one JSON (and prints it).

Per script, on its fixture's data (tests/golden/qsr_*.npz: the real columns, the seeded synthetic SN covariance where the
matrix is not in the snapshot) and W = 20, 256, 1024, 4096, 8192 in-box walkers:
  * per-kernel device time from the handle's timing events (cf_kernel_ms3: the per-walker kernel, the solve + epilogue or
    finalize_kernel), median over 50 device-resident calls;
  * evals/s = W / (device-synchronised wall time per cf_eval_device call, median of 50);
  * the latency of a synchronous 20-walker host call (lk.log_probability: emcee's half-step for these scripts), median of 200;
  * the numpy restatement (tests/quasar_reference.py) on the same host at W = 20: seconds per call.

    python tools/quasar_probe.py --out profiles/r07_quasar_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import quasar_reference as ref  # noqa: E402
from conftest import golden, load_pkg, synthetic_cov  # noqa: E402

WS = (20, 256, 1024, 4096, 8192)


def _walkers(bounds, W, seed=0):
    b = np.asarray(bounds, float)
    lo, hi = b[:, 0] + 0.05 * (b[:, 1] - b[:, 0]), b[:, 1] - 0.05 * (b[:, 1] - b[:, 0])
    return np.random.default_rng(seed).uniform(lo, hi, size=(W, len(b)))


def probe(pkg, name, reps=50):
    g = dict(golden(name))
    qsr, sn, bao = ref.fixture_data(g, synthetic_cov)
    lk = pkg.quasars.build(ref.SCRIPTS[name], qsr=qsr, sn=sn, bao=bao)
    eng = lk.engine
    out = dict(n_qsr=int(len(qsr[0])), n_sn=int(len(sn[0])) if sn else 0, n_bao=int(len(bao[1])) if bao else 0, by_w={})
    f = eng.torch_log_prob()
    for W in WS:
        th = torch.from_numpy(_walkers(lk.bounds, W)).to("cuda")
        for _ in range(5):
            f(th)
        torch.cuda.synchronize()
        eng.enable_timing(reps)
        walls = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f(th)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        t3 = np.array(eng.kernel_ms3())
        eng.enable_timing(0)
        wall = float(np.median(walls))
        out["by_w"][str(W)] = dict(walker_kernel_us=float(np.median(t3[:, 0]) * 1e3), solve_or_finalize_us=float(np.median(t3[:, 2]) * 1e3),
                                   wall_us_per_call=wall * 1e6, evals_per_s=W / wall)
    th20 = _walkers(lk.bounds, 20, seed=1)
    for _ in range(20):
        lk.log_probability(th20)
    lat = []
    for _ in range(200):
        t0 = time.perf_counter()
        lk.log_probability(th20)
        lat.append(time.perf_counter() - t0)
    out["sync_20_walker_call_us"] = float(np.median(lat) * 1e6)
    r = pkg.quasars.RECIPES[ref.SCRIPTS[name]]
    rec = dict(theta=r.theta, nkp=r.nkp, bounds=r.bounds, sn_grid=r.sn_grid, sn_zhel=r.sn_zhel)
    b = None if bao is None else (bao[0]["z"], bao[0]["value"], bao[0]["quantity"], bao[1])
    t0 = time.perf_counter()
    for _ in range(3):
        ref.evaluate(rec, th20, qsr, sn, b)
    out["cpu_restatement_20_walkers_s"] = (time.perf_counter() - t0) / 3
    lk.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r07_quasar_probe.json")
    a = ap.parse_args()
    pkg = load_pkg()
    res = dict(device=torch.cuda.get_device_name(0), cases={})
    for name in ref.CASES:
        res["cases"][name] = probe(pkg, name)
        print(name, json.dumps(res["cases"][name]), flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
