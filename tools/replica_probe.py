#!/usr/bin/env python3
"""Time one step of a replica ensemble against the two things it replaces, on the Pantheon-shaped likelihood (N = 1701, ndim 4).

  (a) ``replicas.ReplicaEnsemble`` of R ensembles of w walkers;
  (b) the same R ensembles as stand-alone ``ensemble.ShardedEnsemble``s, run one after another;
  (c) one ``ShardedEnsemble`` of R w walkers
at (R, w) = (27, 150), (16, 256), (1, 4096), for the stretch move, the DE move and the reference's KDE / DE mix.  The DE move
runs by thirds where 3 divides w and by halves elsewhere (the JSON says which).  Everything is warmed up first; then the three
are timed in turn, round after round, in one process, each block of steps between two device events; the figure is the median
over the rounds of the block's time per step.  (b) and (c) are existing code: they are what (a) is judged against.

    python tools/replica_probe.py [--out profiles/r19_replica_probe.json] [--steps 20] [--rounds 7]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = np.array([(-19.6, -19.1), (60.0, 80.0), (0.15, 0.5), (-2.0, 2.0)])  # inside sn/pantheon.py's box, where log P is finite
SHAPES = [(27, 150), (16, 256), (1, 4096)]


def timed(fn, n_steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(n_steps)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n_steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_replica_probe.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n-sn", type=int, default=1701)
    args = ap.parse_args()

    pkg = importlib.import_module("cosmology-model-fit_amd")
    E, RP = pkg.ensemble, pkg.replicas
    dev = torch.device("cuda:0")
    syn = pkg.synthetic.pantheon_like(n_sn=args.n_sn, seed=3)
    lk = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    f = lk.engine.torch_log_prob()
    rows = []
    for R, w in SHAPES:
        x = torch.from_numpy(pkg.synthetic.walkers(BOX, R * w, seed=R).reshape(R, w, 4)).to(dev)
        for name, moves in (("stretch", E.STRETCH_ONLY), ("de", (("de", 1.0),)), ("mix", E.REFERENCE_MOVES)):
            de_splits = 3 if w % 3 == 0 else 2
            kw = dict(seed=9, moves=moves, de_splits=de_splits)
            a = RP.ReplicaEnsemble(f, x, **kw)
            b = [E.ShardedEnsemble(f, x[r], **kw) for r in range(R)]
            c = E.ShardedEnsemble(f, x.reshape(R * w, 4), **kw)

            def run_b(n):
                for e in b:
                    e.run(n)

            runs = {"replica": a.run, "one_after_another": run_b, "one_big": c.run}
            for fn in runs.values():
                fn(5)
            torch.cuda.synchronize()
            ms = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    ms[k].append(timed(fn, args.steps))
            med = {k: statistics.median(v) for k, v in ms.items()}
            row = {"R": R, "w": w, "move": name, "de_splits": de_splits, "steps_per_block": args.steps, "rounds": args.rounds,
                   "ms_per_step": med, "ms_per_step_min": {k: min(v) for k, v in ms.items()},
                   "ms_per_step_max": {k: max(v) for k, v in ms.items()},
                   "replica_over_one_big": med["replica"] / med["one_big"],
                   "replica_over_one_after_another": med["replica"] / med["one_after_another"],
                   "accept": {"replica": float(a.acceptance_fraction().mean()), "one_big": c.acceptance_fraction()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    lk.engine.close()
    out = {"what": "ms per ensemble step, device events, median over interleaved rounds; see tools/replica_probe.py",
           "n_sn": args.n_sn, "ndim": 4, "device": torch.cuda.get_device_name(0), "rows": rows}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
