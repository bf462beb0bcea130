#!/usr/bin/env python3
"""Cost of the device nested sampler; writes one JSON (and prints it).

* union3: sn/union3_1.py on the golden real-data fixture, n_live = 7000, seed 42 (examples/union3_nested.py);
* pantheon: a Pantheon-shaped synthetic run (synthetic.pantheon_like, N = 1701, 4 parameters, the sn/pantheon.py box as
  uniform priors, log L only), n_live = 6000 (k = 3000 walkers per likelihood call).
Per run: device-synchronised wall time of run(), n_like, iterations, walk acceptance, likelihood evaluations per second of
the walk (walk evaluations / wall time of run(): the sorts, row moves and host bookkeeping included), log Z +- err.

The kernel share comes from a separate rocprofv3 run of the Pantheon-shaped case; ``--share`` folds its stats CSV into the
JSON: the cf_ns_* kernels' device time against the likelihood kernels' (and torch's sort / row moves, listed apart).

    python tools/nested_probe.py --out profiles/r06_nested_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/nested_probe.py --only pantheon --out /dev/null
    python tools/nested_probe.py --share DIR/.../*_kernel_stats.csv --out profiles/r06_nested_probe.json
"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NS_KERNELS = ("ns_prior_draw_kernel", "ns_transform_kernel", "ns_walk_start_kernel", "ns_propose_kernel", "ns_accept_kernel")


def _run(amd, name, prior, f, n_live, seed):
    s = amd.nested.DeviceNestedSampler(prior, f, n_live=n_live, seed=seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reached = s.run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c = s.walk_counts()
    return {"case": name, "n_live": n_live, "n_batch": s.n_batch, "n_walk": s.n_walk, "seed": seed, "f_live_reached": reached,
            "run_wall_s": wall, "n_like": s.n_like, "iterations": s.n_iterations, "acceptance": s.acceptance,
            "walk_evals": c["proposed"], "walk_evals_per_s": c["proposed"] / wall, "out_of_cube": c["out_of_cube"],
            "log_z": s.log_z, "log_z_err": s.log_z_err, "n_eff": s.n_eff}


def union3(amd):
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    p = amd.nested.Prior()
    for key, (lo, hi) in zip(("dM", "om", "v"), box):
        p.add_parameter(key, dist=(float(lo), float(hi)))
    out = _run(amd, "union3_1 (real data, N = 22)", p, lk.engine.torch_log_prob(amd.CF_OUT_LOGL), 7000, 42)
    lk.engine.close()
    return out


def pantheon(amd):
    syn = amd.synthetic.pantheon_like(n_sn=1701, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    p = amd.nested.Prior()
    for key, (lo, hi) in zip(("M", "H0", "Om", "v"), amd.sn_pantheon.bounds):
        p.add_parameter(key, dist=(float(lo), float(hi)))
    out = _run(amd, "pantheon_like (synthetic, N = 1701)", p, lk.engine.torch_log_prob(amd.CF_OUT_LOGL), 6000, 42)
    lk.engine.close()
    return out


def share(path):
    """Device time of the cf_ns_* kernels against the likelihood kernels from a rocprofv3 kernel_stats.csv."""
    ns, other, rows = 0.0, 0.0, {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name, tot = r["Name"], float(r["TotalDurationNs"])
            rows[name[:90]] = {"calls": int(r["Calls"]), "total_ms": tot * 1e-6, "avg_us": float(r["AverageNs"]) * 1e-3}
            if any(k in name for k in NS_KERNELS):
                ns += tot
            elif not any(t in name for t in ("at::", "void at", "rocprim", "hipcub", "elementwise", "sort", "index")):
                other += tot
    torch_ms = sum(v["total_ms"] for k, v in rows.items() if not any(t in k for t in NS_KERNELS)) - other * 1e-6
    return {"ns_kernels_ms": ns * 1e-6, "likelihood_kernels_ms": other * 1e-6, "torch_kernels_ms": torch_ms,
            "ns_share_of_walk": ns / (ns + other), "target": 0.10, "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("union3", "pantheon"), default=None)
    ap.add_argument("--share", default=None, help="rocprofv3 kernel_stats.csv of a `--only pantheon` run to fold in")
    a = ap.parse_args()
    if a.share:
        out = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        out["kernel_share_pantheon"] = share(a.share)
    else:
        amd = importlib.import_module("cosmology-model-fit_amd")
        if amd.lib().cf_device_count() < 1:
            sys.exit("nested_probe needs an MI355X")
        runs = [fn(amd) for key, fn in (("union3", union3), ("pantheon", pantheon)) if a.only in (None, key)]
        out = {"probe": "nested_probe", "device": torch.cuda.get_device_name(0), "runs": runs}
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
