#!/usr/bin/env python3
"""Cost of the batched maximizer (optimize.py); writes one JSON (and prints it).

Cases, each on the engine's log L (the Pantheon-shaped case on its log P, which carries the Gaussian H0 prior):
* union3: sn/union3_1.py on the golden real-data fixture: best fit with 32 starts, the v = 0 fit (32 starts), a 64 x 8 profile of v;
* desi: bao/desi.py on its golden fixture: a 64 x 16 profile of w0 and a 32 x 32 x 4 profile of (Om, w0);
* pantheon: synthetic.pantheon_like (N = 1701, 4 parameters, sn/pantheon.py's box and H0 prior): best fit with 64 starts and a
  64 x 16 profile of Om.
Per call: device-synchronised wall time, device iterations, likelihood rows and rows/s, the status histogram.  Per case the
host-serial path -- scipy L-BFGS-B with laplace.gradient stencils (one synchronous 2n + 1 row call per evaluation) on the same
engine -- on 16 problems of the same kind, timed, then extrapolated to the call's problem count (labelled as extrapolated).

The kernel share comes from a separate rocprofv3 run of the Pantheon-shaped profile; ``--share`` folds its stats CSV in: the
cf_opt_* kernels' device time against the likelihood kernels' (torch's elementwise / copy kernels listed apart).

    python tools/opt_probe.py --out profiles/r08_opt_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/opt_probe.py --only pantheon --out /dev/null
    python tools/opt_probe.py --share DIR/.../*_kernel_stats.csv --out profiles/r08_opt_probe.json
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
OPT_KERNELS = ("opt_starts_kernel", "opt_stencil_kernel", "opt_direction_kernel", "opt_accept_kernel", "opt_compact_kernel")


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def _summary(res, wall, label, problems):
    return {"call": label, "problems": problems, "wall_s": wall, "iterations": res.iterations, "likelihood_calls": res.n_calls,
            "likelihood_rows": res.n_like, "rows_per_s": res.n_like / wall, "status": res.status_counts(),
            "max_n_iter": int(res.n_iter.max())}


def _host_serial(amd, lk, box, x0, free):
    """scipy L-BFGS-B over the free coordinates with laplace.gradient stencils on the engine (host numpy, synchronous)."""
    from scipy.optimize import minimize

    h = 1e-6 * (box[:, 1] - box[:, 0])
    free = list(free)

    def run(start):
        def fg(z):
            t = start.copy()
            t[free] = z
            val, grad = amd.laplace.gradient(lambda pts: lk.engine.log_likelihood(pts), t, h)
            if not np.isfinite(val) or not np.all(np.isfinite(grad)):
                return 1e10, np.zeros(len(free))
            return -val, -grad[free]

        return minimize(fg, x0=start[free], jac=True, bounds=box[free], method="L-BFGS-B")

    t0 = time.perf_counter()
    nfev = sum(run(np.array(s, dtype=np.float64)).nfev for s in x0)
    return time.perf_counter() - t0, nfev


def _case(amd, name, lk, f, box, calls, serial_free):
    out = {"case": name, "calls": []}
    opt = amd.optimize
    for label, fn, problems in calls:
        fn()  # warm-up: workspace growth, first launches
        res, wall = _timed(fn)
        row = _summary(res.problems if hasattr(res, "problems") else res, wall, label, problems)
        if hasattr(res, "chi2"):
            row["chi2"] = res.chi2
        if hasattr(res, "delta_chi2") and len(res.index) == 1:
            row["interval_dchi2_1"] = res.interval(1.0)
        out["calls"].append(row)
    rng = np.random.default_rng(0)
    x0 = rng.uniform(box[:, 0] + 0.05 * (box[:, 1] - box[:, 0]), box[:, 1] - 0.05 * (box[:, 1] - box[:, 0]), (16, box.shape[0]))
    t16, nfev = _host_serial(amd, lk, box, x0, serial_free)
    out["host_serial_16"] = {"wall_s": t16, "evaluations": nfev, "per_problem_s": t16 / 16}
    for row in out["calls"]:
        row["host_serial_extrapolated_s"] = t16 / 16 * row["problems"]
        row["speedup_vs_host_serial_extrapolated"] = row["host_serial_extrapolated_s"] / row["wall_s"]
    del opt
    return out


def union3(amd):
    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX
    lk = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    f, opt = lk.engine.torch_log_prob(amd.CF_OUT_LOGL), amd.optimize
    best = opt.best_fit(f, box, n_starts=32, seed=0)
    calls = [("best_fit 32 starts", lambda: opt.best_fit(f, box, n_starts=32, seed=0), 32),
             ("v = 0 fit 32 starts", lambda: opt.best_fit(f, box, n_starts=32, seed=0, fixed={2: 0.0}), 32),
             ("profile of v 64 x 8", lambda: opt.profile(f, box, 2, np.linspace(-8.5, 8.5, 64), n_starts=8, best=best), 512)]
    out = _case(amd, "union3_1 (real data, N = 22)", lk, f, box, calls, [0, 1, 2])
    v0 = opt.best_fit(f, box, n_starts=32, seed=0, fixed={2: 0.0})
    out["chi2_map"], out["chi2_v0"] = best.chi2, v0.chi2
    out["sigma_v0"] = opt.sigma_from_delta_chi2(v0.chi2 - best.chi2, 1)
    lk.engine.close()
    return out


def desi(amd):
    g = np.load(os.path.join(ROOT, "tests", "golden", "bao_desi.npz"))
    box = np.asarray(g["bounds"], dtype=np.float64)
    lk = amd.likelihoods.DesiBao(g["bao_z"], g["bao_val"], g["bao_qty"], g["bao_inv_cov"], rd=float(g["rd"]), bounds=box)
    f, opt = lk.engine.torch_log_prob(amd.CF_OUT_LOGL), amd.optimize
    best = opt.best_fit(f, box, n_starts=32, seed=0)
    w0 = np.linspace(-0.99, -0.01, 64)
    calls = [("best_fit 32 starts", lambda: opt.best_fit(f, box, n_starts=32, seed=0), 32),
             ("profile of w0 64 x 16", lambda: opt.profile(f, box, 2, w0, n_starts=16, best=best), 1024),
             ("profile of (Om, w0) 32 x 32 x 4",
              lambda: opt.profile(f, box, (1, 2), (np.linspace(0.2, 0.45, 32), np.linspace(-0.99, -0.01, 32)), n_starts=4,
                                  best=best), 4096)]
    out = _case(amd, "bao/desi.py (real data, 13 BAO)", lk, f, box, calls, [0, 1, 2])
    out["chi2_map"] = best.chi2
    lk.engine.close()
    return out


def pantheon(amd, serial=True):
    syn = amd.synthetic.pantheon_like(n_sn=1701, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    box = amd.sn_pantheon.bounds
    f, opt = lk.engine.torch_log_prob(amd.CF_OUT_LOGP), amd.optimize
    best = opt.best_fit(f, box, n_starts=64, seed=0)
    calls = [("best_fit 64 starts", lambda: opt.best_fit(f, box, n_starts=64, seed=0), 64),
             ("profile of Om 64 x 16", lambda: opt.profile(f, box, 2, np.linspace(0.05, 0.65, 64), n_starts=16, best=best), 1024)]
    if not serial:
        for label, fn, _ in calls:
            fn()
        lk.engine.close()
        return {"case": "pantheon_like", "profiled_only": True}
    out = _case(amd, "pantheon_like (synthetic, N = 1701, log P with the H0 prior)", lk, f, box, calls, [0, 1, 2, 3])
    out["log_prob_max"] = best.log_prob
    lk.engine.close()
    return out


def share(path):
    """Device time of the cf_opt_* kernels against the likelihood kernels from a rocprofv3 kernel_stats.csv."""
    optk, other, rows = 0.0, 0.0, {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name, tot = r["Name"], float(r["TotalDurationNs"])
            rows[name[:90]] = {"calls": int(r["Calls"]), "total_ms": tot * 1e-6, "avg_us": float(r["AverageNs"]) * 1e-3}
            if any(k in name for k in OPT_KERNELS):
                optk += tot
            elif not any(t in name for t in ("at::", "void at", "rocprim", "hipcub", "elementwise", "sort", "index")):
                other += tot
    torch_ms = sum(v["total_ms"] for k, v in rows.items() if not any(t in k for t in OPT_KERNELS)) - other * 1e-6
    return {"opt_kernels_ms": optk * 1e-6, "likelihood_kernels_ms": other * 1e-6, "torch_kernels_ms": torch_ms,
            "opt_share": optk / (optk + other), "target": 0.10, "kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("union3", "desi", "pantheon"), default=None)
    ap.add_argument("--share", default=None, help="rocprofv3 kernel_stats.csv of a `--only pantheon` run to fold in")
    a = ap.parse_args()
    if a.share:
        out = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        out["kernel_share_pantheon"] = share(a.share)
    else:
        amd = importlib.import_module("cosmology-model-fit_amd")
        if amd.lib().cf_device_count() < 1:
            sys.exit("opt_probe needs an MI355X")
        if a.only == "pantheon" and a.out == "/dev/null":
            runs = [pantheon(amd, serial=False)]
        else:
            runs = [fn(amd) for key, fn in (("union3", union3), ("desi", desi), ("pantheon", pantheon)) if a.only in (None, key)]
        out = {"probe": "opt_probe", "device": torch.cuda.get_device_name(0), "runs": runs}
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
