#!/usr/bin/env python3
"""Cost of the corner-plot marginals on the device against their numpy restatement on a host copy; writes one JSON file.

* ``marginals.histograms`` and ``marginals.corner_data`` (the reference's corner_plot.py arguments: 100 bins, range 0.9999,
  sigma 2) on a [2500 x 4096, 4] and a [2500 x 4096, 6] unweighted chain and on a 2 x 10^5-row weighted posterior of 6
  columns: device-synchronised wall time, median of REPS calls after one warm-up call;
* the same numbers by numpy on a host copy (tests/marginals_reference.py: np.percentile or the weighted quantile for the
  ranges, np.histogram per column, np.histogram2d per pair), the device-to-host copy included and also given alone, once;
* that both give the same counts (unweighted) at these sizes.

The kernels' own times come from a profiler run of their own, whose stats CSV ``--share`` folds into the same file:

    python tools/marginals_probe.py --out profiles/r09_marginals_probe.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/marginals_probe.py --kernels-only
    python tools/marginals_probe.py --out profiles/r09_marginals_probe.json --share DIR/.../*_kernel_stats.csv

(with ``--only chain6`` on both of the last two commands the table is that shape's alone).
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = (("chain4", 2500 * 4096, 4, False), ("chain6", 2500 * 4096, 6, False), ("posterior6_weighted", 200_000, 6, True))
KERNELS = ("marg_bin_kernel", "marg_hist1_kernel", "marg_hist2_kernel")


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _sample(n, k, weighted, dev):
    """A correlated Gaussian with the offsets of a cosmological chain, made on the device from a seed."""
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + k)
    a = torch.randn((k, k), generator=g, device=dev, dtype=torch.float64)
    chol = torch.linalg.cholesky(a @ a.T + 0.5 * torch.eye(k, device=dev, dtype=torch.float64))
    scale = torch.tensor([0.02, 0.1, 1.5, 0.01, 0.3, 0.05][:k], device=dev, dtype=torch.float64)
    mean = torch.tensor([0.3, -19.3, 70.0, 0.02, -1.0, 0.7][:k], device=dev, dtype=torch.float64)
    x = mean + (torch.randn((n, k), generator=g, device=dev, dtype=torch.float64) @ chol.T) * scale
    w = torch.exp(1.5 * torch.randn(n, generator=g, device=dev, dtype=torch.float64)) if weighted else None
    return x.contiguous(), w


def _numpy_restatement(x, w, bins, r):
    """What a script does today after copying the chain to the host: ranges, 1-D and 2-D histograms by numpy."""
    import marginals_reference as mr

    t0 = time.perf_counter()
    xh = x.cpu().numpy()
    wh = None if w is None else w.cpu().numpy()
    t_copy = time.perf_counter() - t0
    k = xh.shape[1]
    lo_hi = mr.fraction_ranges(xh, r, wh)
    h1 = [np.histogram(xh[:, c], bins=bins, range=tuple(lo_hi[c]), weights=wh)[0] for c in range(k)]
    h2 = [np.histogram2d(xh[:, a], xh[:, b], bins=bins, range=[tuple(lo_hi[a]), tuple(lo_hi[b])], weights=wh)[0]
          for a in range(k) for b in range(a)]
    return time.perf_counter() - t0, t_copy, np.stack(h1), np.stack(h2)


def share(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            if any(k in r["Name"] for k in KERNELS):
                rows[r["Name"][:100]] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) * 1e-6,
                                         "avg_ms": float(r["AverageNs"]) * 1e-6, "min_ms": float(r["MinNs"]) * 1e-6,
                                         "max_ms": float(r["MaxNs"]) * 1e-6}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_marginals_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--kernels-only", action="store_true", help="three histograms() calls per shape and nothing else (for the profiler)")
    ap.add_argument("--only", default=None, help="one of " + ", ".join(s[0] for s in SHAPES))
    ap.add_argument("--share", default=None, help="rocprofv3 kernel_stats.csv of a --kernels-only run to fold into --out")
    a = ap.parse_args()
    if a.share:
        out = json.load(open(a.out)) if os.path.exists(a.out) else {"probe": "marginals_probe"}
        out.setdefault("kernel_trace", {"how": "rocprofv3 --kernel-trace --stats over a --kernels-only run (3 histograms() calls "
                                               "of the named shape, or of all three under 'all')"})
        out["kernel_trace"][a.only or "all"] = share(a.share)
        json.dump(out, open(a.out, "w"), indent=1)
        return

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("marginals_probe needs an MI355X")
    M, dev = amd.marginals, torch.device("cuda:0")
    bins, r = 100, 0.9999
    out = {"probe": "marginals_probe", "bins": bins, "range": r, "reps": a.reps, "shapes": {}}
    for name, n, k, weighted in SHAPES:
        if a.only and name != a.only:
            continue
        x, w = _sample(n, k, weighted, dev)
        if a.kernels_only:
            for _ in range(3):
                M.histograms(x, bins=bins, range=r, weights=w)
            torch.cuda.synchronize()
            continue
        lo_hi = [tuple(v) for v in M.histograms(x, bins=bins, range=r, weights=w)[0][:, [0, -1]]]  # warm-up; the ranges
        M.corner_data(x, bins=bins, range=r, weights=w)
        res = {"rows": n, "columns": k, "weighted": weighted, "pairs": k * (k - 1) // 2}
        for label, fn in (("histograms_given_ranges_ms", lambda: M.histograms(x, bins=bins, range=lo_hi, weights=w)),
                          ("histograms_ms", lambda: M.histograms(x, bins=bins, range=r, weights=w)),
                          ("corner_data_ms", lambda: M.corner_data(x, bins=bins, range=r, weights=w))):
            ts = [_timed(fn)[0] * 1e3 for _ in range(a.reps)]
            res[label] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
        if not a.skip_numpy:
            t_all, t_copy, h1, h2 = _numpy_restatement(x, w, bins, r)
            res["numpy_on_host_copy_s"], res["device_to_host_copy_s"] = t_all, t_copy
            _, g1, g2, _ = M.histograms(x, bins=bins, range=r, weights=w)
            g1, g2 = g1.cpu().numpy(), g2.cpu().numpy()
            if weighted:
                res["max_abs_diff_to_numpy_over_largest_bin"] = float(max(np.abs(g1 - h1).max(), np.abs(g2 - h2).max()) / h1.max())
            else:
                res["counts_equal_numpy"] = bool(np.array_equal(g1, h1) and np.array_equal(g2, h2))
            res["numpy_over_device_histograms"] = t_all / (res["histograms_ms"]["median"] * 1e-3)
        out["shapes"][name] = res
        del x, w
        torch.cuda.empty_cache()
    if a.kernels_only:
        return
    if os.path.exists(a.out):  # keep a kernel trace folded in earlier
        old = json.load(open(a.out))
        if "kernel_trace" in old:
            out["kernel_trace"] = old["kernel_trace"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
