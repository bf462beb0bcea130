#!/usr/bin/env python3
"""Time of the all-pairs kernel density sum (cf_kde_sum_device, csrc/cosmofit_kde.hip) at the sizes a tension estimate uses,
beside scipy.stats.gaussian_kde on a host copy; writes one JSON file.

* n = m = 2^17 with exact leave-one-out (self_offset = 0), d = 1, 2, 4, 6: the densities at the samples.  HIP events on torch's
  current stream around the call, after one warm-up call, REPS repetitions; pairs per second = n m / median.
* m = 1 at n = 2^20 with the squared sum: the density at zero shift (every slice a workgroup of its own).
* scipy.stats.gaussian_kde(samples.T)(samples.T), host wall clock, d = 2, at n = 16384 and, if four times that time stays under
  a minute, at n = 32768.  Its time at n = 2^17 is an EXTRAPOLATION by (2^17 / n)^2 from the largest n timed and is labelled so.

    python tools/tension_probe.py --out profiles/r15_tension_probe.json
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
sys.path[:0] = [ROOT]


def _event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": float(np.median(out)), "min": float(min(out)), "max": float(max(out)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_tension_probe.json"))
    ap.add_argument("--log2-n", type=int, default=17)
    ap.add_argument("--log2-n-zero", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-n", type=int, default=16384)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("tension_probe needs an MI355X")
    L, lib, dev = amd._lib, amd.lib(), torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(0)
    out = {"probe": "tension_probe", "device": torch.cuda.get_device_name(0), "tile": L.CF_KDE_TILE, "slice": L.CF_KDE_SLICE,
           "all_pairs": [], "zero_shift": []}

    n = 1 << a.log2_n
    for d in (1, 2, 4, 6):
        y = torch.from_numpy(rng.standard_normal((n, d))).to(dev)
        res = torch.empty(n, dtype=torch.float64, device=dev)
        t = _event_ms(lambda: L.check(lib.cf_kde_sum_device(y.data_ptr(), None, n, d, y.data_ptr(), n, 0, res.data_ptr(), None, stream)),
                      a.reps)
        out["all_pairs"].append({"n": n, "m": n, "ndim": d, "self_offset": 0, "ms": t, "pairs_per_s": n * n / (t["median"] * 1e-3),
                                 "checksum": float(res.sum())})
    nz = 1 << a.log2_n_zero
    for d in (1, 2, 4, 6):
        y = torch.from_numpy(rng.standard_normal((nz, d))).to(dev)
        w = torch.from_numpy(rng.uniform(0.1, 1.0, nz)).to(dev)
        q = torch.zeros((1, d), dtype=torch.float64, device=dev)
        res, sq = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
        t = _event_ms(lambda: L.check(lib.cf_kde_sum_device(y.data_ptr(), w.data_ptr(), nz, d, q.data_ptr(), 1, -1, res.data_ptr(),
                                                            sq.data_ptr(), stream)), 4 * a.reps)
        out["zero_shift"].append({"n": nz, "m": 1, "ndim": d, "weighted": True, "with_sq": True, "ms": t,
                                  "pairs_per_s": nz / (t["median"] * 1e-3)})

    # the whole estimator through the Python layer, once warm: what a user waits for
    x = torch.from_numpy(rng.standard_normal((n, 2)) + np.array([1.0, 0.5])).to(dev)
    amd.tension.kde_shift(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = amd.tension.kde_shift(x)
    torch.cuda.synchronize()
    out["kde_shift_wall_ms"] = {"n": n, "ndim": 2, "ms": (time.perf_counter() - t0) * 1e3, "p_exceed": r.p_exceed}

    from scipy import stats

    host = []
    ns, d = a.scipy_n, 2
    while True:
        xs = rng.standard_normal((ns, d))
        t0 = time.perf_counter()
        stats.gaussian_kde(xs.T)(xs.T)
        sec = time.perf_counter() - t0
        host.append({"n": ns, "m": ns, "ndim": d, "seconds": sec, "pairs_per_s": ns * ns / sec})
        if 4.0 * sec >= 60.0 or ns >= n:
            break
        ns *= 2
    last = host[-1]
    out["scipy_host"] = host
    out["scipy_host_extrapolated"] = {"n": n, "ndim": d, "seconds": last["seconds"] * (n / last["n"]) ** 2,
                                      "note": f"EXTRAPOLATED by (n / {last['n']})^2 from the largest n timed; not measured"}
    dev2 = next(e for e in out["all_pairs"] if e["ndim"] == d)
    out["speedup_over_scipy_at_equal_pairs_d2"] = dev2["pairs_per_s"] / last["pairs_per_s"]

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
