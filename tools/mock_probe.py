#!/usr/bin/env python3
"""Cost of the mock-data likelihood next to the likelihood kernels of the same call, and of a whole Delta chi^2 calibration;
writes one JSON file.

Per 4096-row chunk (the library's own chunk) of the Pantheon+-shaped synthetic likelihood (1701 SNe by default), every row on a
mock of its own (4096 mocks: g is 4096 x 1701 doubles = 56 MB, read once), HIP events on torch's current stream around

* ``cf_resid_device`` asked for nothing but ``chi2_blocks``: the accessor path of the likelihood, the common part;
* ``cf_mock_eval_device`` with every row on the observed data (k = -1: the accessor path and the launch of mock_shift_kernel,
  no g traffic) and with distinct mocks: the difference is the pass over g (differences below the spread of the repetitions
  are not resolved and are reported as such);
* ``cf_eval_device``: the production path of the same rows, for scale.

Then ``MockSet.draw`` + ``MockSet.delta_chi2`` for MOCKS mocks, device-synchronised wall time: the velocity step of the
Pantheon+-shaped likelihood (v = 0 against free, 4 parameters) and of the Union3 likelihood of the golden fixture (22 bins).

    python tools/mock_probe.py --out profiles/r14_mock_probe.json
"""
import argparse
import ctypes as C
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
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": float(np.median(out)), "min": float(min(out)), "max": float(max(out))}


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def _calibration(amd, engine, theta_fid, fixed, n_mocks, n_starts):
    M = amd.mocks
    ms, t_draw = _wall(lambda: M.MockSet.draw(engine, theta_fid, n_mocks, seed=0))
    res, t_fit = _wall(lambda: ms.delta_chi2(fixed, n_starts=n_starts, seed=0))
    d = res["delta_chi2"]
    return {"n_mocks": n_mocks, "n_starts": n_starts, "draw_ms": t_draw, "delta_chi2_ms": t_fit, "likelihood_rows": res["n_like"],
            "rows_per_s": res["n_like"] / (t_fit * 1e-3), "n_below_minus_tol": res["n_below"], "median_delta_chi2": float(np.median(d)),
            "q95_delta_chi2": float(np.quantile(d, 0.95)), "wilks_q95_chi2_1": 3.841458820694124,
            "status_full": res["full"].status_counts, "status_nested": res["nested"].status_counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_mock_probe.json"))
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--mocks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n-starts", type=int, default=4)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("mock_probe needs an MI355X")
    L, lib, M, dev = amd._lib, amd.lib(), amd.mocks, torch.device("cuda:0")
    syn = amd.synthetic.pantheon_like(n_sn=a.n_sn, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], h0_prior=None)
    eng = lk.engine
    rng = np.random.default_rng(1)
    m = L.CF_MOCK_CHUNK
    theta = amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * rng.standard_normal((m, 4))
    x = torch.from_numpy(theta).to(dev)
    fid = np.array(amd.synthetic.THETA_TRUE, dtype=np.float64)
    fid[3] = 0.0
    ms = M.MockSet.draw(eng, fid, m, seed=0)
    distinct = torch.arange(m, dtype=torch.int32, device=dev)
    observed = torch.full((m,), -1, dtype=torch.int32, device=dev)
    out_t = torch.empty(m, dtype=torch.float64, device=dev)
    blocks = torch.empty((m, 10), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def mock_call(idx):
        L.check(lib.cf_mock_eval_device(eng._h, C.byref(ms._c), x.data_ptr(), m, idx.data_ptr(), L.CF_OUT_LOGL, out_t.data_ptr(), None,
                                        stream))

    per = {
        "accessor_path_only": _event_ms(lambda: L.check(lib.cf_resid_device(eng._h, x.data_ptr(), m, None, L.CF_RB_SN, None, 0, None,
                                                                            blocks.data_ptr(), None, stream)), a.reps),
        "mock_observed_rows": _event_ms(lambda: mock_call(observed), a.reps),
        "mock_distinct_mocks": _event_ms(lambda: mock_call(distinct), a.reps),
        "production_eval": _event_ms(lambda: eng.eval_device(x.data_ptr(), m, out_t.data_ptr(), L.CF_OUT_LOGL, stream), a.reps),
    }
    g_bytes = m * a.n_sn * 8
    med = {k: v["median"] for k, v in per.items()}
    spread = max(v["max"] - v["min"] for v in per.values())
    out = {"probe": "mock_probe", "n_sn": a.n_sn, "chunk_rows": m, "reps": a.reps, "info": eng.info()["gcn_arch"], "g_bytes": g_bytes,
           "per_chunk_ms": per, "largest_spread_ms": spread,
           # differences of medians; one that is below largest_spread_ms is not resolved by this probe.  The accessor-path call is
           # not a bare baseline: it carries resid_sample_kernel's block assembly and three memsets
           "mock_call_minus_accessor_call_ms": med["mock_distinct_mocks"] - med["accessor_path_only"],
           "g_pass_ms": med["mock_distinct_mocks"] - med["mock_observed_rows"],
           "mock_call_over_production_eval": med["mock_distinct_mocks"] / med["production_eval"]}
    del ms
    out["pantheon_velocity_step"] = _calibration(amd, eng, fid, {3: 0.0}, a.mocks, a.n_starts)
    eng.close()

    g = np.load(os.path.join(ROOT, "tests", "golden", "sn_union3_1.npz"))
    box = amd.likelihoods.SnUnion3.PRIOR_BOX
    u3 = amd.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    null = amd.optimize.best_fit(u3.engine.torch_log_prob(amd.CF_OUT_LOGL), box, n_starts=32, seed=0, fixed={2: 0.0})
    out["union3_velocity_step"] = _calibration(amd, u3.engine, null.x, {2: 0.0}, a.mocks, a.n_starts)
    u3.engine.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
