#!/usr/bin/env python3
"""Cost of the attribution on the device next to the likelihood evaluation of the same rows and next to ``torch.matmul``; writes
one JSON file.

Shape: the Pantheon+-shaped synthetic likelihood (sn/pantheon.py, 1701 SNe by default).  Per 4096-row chunk (the library's own
chunk), HIP events on torch's current stream around

* ``cf_prec_apply_device`` on 4096 residual rows at the pitch the engine keeps them (``prec_gemm_kernel`` alone);
* ``torch.matmul`` of the same rows and the same K on the same device (rocBLAS: no promise about a row's bits);
* ``cf_eval_device`` of the same chunk of theta (the likelihood's own kernels);
* ``cf_infl_device`` asked for the per-sample table alone, and with both accumulators.

Device-synchronised wall time of ``influence.report`` on ROWS rows (median of REPS after a warm-up), and the host time of
``cf_prec_create`` for this n and for n = 1590.  The probe records the outcome whatever it is.

    python tools/infl_probe.py --out profiles/r16_infl_probe.json
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
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": float(np.median(out)), "min": float(min(out)), "max": float(max(out))}


def _wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median": float(np.median(out)), "min": float(min(out)), "max": float(max(out))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_infl_probe.json"))
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("infl_probe needs an MI355X")
    L, infl, dev = amd._lib, amd.influence, torch.device("cuda:0")
    syn = amd.synthetic.pantheon_like(n_sn=a.n_sn, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    eng = lk.engine
    t0 = time.perf_counter()
    prec = eng.precision("sn")
    t_create = time.perf_counter() - t0
    rng = np.random.default_rng(1)
    theta = amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * rng.standard_normal((a.rows, 4))
    x = torch.from_numpy(theta).to(dev)
    m, n = min(a.rows, L.CF_INFL_CHUNK), a.n_sn
    xc = x[:m].contiguous()
    pitch = (n + 63) // 64 * 64
    rows = torch.zeros((m, pitch), dtype=torch.float64, device=dev)
    rows[:, :n] = torch.from_numpy(rng.standard_normal((m, n)) @ syn["chol"].T).to(dev)
    g = torch.empty((m, n), dtype=torch.float64, device=dev)
    K = torch.from_numpy(np.linalg.inv(syn["cov"])).to(dev)  # numpy's inverse: timing and a sanity difference only
    compact = rows[:, :n].contiguous()
    logp = torch.empty(m, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    out = {"probe": "infl_probe", "n_sn": n, "rows": a.rows, "chunk_rows": m, "reps": a.reps, "info": eng.info()["gcn_arch"],
           "prec_create_s": {"n": n, "s": t_create}}
    per = {
        "prec_gemm_kernel": _event_ms(lambda: prec.apply(rows, out=g), a.reps),
        "torch_matmul": _event_ms(lambda: torch.matmul(compact, K, out=g), a.reps),
        "cf_eval_device": _event_ms(lambda: eng.eval_device(xc.data_ptr(), m, logp.data_ptr(), L.CF_OUT_LOGP, stream), a.reps),
        "cf_infl_device_sample": _event_ms(lambda: infl.rows(eng, xc, want=()), a.reps),
    }
    acc = infl.Accumulator(eng, "sn", (2.0, 3.0), device=dev)
    per["cf_infl_device_sample_and_accumulators"] = _event_ms(lambda: acc.update(xc, want_sample=True), a.reps)
    out["per_chunk_ms"] = per
    gemm = per["prec_gemm_kernel"]["median"]
    out["gemm_tflops"] = 2.0 * m * n * n / (gemm * 1e-3) / 1e12
    out["gemm_over_torch_matmul"] = gemm / per["torch_matmul"]["median"]
    out["gemm_over_cf_eval_device"] = gemm / per["cf_eval_device"]["median"]
    got, ref = prec.apply(rows), torch.matmul(compact, K)
    out["max_abs_diff_to_torch_matmul_over_max_abs"] = float((got - ref).abs().max() / ref.abs().max())
    out["whole_chain_report_ms"] = _wall_ms(lambda: infl.report(eng, x, thresholds=(2.0, 3.0)), max(2, a.reps // 2))
    out["rows_per_s"] = a.rows / (out["whole_chain_report_ms"]["median"] * 1e-3)
    lk.engine.close()
    if n != 1590:
        syn = amd.synthetic.pantheon_like(n_sn=1590, seed=0)
        t0 = time.perf_counter()
        p = infl.Precision(syn["chol"], device=0)
        out["prec_create_1590_s"] = time.perf_counter() - t0
        p.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
