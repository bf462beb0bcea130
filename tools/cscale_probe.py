#!/usr/bin/env python3
"""Cost of the scaled covariance C(s) = C0 + s C1 on the device next to its measured neighbours; writes one JSON file.

Shape: the Pantheon+-shaped synthetic likelihood (sn/pantheon.py, 1701 SNe by default), C1 = the 0/1 diagonal of z <= 0.2 (the
extra scatter of the low-z sample), one chunk of 4096 rows.  HIP events on torch's current stream; A and B interleaved round by
round on one device (ROUNDS rounds after a warm-up of every shape), the median and the spread (min, max) of each reported:

* the fused product + row kernel (``cf_cscale_apply_device`` with quad and logdet, y never stored) against
  ``cf_prec_apply_device`` on the same rows: the same flop count, but the latter writes its [4096, n] result;
* the same with y stored, and with 16 amplitudes per row;
* the row kernel alone, as the difference to a call that asks for y only (the product without a partial or a row kernel) --
  an estimate, named as such;
* ``cf_cscale_eval_device`` (one amplitude, and 16) against ``cf_eval_device`` on the same rows of theta;
* host time of ``covscale.decompose`` and of ``cf_cscale_create``.

    python tools/cscale_probe.py --out profiles/r20_cscale_probe.json
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


def _interleaved_ms(fns: dict, rounds: int) -> dict:
    """Every function once per round, in turn, each between its own pair of events; per function median / min / max."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}


def _ratio(t, a, b):
    """median(a) / median(b) and the range the spreads of both allow."""
    return {"median": t[a]["median"] / t[b]["median"], "lowest": t[a]["min"] / t[b]["max"], "highest": t[a]["max"] / t[b]["min"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_cscale_probe.json"))
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("cscale_probe needs an MI355X")
    L, V, dev = amd._lib, amd.covscale, torch.device("cuda:0")
    n, m = a.n_sn, a.rows
    syn = amd.synthetic.pantheon_like(n_sn=n, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    eng = lk.engine
    c1 = (syn["z_cmb"] <= 0.2).astype(np.float64)
    t0 = time.perf_counter()
    T, lam, info = V.decompose(syn["chol"], c1)
    t_decompose = time.perf_counter() - t0
    t0 = time.perf_counter()
    dec = V.Decomposition(T, lam, device=0)
    t_create = time.perf_counter() - t0
    sc = V.ScaledCovariance(eng, c1, (0.0, 0.09), power=2)
    prec = eng.precision("sn")

    rng = np.random.default_rng(1)
    pitch = (n + 63) // 64 * 64
    rows = torch.zeros((m, pitch), dtype=torch.float64, device=dev)
    rows[:, :n] = torch.from_numpy(rng.standard_normal((m, n)) @ syn["chol"].T).to(dev)
    g = torch.empty((m, n), dtype=torch.float64, device=dev)
    s1 = torch.from_numpy(rng.uniform(0.0, 0.04, (m, 1))).to(dev)
    s16 = torch.from_numpy(rng.uniform(0.0, 0.04, (m, 16))).to(dev)
    theta = torch.from_numpy(amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * rng.standard_normal((m, 4))).to(dev)
    out_e = torch.empty(m, dtype=torch.float64, device=dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream

    def engine_eval():
        L.check(amd.lib().cf_eval_device(eng._h, theta.data_ptr(), m, out_e.data_ptr(), L.CF_OUT_LOGP, stream()))

    kernels = _interleaved_ms({
        "cf_prec_apply_device": lambda: prec.apply(rows, out=g),
        "cscale_apply_1": lambda: dec.apply(rows, s1),
        "cscale_apply_1_with_y": lambda: dec.apply(rows, s1, want_y=True),
        "cscale_apply_16": lambda: dec.apply(rows, s16),
        "cscale_product_y_only": lambda: dec.apply(rows, s1, want_y=True, want=()),
    }, a.rounds)
    evals = _interleaved_ms({
        "cf_eval_device": engine_eval,
        "cf_cscale_eval_device_1": lambda: sc._device(theta, s1, L.CF_OUT_LOGP),
        "cf_cscale_eval_device_16": lambda: sc._device(theta, s16, L.CF_OUT_LOGP),
    }, a.rounds)

    flops = 2.0 * m * n * n
    out = {"probe": "cscale_probe", "n_sn": n, "rows": m, "rounds": a.rounds, "info": eng.info()["gcn_arch"],
           "c1": "diag(z <= 0.2)", "n_nonzero_eigenvalues": int(np.count_nonzero(lam)), "s_min": info["s_min"],
           "probe_rel": info["probe_rel"], "decompose_s": t_decompose, "cf_cscale_create_s": t_create,
           "kernels_ms": kernels, "evals_ms": evals,
           "ratios": {
               "fused_product_and_row_over_prec_apply": _ratio(kernels, "cscale_apply_1", "cf_prec_apply_device"),
               "with_y_over_prec_apply": _ratio(kernels, "cscale_apply_1_with_y", "cf_prec_apply_device"),
               "sixteen_amplitudes_over_one": _ratio(kernels, "cscale_apply_16", "cscale_apply_1"),
               "cscale_eval_1_over_cf_eval_device": _ratio(evals, "cf_cscale_eval_device_1", "cf_eval_device"),
               "cscale_eval_16_over_cf_eval_device": _ratio(evals, "cf_cscale_eval_device_16", "cf_eval_device"),
           },
           "row_kernel_and_partials_ms_estimate": kernels["cscale_apply_1_with_y"]["median"] - kernels["cscale_product_y_only"]["median"],
           "fused_product_tflops": flops / (kernels["cscale_apply_1"]["median"] * 1e-3) / 1e12,
           "prec_gemm_tflops": flops / (kernels["cf_prec_apply_device"]["median"] * 1e-3) / 1e12,
           "partial_bytes_one_amplitude": int(m * ((n + 31) // 32) * 8), "y_bytes_not_written": int(m * n * 8)}
    sc.close()
    dec.close()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
