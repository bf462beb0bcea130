#!/usr/bin/env python3
"""Cost of the template scan (csrc/cosmofit_scan.hip) next to its measured neighbours; writes one JSON file.

Shape: the Pantheon+-shaped synthetic likelihood (sn/pantheon.py, 1701 SNe by default), one chunk of 4096 rows, K = 256, 4096
and 16384 candidates.  HIP events on torch's current stream; the shapes interleaved round by round on one device (ROUNDS rounds
after a warm-up of every shape), the median and the spread (min, max) of each reported:

* the three kernels on resident rows (``cf_scan_apply_device``) without the map (row outputs and column accumulators) and with it;
* ``torch.matmul`` + ``torch.max`` on the same rows and V (the map stored, the statistic and its maximum as tensor operations);
* ``prec_gemm_kernel`` (``cf_prec_apply_device``) on the same rows: the n x n product whose rate is the yardstick;
* ``cf_scan_eval_device`` (K = 4096) beside ``cf_marg_eval_device`` (the offset) and ``cf_eval_device`` on the same rows of theta;
* host time of ``scan.prepare`` and wall time of ``TemplateScan.null(10^5)`` at K = 4096.

    python tools/scan_probe.py --out profiles/r22_scan_probe.json
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
M_REF = -19.35


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_scan_probe.json"))
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--candidates", type=int, nargs="+", default=[256, 4096, 16384])
    ap.add_argument("--null-draws", type=int, default=100000)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("scan_probe needs an MI355X")
    L, N, SC, SP, Param, dev = amd._lib, amd.nuisance, amd.scan, amd.sn_pantheon, amd.Param, torch.device("cuda:0")
    n, m = a.n_sn, a.rows
    syn = amd.synthetic.pantheon_like(n_sn=n, seed=0)
    red = amd.LikelihoodEngine(ndim=3, z_max=float(syn["z_max"]), n_grid=SP.N_GRID,
                               params=dict(offset=Param(fixed=M_REF), H0=Param(0), Om=Param(1), v=Param(2)),
                               sn=dict(z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"], z_turn=SP.Z_TURN),
                               bounds=SP.bounds[1:], gauss=[(0,) + tuple(SP.H0_PRIOR[1:])])
    rng = np.random.default_rng(1)
    pitch = (n + 63) // 64 * 64
    rows = torch.zeros((m, pitch), dtype=torch.float64, device=dev)
    rows[:, :n] = torch.from_numpy(rng.standard_normal((m, n)) @ syn["chol"].T).to(dev)
    theta = torch.from_numpy(amd.synthetic.THETA_TRUE[1:] + np.array([1.0, 0.03, 0.3]) * rng.standard_normal((m, 3))).to(dev)
    prec = red.precision("sn")
    g = torch.empty((m, n), dtype=torch.float64, device=dev)

    fns, flops, scans = {"prec_gemm": lambda: prec.apply(rows, out=g)}, {"prec_gemm": 2.0 * m * n * n}, []
    for K in a.candidates:
        V = rng.standard_normal((n, K)) / np.sqrt(n)
        sc = SC.Scan(V, device=0)
        Vd = torch.from_numpy(V).to(dev)
        acc = torch.zeros(2 * K + 1, dtype=torch.float64, device=dev)
        scans.append(sc)

        def torch_path(Vd=Vd):
            Z = rows[:, :n] @ Vd
            return (Z * Z).max(dim=1)

        fns["scan_K%d" % K] = lambda sc=sc, acc=acc: sc.apply(rows, want=("best", "best_k", "s_best"), colacc=acc)
        fns["scan_rows_only_K%d" % K] = lambda sc=sc: sc.apply(rows, want=("best", "best_k", "s_best"))
        fns["scan_with_map_K%d" % K] = lambda sc=sc, acc=acc: sc.apply(rows, want=("best", "best_k", "s_best", "map"), colacc=acc)
        fns["torch_matmul_max_K%d" % K] = torch_path
        for name in ("scan", "scan_rows_only", "scan_with_map", "torch_matmul_max"):
            flops["%s_K%d" % (name, K)] = 2.0 * m * n * K
    kernels = _interleaved_ms(fns, a.rounds)
    tflops = {k: flops[k] / (v["median"] * 1e-3) / 1e12 for k, v in kernels.items()}
    ratios = {}
    for K in a.candidates:
        ratios["K%d" % K] = {
            "rate_over_prec_gemm_rate": tflops["scan_K%d" % K] / tflops["prec_gemm"],
            "scan_over_torch": _ratio(kernels, "scan_K%d" % K, "torch_matmul_max_K%d" % K),
            "scan_with_map_over_torch": _ratio(kernels, "scan_with_map_K%d" % K, "torch_matmul_max_K%d" % K),
            "with_map_over_without": _ratio(kernels, "scan_with_map_K%d" % K, "scan_K%d" % K)}

    # the entry points on rows of theta, K = 4096 (or the middle of the list), real candidates: every step over the offset
    K_eval = a.candidates[len(a.candidates) // 2]
    cand = rng.standard_normal((n, K_eval))
    t0 = time.perf_counter()
    prep = SC.prepare(syn["chol"], cand, base=np.ones(n))
    t_prepare = time.perf_counter() - t0
    ts = SC.TemplateScan(red, cand, base=np.ones(n))
    ln1 = N.LinearNuisance(red, N.Templates.offset(n), slots=("offset",))
    out_e = torch.empty(m, dtype=torch.float64, device=dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream

    def engine_eval():
        L.check(amd.lib().cf_eval_device(red._h, theta.data_ptr(), m, out_e.data_ptr(), L.CF_OUT_LOGP, stream()))

    evals = _interleaved_ms({
        "cf_eval_device": engine_eval,
        "cf_marg_eval_device_m1": lambda: ln1._device(theta, L.CF_OUT_LOGP),
        "cf_scan_eval_device": lambda: ts.torch_rows(theta),
    }, a.rounds)
    ts.null(4096, seed=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    null = ts.null(a.null_draws, seed=1)
    torch.cuda.synchronize()
    t_null = time.perf_counter() - t0

    out = {"probe": "scan_probe", "n_sn": n, "rows": m, "rounds": a.rounds, "info": red.info()["gcn_arch"],
           "candidates": a.candidates, "tile": L.CF_SCAN_TILE, "kernels_ms": kernels, "kernels_tflops": tflops, "ratios": ratios,
           "K_eval": K_eval, "evals_ms": evals,
           "eval_ratios": {"scan_eval_over_cf_eval_device": _ratio(evals, "cf_scan_eval_device", "cf_eval_device"),
                           "scan_eval_over_marg_eval": _ratio(evals, "cf_scan_eval_device", "cf_marg_eval_device_m1")},
           "prepare_s": t_prepare, "probe_rel": prep["probe_rel"], "null_draws": a.null_draws, "null_s": t_null,
           "null_best_median": float(null.median().item())}
    for o in scans + [ts, ln1, red]:
        o.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
