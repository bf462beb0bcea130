#!/usr/bin/env python3
"""Cost of the leave-group-out pass on the device next to the GEMM that forms g and next to the tensor restatement of the
importance summary; writes one JSON file.

Shape: the Pantheon+-shaped synthetic likelihood (sn/pantheon.py, 1701 SNe by default).  HIP events on torch's current stream,
median of REPS after a warm-up:

* per 4096-row chunk, for a partition into 10 redshift bins of equal count and into 17 label groups of unequal size:
  ``cf_group_quad_device`` (``group_quad_kernel``) beside ``cf_prec_apply_device`` (``prec_gemm_kernel``) on the same chunk;
* ``cf_reweight_device`` at S = 2^18, G = 32, ncol = 6 beside the torch restatement (``logsumexp`` and weighted moments) on
  the same tensors;
* device-synchronised wall time of ``leaveout.leave_group_out`` on ROWS rows, and the host time of ``cf_group_create``.

By flop count a partition into G equal groups costs n^2 / (2 G) multiply-adds per row against n^2 for the GEMM, and the
summary should be bound by the bandwidth of lw and x.  The probe records the outcome whatever it is.

    python tools/leaveout_probe.py --out profiles/r18_leaveout_probe.json
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


def _torch_summary(lw, x, pivot):
    """The tensor restatement of the record: logsumexp and weighted first and second moments about the pivot."""
    lse = torch.logsumexp(lw, dim=0)
    w = torch.exp(lw - lw.max(dim=0).values[None, :])
    d = x - pivot[None, :]
    m1 = w.T @ d
    m2 = torch.einsum("sg,si,sj->gij", w, d, d)
    return lse, w.sum(dim=0), (w * w).sum(dim=0), m1, m2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_leaveout_probe.json"))
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("leaveout_probe needs an MI355X")
    L, LO, dev = amd._lib, amd.leaveout, torch.device("cuda:0")
    syn = amd.synthetic.pantheon_like(n_sn=a.n_sn, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    eng, n = lk.engine, a.n_sn
    prec = eng.precision("sn")
    rng = np.random.default_rng(1)
    theta = amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * rng.standard_normal((a.rows, 4))
    x = torch.from_numpy(theta).to(dev)
    m = min(a.rows, L.CF_INFL_CHUNK)
    pitch = (n + 63) // 64 * 64
    rows = torch.zeros((m, pitch), dtype=torch.float64, device=dev)
    rows[:, :n] = torch.from_numpy(rng.standard_normal((m, n)) @ syn["chol"].T).to(dev)
    g = torch.empty((m, n), dtype=torch.float64, device=dev)

    out = {"probe": "leaveout_probe", "n_sn": n, "rows": a.rows, "chunk_rows": m, "reps": a.reps, "info": eng.info()["gcn_arch"]}
    gemm = _event_ms(lambda: prec.apply(rows, out=g), a.reps)
    out["prec_gemm_kernel_ms"] = gemm
    order = np.argsort(syn["z_cmb"], kind="stable")
    bins = [np.sort(c).astype(np.int32) for c in np.array_split(order, 10)]
    cuts = np.sort(rng.choice(np.arange(1, n), size=16, replace=False))
    labels = np.searchsorted(cuts, rng.permutation(n), side="right")
    surveys = LO.groups_from_labels(labels)[0]
    parts = {}
    for name, groups in (("redshift_bins_10", bins), ("label_groups_17", surveys)):
        t0 = time.perf_counter()
        G = LO.Groups(eng, groups, "sn")
        t_create = time.perf_counter() - t0
        q = torch.empty((m, G.n_groups), dtype=torch.float64, device=dev)
        ms = _event_ms(lambda: G.quad(g, out=q), a.reps)
        sizes = np.diff(G.offsets)
        madds = float((sizes.astype(np.float64)**2).sum() / 2.0)
        parts[name] = {"n_groups": int(G.n_groups), "sizes": sizes.tolist(), "group_create_s": t_create, "group_quad_kernel_ms": ms,
                       "over_prec_gemm_kernel": ms["median"] / gemm["median"], "flop_ratio_expected": madds / float(n * n),
                       "group_quad_tflops": 2.0 * m * madds / (ms["median"] * 1e-3) / 1e12}
        if name == "redshift_bins_10":
            out["leave_group_out_ms"] = _wall_ms(lambda: LO.leave_group_out(eng, x, G, "sn"), max(2, a.reps // 2))
            out["leave_group_out_rows_per_s"] = a.rows / (out["leave_group_out_ms"]["median"] * 1e-3)
        G.close()
    out["partitions"] = parts
    out["gemm_tflops"] = 2.0 * m * n * n / (gemm["median"] * 1e-3) / 1e12

    S, Gc, ncol = 1 << 18, 32, 6
    lw = torch.from_numpy(-700.0 + 2.0 * rng.standard_normal((S, Gc))).to(dev)
    xs = torch.from_numpy(rng.standard_normal((S, ncol))).to(dev)
    pivot = xs.mean(dim=0)
    pv = pivot.cpu().numpy()
    rw = {"S": S, "G": Gc, "ncol": ncol,
          "cf_reweight_device_ms": _event_ms(lambda: LO.reweight_record(lw, xs, None, pv), a.reps),
          "torch_restatement_ms": _event_ms(lambda: _torch_summary(lw, xs, pivot), a.reps)}
    rw["over_torch_restatement"] = rw["cf_reweight_device_ms"]["median"] / rw["torch_restatement_ms"]["median"]
    rw["input_bytes"] = int((lw.numel() + xs.numel()) * 8)
    rw["input_gb_per_s"] = rw["input_bytes"] / (rw["cf_reweight_device_ms"]["median"] * 1e-3) / 1e9
    rec = LO.reweight_record(lw, xs, None, pv).cpu().numpy()
    ref = _torch_summary(lw, xs, pivot)
    rw["max_rel_diff_sum_w_to_torch"] = float(np.max(np.abs(rec[:, 1] / ref[1].cpu().numpy() - 1)))
    out["reweight"] = rw
    lk.engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
