#!/usr/bin/env python3
"""Cost of the fit report on the device next to the likelihood kernels of the same call, and next to numpy on a host copy of
``engine.parts``; writes one JSON file.

Shape: the Pantheon+-shaped synthetic likelihood (sn/pantheon.py, 1701 SNe by default) and a chain of ROWS rows drawn around the
truth.  Per 4096-row chunk (the library's own chunk), HIP events on torch's current stream around

* ``cf_resid_device`` asked for nothing but ``chi2_blocks`` (the accessor path of the likelihood and the 80 bytes per row of the
  block assembly): the cost of the likelihood kernels of the call;
* the same call with the per-sample statistics (kernel A), with the per-datum accumulators (kernel B), and with both:
  the differences are the two kernels' shares.

Device-synchronised wall time of the whole chain through ``fit_report.report`` (median of REPS after a warm-up), and the host
route a script would take: ``engine.parts`` on chunks of the same rows (the S x N doubles of ``delta`` and ``mu_corr`` cross to
the host), then numpy / ``scipy.stats`` on them, on the first NUMPY_ROWS rows, scaled to the chain and marked ``extrapolated``.

    python tools/resid_probe.py --out profiles/r13_resid_probe.json
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

NUMPY_ROWS = 4096


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_resid_probe.json"))
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-numpy", action="store_true")
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("resid_probe needs an MI355X")
    import ctypes as C

    L, lib, F, dev = amd._lib, amd.lib(), amd.fit_report, torch.device("cuda:0")
    syn = amd.synthetic.pantheon_like(n_sn=a.n_sn, seed=0)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    eng = lk.engine
    rng = np.random.default_rng(1)
    theta = amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * rng.standard_normal((a.rows, 4))
    x = torch.from_numpy(theta).to(dev)
    chunk = L.CF_RESID_CHUNK
    xc = x[:chunk].contiguous()
    m = xc.shape[0]
    sample = torch.empty((m, L.CF_RS_NCOL), dtype=torch.float64, device=dev)
    blocks = torch.empty((m, 10), dtype=torch.float64, device=dev)
    thr = np.array([2.0, 3.0])
    acc = F.Accumulator(eng, "sn", thr, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(want_a, want_b):
        L.check(lib.cf_resid_device(eng._h, xc.data_ptr(), m, None, L.CF_RB_SN, thr.ctypes.data_as(C.c_void_p), 2,
                                    sample.data_ptr() if want_a else None, blocks.data_ptr(), C.byref(acc.c) if want_b else None,
                                    stream))

    out = {"probe": "resid_probe", "n_sn": a.n_sn, "rows": a.rows, "chunk_rows": m, "reps": a.reps, "info": eng.info()["gcn_arch"]}
    per = {name: _event_ms(lambda wa=wa, wb=wb: call(wa, wb), a.reps)
           for name, wa, wb in (("likelihood_only", False, False), ("with_A", True, False), ("with_B", False, True),
                                ("with_A_and_B", True, True))}
    base = per["likelihood_only"]["median"]
    out["per_chunk_ms"] = per
    out["kernel_A_ms"] = per["with_A"]["median"] - base
    out["kernel_B_ms"] = per["with_B"]["median"] - base
    out["share_of_likelihood"] = {"A": out["kernel_A_ms"] / base, "B": out["kernel_B_ms"] / base}
    out["kernel_A_GB_per_s"] = 2 * m * a.n_sn * 2 * 8 / max(out["kernel_A_ms"], 1e-6) / 1e6  # delta and mu_corr, read twice
    out["whole_chain_report_ms"] = _wall_ms(lambda: F.report(eng, x, thresholds=(2.0, 3.0)), max(2, a.reps // 2))
    out["rows_per_s"] = a.rows / (out["whole_chain_report_ms"]["median"] * 1e-3)

    if not a.skip_numpy:
        import scipy.stats as stats

        nrows = min(a.rows, NUMPY_ROWS)
        t0 = time.perf_counter()
        p = eng.parts(theta[:nrows])
        t_parts = time.perf_counter() - t0
        t0 = time.perf_counter()
        r, y = p["delta"], syn["obs"][None, :] - p["mu_corr"]
        ss_res, ss_tot = np.sum(r**2, axis=1), np.sum((y - y.mean(axis=1, keepdims=True)) ** 2, axis=1)
        host = np.stack([r.mean(axis=1), r.std(axis=1), ss_res, np.sqrt(np.mean(r**2, axis=1)), ss_tot, 1 - ss_res / ss_tot,
                         stats.skew(r, axis=1), stats.kurtosis(r, axis=1)], axis=1)
        mean_i, std_i = r.mean(axis=0), r.std(axis=0)
        t_numpy = time.perf_counter() - t0
        got = F.sample_stats(eng, x[:nrows].contiguous())[0].cpu().numpy()[:, :8]
        d = F.datum_stats(eng, x[:nrows].contiguous())
        out["host_route"] = {"rows": nrows, "parts_s": t_parts, "numpy_s": t_numpy,
                             "extrapolated_to_all_rows_s": (t_parts + t_numpy) * a.rows / nrows,
                             "bytes_to_host_per_row": 3 * a.n_sn * 8,
                             "max_abs_diff_of_the_statistics": float(np.max(np.abs(got - host))),
                             "max_abs_diff_of_datum_mean_std": float(max(np.max(np.abs(d["mean"] - mean_i)),
                                                                         np.max(np.abs(d["std"] - std_i))))}
    lk.engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
