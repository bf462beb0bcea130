#!/usr/bin/env python3
"""Cost of the quintessence reconstruction (csrc/cosmofit_field.hip) at the reference's sizes; writes one JSON file.

For [10^5, 3] and [10^6, 3] thawing samples at field.py's sizes -- 5000 nodes, every row's own 2000 field values and 1000 times:

* the time of ``cf_field_device`` by device events: REPS windows after a warm-up of the same shape, outputs ``V_phi`` and
  ``a_t`` and the scalars (what ``bands`` asks for), written in row chunks so that the output buffers stay at 2 x 64 MB;
* node evaluations per second (rows x 5000 / kernel time) and, from the operation count of the node loop (2 sqrt, 2 reciprocals
  and ~25 multiply-adds per node), the rate of those FP64 operations -- to be held against the FP64 vector rate of the device;
* the time of the table alone (no queries: scalars only), which separates the node loop and the sums from the look-ups;
* the float64 numpy restatement of field.py on a host copy (tests/field_reference.py's arithmetic in float64, scipy-free), timed
  on 200 rows and extrapolated linearly, with the device-to-host copy of the samples timed alone.

No speed bar is set: there is no earlier implementation to compare with.  The file is the record.

    python tools/field_probe.py --out profiles/r12_field_probe.json
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N_A, N_PHI, N_T, CHUNK = 5000, 2000, 1000, 4096
OPS_PER_NODE = {"sqrt": 2, "reciprocal": 2, "mul_add": 25}


def host_row(H0, Om, w0, a):
    """field.py in float64 numpy for one row (1 + w formed directly): the arrays behind V(phi), a(t) and the scalars."""
    a3 = a**3
    D = (1 + w0) * a3 + 1 - w0
    opw, rho = 2 * (1 + w0) * a3 / D, 4 / D**2
    Or = 4.1835e-05 / (H0 / 100) ** 2
    E = np.sqrt(Om / a3 + Or / (a3 * a) + (1 - Om - Or) * rho)
    da = np.diff(a)

    def cum(y):
        out = np.zeros_like(y)
        out[1:] = np.cumsum(da * (y[1:] + y[:-1]) / 2)
        return out

    phi = cum(np.sqrt(opw * rho) / (a * H0 * E))
    t = cum(1 / (a * E)) * 9.77813 / (H0 / 100)
    pq = np.linspace(phi[0], phi[-1], N_PHI)
    i = np.clip(np.searchsorted(phi, pq), 1, a.size - 1)
    a_phi = (a[i] - a[i - 1]) / (phi[i] - phi[i - 1]) * (pq - phi[i - 1]) + a[i - 1]
    Dq = (1 + w0) * a_phi**3 + 1 - w0
    V = (2 - 2 * (1 + w0) * a_phi**3 / Dq) * (4 / Dq**2) / 2
    t0 = np.interp(1.0, a, t)
    tq = np.linspace(t[10], min(1.5 * t0, 0.95 * t[-1]), N_T)
    j = np.clip(np.searchsorted(t, tq), 1, a.size - 1)
    a_t = (a[j] - a[j - 1]) / (t[j] - t[j - 1]) * (tq - t[j - 1]) + a[j - 1]
    return V, a_t, t0, np.interp(1.0, a, phi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_field_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[10**5, 10**6])
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("field_probe needs an MI355X")
    Q, dev = amd.quintessence, torch.device("cuda:0")
    model = Q.Model(columns={"H0": 0, "Om": 1, "w0": 2}, n_a=N_A)
    out = {"probe": "field_probe", "device": torch.cuda.get_device_name(0), "reps": a.reps, "n_a": N_A, "n_phi": N_PHI, "n_t": N_T,
           "rows_per_launch": CHUNK, "ops_per_node": OPS_PER_NODE, "sizes": {}}
    gen = torch.Generator(device=dev).manual_seed(1)
    for S in a.rows:
        x = torch.tensor([66.53, 0.312, -0.763], dtype=torch.float64, device=dev) + torch.tensor(
            [0.6, 0.008, 0.06], dtype=torch.float64, device=dev) * torch.randn((S, 3), dtype=torch.float64, device=dev, generator=gen)
        x[:, 2].clamp_(min=-0.999)

        def full():
            for k0 in range(0, S, CHUNK):
                Q.reconstruct(model, x[k0:k0 + CHUNK], phi=N_PHI, t=N_T, _want=("V_phi", "a_t", "scalars", "status"))

        def table_only():
            for k0 in range(0, S, CHUNK):
                Q.reconstruct(model, x[k0:k0 + CHUNK], _want=("scalars", "status"))

        res = {}
        for name, fn in (("full", full), ("table_only", table_only)):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            med = float(np.median(ts))
            res[name] = {"ms": {"median": med, "min": float(min(ts)), "max": float(max(ts))}, "launches": -(-S // CHUNK),
                         "rows_per_s": S / (med * 1e-3), "node_evaluations_per_s": S * N_A / (med * 1e-3)}
        res["table_only"]["fp64_ops_per_s"] = res["table_only"]["node_evaluations_per_s"] * sum(OPS_PER_NODE.values())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = x.cpu().numpy()
        res["copy_to_host_ms"] = (time.perf_counter() - t0) * 1e3
        grid = np.linspace(1e-8, 5, N_A)
        t0 = time.perf_counter()
        for r in host[:200]:
            host_row(*r, grid)
        per_row = (time.perf_counter() - t0) / 200
        res["numpy_host"] = {"rows_timed": 200, "ms_per_row": per_row * 1e3, "extrapolated_s": per_row * S,
                             "over_device_full": per_row * S / (res["full"]["ms"]["median"] * 1e-3)}
        out["sizes"][str(S)] = res
        del x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
