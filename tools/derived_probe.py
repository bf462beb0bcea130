#!/usr/bin/env python3
"""Cost of derived parameters and prediction bands on the device against numpy on a host copy; writes one JSON file.

Shapes: a [2500 x 4096, 3] cmb/cmb.py-shaped chain (H0, wb, wc; Planck+ACT compression) and a 2 x 10^5-row weighted
posterior of bao/desi_cmb_union3_fs8.py's six parameters.  On each, device-synchronised wall time (median of REPS calls after
one warm-up call) of

* ``derived.columns`` of the closed-form quantities alone, with the bytes they read and write over that time;
* ``derived.columns`` of the five Gauss-Legendre quantities (2 x 100 evaluations of H per row), with the H evaluations per
  second;
* ``derived.augment`` + ``marginals.corner_data`` (cmb/cmb.py: the eight-parameter triangle of :142);

and a 200-redshift D_V / r_d band (``derived.bands``, bao/desi_cmb.py's engine, 4000-node table per sample) on 10^5 and 10^6
rows, with the table nodes per second of its ``derived.curves`` part.

The host side is the float64 form of tests/derived_reference.py on a host copy of the same rows (the copy timed alone): in
full for the closed forms, on the first NUMPY_ROWS rows for the Gauss-Legendre quantities and the first NUMPY_CURVE_ROWS rows
for the curves (per-row Python there), scaled to the full size and marked ``extrapolated``.

    python tools/derived_probe.py --out profiles/r10_derived_probe.json
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

NUMPY_ROWS, NUMPY_CURVE_ROWS = 100_000, 200
GL = ["theta_star100", "rs_star", "DM_star", "R", "lA"]


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _median_ms(fn, reps):
    fn()
    ts = [_timed(fn)[0] * 1e3 for _ in range(reps)]
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def _rows(n, mean, sd, dev, seed, weighted=False):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    k = len(mean)
    x = torch.tensor(mean, device=dev, dtype=torch.float64) + \
        torch.randn((n, k), generator=g, device=dev, dtype=torch.float64) * torch.tensor(sd, device=dev, dtype=torch.float64)
    w = torch.exp(1.5 * torch.randn(n, generator=g, device=dev, dtype=torch.float64)) if weighted else None
    return x.contiguous(), w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_derived_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every row count (rehearsals)")
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("derived_probe needs an MI355X")
    import derived_reference as R
    import derived_shapes as DS

    R.LD = np.float64  # the host side is what a script would run: float64 numpy
    D, M, dev = amd.derived, amd.marginals, torch.device("cuda:0")
    out = {"probe": "derived_probe", "reps": a.reps, "numpy_rows": NUMPY_ROWS, "numpy_curve_rows": NUMPY_CURVE_ROWS, "shapes": {},
           "bands": {}}

    shapes = (("cmb_chain", "cmb_cmb", int(2500 * 4096 * a.scale), [67.3, 0.02236, 0.1202], [0.6, 1.5e-4, 1.4e-3], False,
               ["omh2", "Om", "z_drag", "r_drag", "z_eq", "z_star"], ["theta_star100", "H0", "Om", "DM_star", "rs_star", "z_star",
                                                                     "z_drag", "r_drag"]),
              ("union3_fs8_posterior_weighted", "desi_cmb_union3_fs8", int(200_000 * a.scale),
               [0.0, 67.5, 0.0224, 0.119, 0.0, 0.8], [0.03, 0.5, 1.4e-4, 1e-3, 1.0, 0.03], True,
               ["omh2", "Om", "S8", "rd", "q0", "j0"], None))
    for name, case, n, mean, sd, weighted, closed, triangle in shapes:
        eng = amd.LikelihoodEngine(**DS.engine_kwargs(amd, case))
        consts = DS.consts(amd, case)
        x, w = _rows(n, mean, sd, dev, 100 + len(mean), weighted)
        k = x.shape[1]
        res = {"rows": n, "columns": k, "weighted": weighted, "closed_form": closed, "gauss_legendre": GL}
        s_closed, s_gl = D.Spec(eng, closed, **consts), D.Spec(eng, GL, **consts)
        res["closed_form_ms"] = _median_ms(lambda: D.columns(s_closed, x), a.reps)
        res["closed_form_GB_per_s"] = n * (k + len(closed)) * 8 / (res["closed_form_ms"]["median"] * 1e-3) / 1e9
        res["gauss_legendre_ms"] = _median_ms(lambda: D.columns(s_gl, x), a.reps)
        res["gauss_legendre_H_evaluations_per_s"] = n * 200 / (res["gauss_legendre_ms"]["median"] * 1e-3)
        if triangle is not None:  # cmb/cmb.py:142: thetastar, H0, omegam, DAstar, rstar, zstar, zdrag, rdrag
            s_tri = D.Spec(eng, [t for t in triangle if t != "H0"], **consts)

            def tri():
                aug = D.augment(s_tri, x)
                return M.corner_data(aug[:, [3, 0, 4, 5, 6, 7, 8, 9]].contiguous(), weights=w)
        else:
            s_tri = D.Spec(eng, closed, **consts)

            def tri():
                return M.corner_data(D.augment(s_tri, x), weights=w)
        res["augment_corner_data_ms"] = _median_ms(tri, max(2, a.reps // 2))
        res["corner_data_alone_ms"] = _median_ms(lambda: M.corner_data(x, weights=w), max(2, a.reps // 2))
        if not a.skip_numpy:
            model = DS.model(amd, case)
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            res["device_to_host_copy_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref = R.scalars(model, xh, closed)
            res["numpy_closed_form_s"] = time.perf_counter() - t0
            got = D.columns(s_closed, x).cpu().numpy()
            res["closed_form_max_rel_diff_to_numpy"] = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))
            m = min(n, NUMPY_ROWS)
            t0 = time.perf_counter()
            R.scalars(model, xh[:m], GL)
            t = time.perf_counter() - t0
            res["numpy_gauss_legendre_s"] = {"rows": m, "seconds": t, "extrapolated_to_all_rows": t * n / m}
        out["shapes"][name] = res
        del x, w
        eng.close()
        torch.cuda.empty_cache()

    eng = amd.LikelihoodEngine(**DS.engine_kwargs(amd, "desi_cmb_thawing"))
    z = np.linspace(0.0, 2.33, 200)  # bao/plot_predictions.py:23
    for n in (int(100_000 * a.scale), int(1_000_000 * a.scale)):
        x, _ = _rows(n, [67.5, 0.0222, 0.119, -0.8], [0.6, 1.5e-4, 1.4e-3, 0.08], dev, 7)
        res = {"rows": n, "redshifts": 200, "n_grid": 4000, "chunk_redshifts": D.band_chunk(n, 200, 2**31)}
        res["curves_ms"] = _median_ms(lambda: D.curves(eng, x, z, "DV_rd"), a.reps)
        res["table_nodes_per_s"] = n * 4000 / (res["curves_ms"]["median"] * 1e-3)
        res["bands_ms"] = _median_ms(lambda: D.bands(eng, x, z, "DV_rd"), max(2, a.reps // 2))
        if not a.skip_numpy:
            model = DS.model(amd, "desi_cmb_thawing")
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            res["device_to_host_copy_s"] = time.perf_counter() - t0
            m = min(n, NUMPY_CURVE_ROWS)
            t0 = time.perf_counter()
            R.curves(model, xh[:m], z, "DV_rd")
            t = time.perf_counter() - t0
            res["numpy_curves_s"] = {"rows": m, "seconds": t, "extrapolated_to_all_rows": t * n / m}
            curve = D.curves(eng, x, z, "DV_rd").cpu().numpy()
            t0 = time.perf_counter()
            np.percentile(curve, [15.9, 50.0, 84.1], axis=0)
            res["numpy_percentile_of_host_curves_s"] = time.perf_counter() - t0
        out["bands"][str(n)] = res
        del x
        torch.cuda.empty_cache()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
