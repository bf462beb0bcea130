#!/usr/bin/env python3
"""Cost of the Gaussian-process kernels (csrc/cosmofit_gp.hip) against the same arithmetic in plain torch on the same device
and inputs; writes one JSON file.

At n = 38 (the cosmic-chronometer data) and n = 64 (the largest size the kernels take; synthetic data of tests/gp_shapes.py):

* ``cf_gp_mll_device`` at W = 64, 4096 and 65536 rows;
* ``cf_gp_predict_device`` at S = 4096 rows x 100 test redshifts;
* the torch pipeline the reference's own arithmetic amounts to: build K [W, n, n], ``torch.linalg.cholesky_ex``,
  ``cholesky_solve``, log-determinant (and two ``solve_triangular`` for the predictions), with its per-phase split
  (build K / factor / solve);
* the wall time of ``HubbleGP.fit()`` and of a 64-walker x 500-step ``ShardedEnsemble`` chain on the real data.

Times are device events around REPS back-to-back calls after a warm-up of every shape, the two sides alternating; the
median, minimum and maximum per call are kept.  The requirement recorded in the file: the fused kernels are not slower than
the torch pipeline at W = 4096.  Where the torch side of the predictions had to run in pieces (``torch_rows_per_call`` below
4096), its time includes the extra launches and the concatenation, and the ratio flatters the fused kernel by that much.

    python tools/gp_probe.py --out profiles/r11_gp_probe.json
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

W_SET, S_PRED, NZ_PRED = (64, 4096, 65536), 4096, 100
TORCH_PREDICT_ROWS = (4096, 1024, 256, 64)  # tried in turn: the largest piece torch's batched solve accepts


def _event_ms(fn, reps, inner):
    """Per-call milliseconds of fn: `reps` windows of `inner` back-to-back calls between two events."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def _stats(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def _alternate(fns: dict, reps, inner):
    """Warm every entry up, then time them in turn, `reps` rounds."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k] += _event_ms(f, 1, inner)
    return {k: _stats(v) for k, v in ts.items()}


class TorchGP:
    """The pipeline in plain torch, float64, on the device: what the reference's arithmetic costs without the fused kernels."""

    def __init__(self, z, y, C, dev):
        self.z, self.y, self.C = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (z, y, C))
        self.dz2 = (self.z[:, None] - self.z[None, :]) ** 2
        self.n = len(z)

    def build(self, th):
        return th[:, 1, None, None] * torch.exp(-self.dz2[None] / (2 * th[:, 2, None, None] ** 2)) + th[:, 3, None, None] * self.C[None]

    def factor(self, K):
        return torch.linalg.cholesky_ex(K)[0]

    def solve(self, Lw, th):
        r = (self.y[None, :] - th[:, 0, None])[:, :, None]
        alpha = torch.cholesky_solve(r, Lw)
        quad = (r * alpha).sum((1, 2))
        logdet = 2 * torch.log(torch.diagonal(Lw, dim1=1, dim2=2)).sum(1)
        return -0.5 * quad - 0.5 * logdet - 0.5 * self.n * math.log(2 * math.pi)

    def mll(self, th):
        return self.solve(self.factor(self.build(th)), th)

    def predict(self, th, zs, noise):
        Lw = self.factor(self.build(th))
        r = (self.y[None, :] - th[:, 0, None])[:, :, None]
        alpha = torch.cholesky_solve(r, Lw)[:, :, 0]
        d = self.z[None, :, None] - zs[None, None, :]
        l2 = th[:, 2, None, None] ** 2
        ks = th[:, 1, None, None] * torch.exp(-(d * d) / (2 * l2))
        dks = ks * d / l2
        v = torch.linalg.solve_triangular(Lw, ks, upper=False)
        u = torch.linalg.solve_triangular(Lw, dks, upper=False)
        sf2 = th[:, 1, None]
        return torch.stack([th[:, 0, None] + (ks * alpha[:, :, None]).sum(1), sf2 - (v * v).sum(1) + th[:, 3, None] * noise,
                            (dks * alpha[:, :, None]).sum(1), sf2 / l2[:, :, 0] - (u * u).sum(1), -(v * u).sum(1)], dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_gp_probe.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-wall", action="store_true", help="skip fit() and the chain")
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("gp_probe needs an MI355X")
    import gp_shapes as GS

    L, so, dev = amd._lib, amd.lib(), torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {"probe": "gp_probe", "reps": a.reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in (38, 64):
        z, y, C, b = GS.data(n)[:4]
        g = amd.gp.HubbleGP(z, y, C, bounds=b, normalise=False)
        tg = TorchGP(z, y, C, dev)
        res = {"info": g.info(), "mll": {}, "predict": {}}
        rng = np.random.default_rng(n)
        for W in W_SET:
            th = torch.from_numpy(b[:, 0] + rng.uniform(0.02, 0.98, (W, 4)) * (b[:, 1] - b[:, 0])).to(dev).contiguous()
            o = torch.empty(W, dtype=torch.float64, device=dev)
            fused = lambda: L.check(so.cf_gp_mll_device(g._h, th.data_ptr(), W, o.data_ptr(), None, stream))
            inner = max(1, min(50, 200000 // W))
            K = tg.build(th)
            Lw = tg.factor(K)
            t = _alternate({"fused": fused, "torch": lambda: tg.mll(th), "torch_build_K": lambda: tg.build(th),
                            "torch_factor": lambda: tg.factor(K), "torch_solve_logdet": lambda: tg.solve(Lw, th)}, a.reps, inner)
            fused()
            diff = float(torch.max(torch.abs(o - tg.mll(th)) / torch.abs(o)))
            res["mll"][str(W)] = {"rows": W, "calls_per_window": inner, "ms": t, "torch_over_fused": t["torch"]["median"] / t["fused"]["median"],
                                  "rows_per_s_fused": W / (t["fused"]["median"] * 1e-3), "max_rel_diff_fused_vs_torch": diff}
            del K, Lw
            torch.cuda.empty_cache()
        th = torch.from_numpy(b[:, 0] + rng.uniform(0.02, 0.98, (S_PRED, 4)) * (b[:, 1] - b[:, 0])).to(dev).contiguous()
        zs = torch.linspace(0.0, float(np.max(z)), NZ_PRED, dtype=torch.float64, device=dev)  # cc_gp.py:75
        o = torch.empty((S_PRED, NZ_PRED, 5), dtype=torch.float64, device=dev)
        fused = lambda: L.check(so.cf_gp_predict_device(g._h, th.data_ptr(), S_PRED, zs.data_ptr(), NZ_PRED, 1e-4, o.data_ptr(), stream))
        # torch's batched triangular solve can refuse 4096 x n x 100 (HIPBLAS_STATUS_ALLOC_FAILED): then the torch side runs
        # in pieces, which costs it extra launches and a concatenation.  Any other error is not a reason to go on.
        rows_per_call = None
        for cand in TORCH_PREDICT_ROWS:
            try:
                tg.predict(th[:cand], zs, 1e-4)
                torch.cuda.synchronize()
                rows_per_call = cand
                break
            except RuntimeError as e:
                if "HIPBLAS_STATUS_ALLOC_FAILED" not in str(e):
                    raise
                print(f"torch predict at {cand} rows per call: {str(e).splitlines()[0]}", file=sys.stderr)
        if rows_per_call is None:
            sys.exit("the torch pipeline could not predict at any piece size")
        torch_predict = lambda: torch.cat([tg.predict(th[k:k + rows_per_call], zs, 1e-4) for k in range(0, S_PRED, rows_per_call)])
        t = _alternate({"fused": fused, "torch": torch_predict}, a.reps, 5)
        fused()
        ref = torch_predict()
        scale = torch.amax(torch.abs(ref), dim=(0, 1))
        res["predict"] = {"rows": S_PRED, "redshifts": NZ_PRED, "torch_rows_per_call": rows_per_call, "ms": t, "torch_over_fused": t["torch"]["median"] / t["fused"]["median"],
                          "points_per_s_fused": S_PRED * NZ_PRED / (t["fused"]["median"] * 1e-3),
                          "max_diff_over_column_max_fused_vs_torch": float(torch.max(torch.amax(torch.abs(o - ref), dim=(0, 1)) / scale))}
        out["sizes"][str(n)] = res
        g.close()
        del tg
        torch.cuda.empty_cache()
    ok = all(out["sizes"][k]["mll"]["4096"]["torch_over_fused"] >= 1.0 and out["sizes"][k]["predict"]["torch_over_fused"] >= 1.0
             for k in out["sizes"])
    out["requirement_fused_not_slower_than_torch_at_4096"] = bool(ok)

    if not a.skip_wall:
        g = amd.gp.HubbleGP(*GS.raw_data(38))
        g.fit()  # warm-up: code objects, the optimizer's kernels
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = g.fit()
        torch.cuda.synchronize()
        out["fit"] = {"wall_s": time.perf_counter() - t0, "n_starts": 32, "iterations": fit.problems.iterations,
                      "likelihood_rows": fit.problems.n_like, "x": fit.x.tolist(), "log_ml_normalised": fit.log_prob + g.log_norm,
                      "physical": g.physical(fit.x).tolist(), "converged": bool(fit.best_converged)}
        bb = g.bounds
        w = bb[:, 1] - bb[:, 0]
        lo, hi = np.maximum(bb[:, 0] + 1e-3 * w, fit.x - 0.1 * w), np.minimum(bb[:, 1] - 1e-3 * w, fit.x + 0.1 * w)
        start = torch.from_numpy(lo + np.random.default_rng(1).uniform(0, 1, (64, 4)) * (hi - lo)).to(dev)
        amd.ensemble.ShardedEnsemble(g.torch_log_prob(), start, seed=1).run_mcmc(20)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ens = amd.ensemble.ShardedEnsemble(g.torch_log_prob(), start, seed=2)
        ens.run_mcmc(500)
        torch.cuda.synchronize()
        out["chain_64x500"] = {"wall_s": time.perf_counter() - t0, "acceptance_fraction": ens.acceptance_fraction()}
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
