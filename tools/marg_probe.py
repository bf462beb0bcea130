#!/usr/bin/env python3
"""Cost of the closed-form nuisance treatment (csrc/cosmofit_marg.hip) next to its measured neighbours; writes one JSON file.

Shape: the Pantheon+-shaped synthetic likelihood (sn/pantheon.py, 1701 SNe by default), one chunk of 4096 rows.  HIP events on
torch's current stream; the shapes interleaved round by round on one device (ROUNDS rounds after a warm-up of every shape), the
median and the spread (min, max) of each reported:

* the two new kernels alone (``cf_marg_apply_device`` on resident rows) for m = 1 (the offset) and m = 16;
* ``cf_marg_eval_device`` (m = 1 and m = 16) beside ``cf_mock_eval_device`` and ``cf_eval_device`` on the same rows of theta;
* ``ShardedEnsemble``, 64 walkers: steps per second and the integrated autocorrelation time of H0 with M sampled (four
  parameters) and with M marginalised (three);
* host time of ``nuisance.project`` and of ``cf_marg_create``.

    python tools/marg_probe.py --out profiles/r21_marg_probe.json
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


def _sample(amd, log_prob, box, steps, seed):
    """(steps per second, tau of every column) of a 64-walker stretch-move ensemble."""
    start = torch.from_numpy(amd.synthetic.walkers(box, 64, seed=seed)).to("cuda:0")
    ens = amd.ensemble.ShardedEnsemble(log_prob, start, seed=seed, moves=(("stretch", 1.0),))
    ens.run_mcmc(50)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ens.run_mcmc(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return steps / dt, ens.get_autocorr_time(discard=50 + steps // 5, quiet=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_marg_probe.json"))
    ap.add_argument("--n-sn", type=int, default=1701)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=2000)
    a = ap.parse_args()

    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("marg_probe needs an MI355X")
    L, N, SP, Param, dev = amd._lib, amd.nuisance, amd.sn_pantheon, amd.Param, torch.device("cuda:0")
    n, m = a.n_sn, a.rows
    syn = amd.synthetic.pantheon_like(n_sn=n, seed=0)
    full = SP.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    red = amd.LikelihoodEngine(ndim=3, z_max=full.z_max, n_grid=SP.N_GRID,
                               params=dict(offset=Param(fixed=M_REF), H0=Param(0), Om=Param(1), v=Param(2)),
                               sn=dict(z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"], z_turn=SP.Z_TURN),
                               bounds=SP.bounds[1:], gauss=[(0,) + tuple(SP.H0_PRIOR[1:])])
    rng = np.random.default_rng(1)
    A16 = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(15)])
    t0 = time.perf_counter()
    proj1 = N.project(syn["chol"], N.Templates.offset(n))
    t_project = time.perf_counter() - t0
    t0 = time.perf_counter()
    dec1 = N.Projection(proj1, device=0)
    t_create = time.perf_counter() - t0
    dec16 = N.Projection(N.project(syn["chol"], A16), device=0)
    box_m = [tuple(SP.bounds[0] - M_REF)]
    ln1 = N.LinearNuisance(red, N.Templates.offset(n), box=box_m, slots=("offset",))
    ln16 = N.LinearNuisance(red, A16)
    mocks = amd.mocks.MockSet.from_shifts(red, sn=0.1 * rng.standard_normal((8, n)))

    pitch = (n + 63) // 64 * 64
    rows = torch.zeros((m, pitch), dtype=torch.float64, device=dev)
    rows[:, :n] = torch.from_numpy(rng.standard_normal((m, n)) @ syn["chol"].T).to(dev)
    theta = torch.from_numpy(amd.synthetic.THETA_TRUE[1:] + np.array([1.0, 0.03, 0.3]) * rng.standard_normal((m, 3))).to(dev)
    mock = torch.from_numpy(rng.integers(0, 8, m).astype(np.int32)).to(dev)
    out_e = torch.empty(m, dtype=torch.float64, device=dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream

    def engine_eval():
        L.check(amd.lib().cf_eval_device(red._h, theta.data_ptr(), m, out_e.data_ptr(), L.CF_OUT_LOGP, stream()))

    kernels = _interleaved_ms({
        "marg_apply_m1": lambda: dec1.apply(rows),
        "marg_apply_m16": lambda: dec16.apply(rows),
    }, a.rounds)
    evals = _interleaved_ms({
        "cf_eval_device": engine_eval,
        "cf_mock_eval_device": lambda: mocks.log_prob(theta, mock, L.CF_OUT_LOGP),
        "cf_marg_eval_device_m1": lambda: ln1._device(theta, L.CF_OUT_LOGP),
        "cf_marg_eval_device_m16": lambda: ln16._device(theta, L.CF_OUT_LOGP),
    }, a.rounds)

    box4 = np.array([(-19.6, -19.1), (60.0, 80.0), (0.15, 0.5), (-2.0, 2.0)])
    sps4, tau4 = _sample(amd, full.engine.torch_log_prob(), box4, a.steps, seed=3)
    sps3, tau3 = _sample(amd, ln1.torch_log_prob(), box4[1:], a.steps, seed=3)

    out = {"probe": "marg_probe", "n_sn": n, "rows": m, "rounds": a.rounds, "info": red.info()["gcn_arch"],
           "slice": L.CF_MARG_SLICE, "n_slices": (n + L.CF_MARG_SLICE - 1) // L.CF_MARG_SLICE,
           "waves_in_flight": ((m + 63) // 64) * ((n + L.CF_MARG_SLICE - 1) // L.CF_MARG_SLICE) * 4,
           "project_s": t_project, "cf_marg_create_s": t_create, "probe_rel": proj1["probe_rel"],
           "kernels_ms": kernels, "evals_ms": evals,
           "row_bytes_read": int(m * n * 8), "partial_bytes": int(m * ((n + L.CF_MARG_SLICE - 1) // L.CF_MARG_SLICE) * 16 * 8),
           "kernels_m1_effective_tb_per_s": m * n * 8 / (kernels["marg_apply_m1"]["median"] * 1e-3) / 1e12,
           "ratios": {
               "m16_over_m1": _ratio(kernels, "marg_apply_m16", "marg_apply_m1"),
               "marg_eval_m1_over_cf_eval_device": _ratio(evals, "cf_marg_eval_device_m1", "cf_eval_device"),
               "marg_eval_m1_over_mock_eval": _ratio(evals, "cf_marg_eval_device_m1", "cf_mock_eval_device"),
               "marg_eval_m16_over_m1": _ratio(evals, "cf_marg_eval_device_m16", "cf_marg_eval_device_m1"),
           },
           "ensemble": {"walkers": 64, "steps": a.steps,
                        "M_sampled": {"steps_per_s": sps4, "tau": [float(x) for x in tau4], "tau_H0": float(tau4[1])},
                        "M_marginalised": {"steps_per_s": sps3, "tau": [float(x) for x in tau3], "tau_H0": float(tau3[0])}}}
    for o in (ln1, ln16, dec1, dec16, red, full.engine):
        o.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
