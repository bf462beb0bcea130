#!/usr/bin/env python3
"""
Generate the quasar fixtures tests/golden/qsr_*.npz by RUNNING THE REFERENCE's quasars/ scripts.

Run from the repo root, in the build container only (needs the reference checkout):

    python tests/golden/generate_quasars.py [case ...]

The helpers (entering the reference, the seeded synthetic SN covariance, the theta batch, the Pantheon+ / Dovekie
injections) are imported from generate_golden.py unchanged.  The quasar scripts import emcee and corner at top level;
neither is needed to evaluate a likelihood, so both are stubbed as empty modules, and matplotlib runs headless.

SN sets whose matrices are not in the snapshot use the real columns with ``synthetic_cov(sigma)`` (the tests rebuild it
from the stored sigma).  ``y2024DES`` is absent entirely: a DES-shaped stand-in (the Dovekie columns, same recipe) is
injected as ``y2024DES.data``.  Each case runs in its own subprocess (the scripts hold their data at module level).
"""
import os
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate_golden as gg  # noqa: E402

QTY = {"DV_over_rs": 0, "DM_over_rs": 1, "DH_over_rs": 2}

# "Flat wzCDM" medians of each script's closing docstring, and the chi^2 it prints there
MEDIANS = {
    "qsr_pantheon": ([-0.137, 0.386, -19.352, 0.356, -1.066], dict(sn=1404.47, qsr=19.64)),
    "qsr_des5y": ([-0.093, 0.408, 0.024, 0.373, -1.052], dict(sn=1641.56, qsr=48.63)),
    "qsr_union3": ([-0.101, 0.391, -0.064, 0.350, -0.893], dict(sn=22.94, qsr=19.71)),
    "qsr_desi": ([-0.125, 0.405, 139.974, 0.312, -0.787], dict(bao=8.36, qsr=19.85)),
    "qsr_des5y_desi": ([-0.134, 0.408, 0.033, 140.800, 0.309, -0.836], dict(sn=1638.08, qsr=19.55)),
}
# qsr_des5y_desi.py has no bounds array: the inequalities of its log_prior
DES5Y_DESI_BOX = np.array([(-1, 1), (0, 2.5), (-0.6, 0.6), (110, 170), (0, 0.6), (-1.5, 0)], dtype=np.float64)


def _stubs():
    os.environ["MPLBACKEND"] = "Agg"
    for name in ("emcee", "corner"):
        sys.modules[name] = types.ModuleType(name)


def _inject_des5y():
    z, zh, mu, sig = gg._inject_dovekie()
    cov = gg.synthetic_cov(sig)
    pkg = types.ModuleType("y2024DES")
    pkg.__path__ = []
    mod = types.ModuleType("y2024DES.data")
    mod.get_data = lambda: ("DES-SN5YR stand-in (Dovekie columns, synthetic cov)", z, zh, mu, cov)
    sys.modules["y2024DES"] = pkg
    sys.modules["y2024DES.data"] = mod
    return z, zh, mu, sig


def _a(x):
    return np.asarray(x, dtype=np.float64).copy()


def run_case(name):
    _stubs()
    gg._enter_reference()
    script = name if name != "qsr_union3_unbinned" else "qsr_union3"
    sn_sigma = None
    if script == "qsr_pantheon":
        sn_sigma = gg._inject_pantheon()[3]
    elif script in ("qsr_des5y", "qsr_des5y_desi"):
        sn_sigma = _inject_des5y()[3]
    if name == "qsr_union3_unbinned":
        import y2018quasars.data as qd
        qd.get_binned_data = lambda *a, **k: qd.get_data()  # the whole catalogue instead of the 22 bins
    import importlib
    m = importlib.import_module("quasars." + script)

    box = DES5Y_DESI_BOX if script == "qsr_des5y_desi" else np.asarray(m.bounds, dtype=np.float64)
    rng = np.random.default_rng(sum(name.encode()))
    med, printed = MEDIANS[script]
    thetas = np.vstack([gg.theta_batch(box, 12, rng), [med]])
    out = dict(bounds=box, thetas=thetas, printed_sn=np.float64(printed.get("sn", np.nan)),
               printed_qsr=np.float64(printed["qsr"]), printed_bao=np.float64(printed.get("bao", np.nan)))

    if script == "qsr_des5y_desi":
        qz, qmu = m.z_qsr, m.mu_qsr
    else:
        qz, qmu = m.z, m.mu
    out.update(qsr_z=_a(qz), qsr_mu=_a(qmu), qsr_sigma=_a(m.sigma_mu))
    has_sn = script != "qsr_desi"
    has_bao = script in ("qsr_desi", "qsr_des5y_desi")
    if has_sn:
        if script == "qsr_des5y_desi":
            sz, szh, sobs = m.z_sn, m.z_hel_sn, m.mu_sn
        elif script == "qsr_pantheon":
            sz, szh, sobs = m.sn_z, m.sn_z_hel, m.sn_mag
        elif script == "qsr_des5y":
            sz, szh, sobs = m.sn_z, m.sn_z_hel, m.sn_mu
        else:
            sz, szh, sobs = m.sn_z, m.sn_zhel, m.sn_mu
        out.update(sn_z=_a(sz), sn_zhel=_a(szh), sn_obs=_a(sobs))
        if sn_sigma is not None:
            out["sn_sigma"] = _a(sn_sigma)  # covariance = generate_golden.synthetic_cov(sn_sigma)
        else:
            out["sn_cov"] = _a(m.sn_cov)
    if has_bao:
        out.update(bao_z=_a(m.bao_data["z"]), bao_val=_a(m.bao_data["value"]), bao_cov=_a(m.bao_cov),
                   bao_qty=np.array([QTY[str(q)] for q in m.bao_data["quantity"]], dtype=np.int32))

    def parts(t):
        """(chi2_sn, chi2_qsr, chi2_bao), mu at the SN z, mu at the quasar z, BAO predictions -- the script's own functions."""
        nb = len(m.bao_data) if has_bao else 0
        if script == "qsr_desi":
            c2q = m.chi_squared_quasar(t)
            return (0.0, c2q, m.chi_squared_bao(t)), np.zeros(0), _a(m.mu_model(qz, t)), _a(m.bao_predictions(t))
        if script == "qsr_des5y_desi":
            return ((m.chi_squared_sn(t), m.chi_squared_quasar(t), m.chi_squared_bao(t)), _a(m.mu_theory(szh, sz, t)),
                    _a(m.mu_theory(qz, qz, t)), _a(m.bao_predictions(t)))
        c2s, mu_u = m.chi_squared_sn(t)
        c2q, _ = m.chi_squared_quasar(mu_u, t)
        return (c2s, c2q, 0.0), _a(np.interp(sz, m.z_unique, mu_u)), _a(np.interp(qz, m.z_unique, mu_u)), np.zeros(nb)

    def guarded(f, t, fail):
        """cho_solve refuses a non-finite residual (rows outside the box, e.g. Omega_m < 0): NaN there."""
        try:
            return f(t)
        except ValueError:
            return fail

    nan_parts = ((np.nan,) * 3, np.full(len(sz) if has_sn else 0, np.nan), np.full(len(qz), np.nan),
                 np.full(len(m.bao_data) if has_bao else 0, np.nan))
    with np.errstate(all="ignore"):
        res = [guarded(parts, t, nan_parts) for t in thetas]
        out["chi2_parts"] = np.array([r[0] for r in res], dtype=np.float64)
        out["logl"] = np.array([guarded(m.log_likelihood, t, np.nan) for t in thetas], dtype=np.float64)
        out["logp"] = np.array([m.log_posterior(t) for t in thetas], dtype=np.float64)
    # theory vectors of three rows: the docstring medians and the first two in-box rows
    rows = np.array([len(thetas) - 1, 0, 1])
    out["theory_rows"] = rows
    if has_sn:
        out["mu_sn"] = np.array([res[r][1] for r in rows])
    out["mu_qsr"] = np.array([res[r][2] for r in rows])
    if has_bao:
        out["bao_theory"] = np.array([res[r][3] for r in rows])
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "chi2 parts at the docstring medians:", out["chi2_parts"][-1], "size", os.path.getsize(path))


CASES = ["qsr_pantheon", "qsr_des5y", "qsr_union3", "qsr_desi", "qsr_des5y_desi", "qsr_union3_unbinned"]

if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--run":
        run_case(sys.argv[2])
        sys.exit(0)
    for case in sys.argv[1:] or CASES:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--run", case], check=True)
