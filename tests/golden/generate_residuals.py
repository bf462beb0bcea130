#!/usr/bin/env python3
"""
Generate tests/golden/residuals.npz: the residual block every ``main()`` of the reference ends with, by RUNNING THE REFERENCE's
own functions on 32 in-box thetas per script.

Run from the repo root, in the build container only (needs the reference checkout):

    python tests/golden/generate_residuals.py [case ...]

The post-fit blocks live inside each script's ``main()`` (they follow a sampler run), so the expressions of the cited lines are
evaluated here for every theta with the module's own functions, numpy and ``scipy.stats``: the residual vector, the corrected
data y, ss_res, ss_tot, R^2, RMSD, ``stats.skew``, ``stats.kurtosis`` and ``norm.fit`` (sn/plotting.py:52).  The helpers
(entering the reference under the numba stand-in, the synthetic Pantheon+ covariance) are generate_golden.py's, unchanged.  Each
case runs in its own subprocess; the parent merges the cases into one file, keys ``<case>/<name>``.  Only numbers are stored:
the statistics of all rows, the residual and y vectors of the first 8.  The data the tests build their engines from are in the
scripts' own fixtures (sn_pantheon.npz, sn_pantheon_and_sh0es.npz, sn_union3_1.npz, bao_desi_fs_lya.npz).

    sn_pantheon             sn/pantheon.py:152-164, 196-201
    sn_pantheon_and_sh0es   sn/pantheon_and_sh0es.py:157-165, 181-182, 198
    sn_union3_1             sn/union3_1.py:105-108, 129 (real data; the script prints no statistics of its residuals: the
                            expressions of sn/pantheon.py:157-164 on its residuals and corrected moduli)
    bao_desi_fs_lya         bao/desi_fs_lya.py:99-102, 113 (real data)
"""
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate_golden as gg  # noqa: E402

N_ROWS = 32
N_VECTOR_ROWS = 8


def _box(box, rng, n=N_ROWS):
    box = np.asarray(box, dtype=np.float64)
    return rng.uniform(box[:, 0], box[:, 1], size=(n, len(box)))


def _block(thetas, residuals_of):
    """The post-fit lines for every theta: residuals_of(theta) -> (residuals, y)."""
    import scipy.stats as stats
    from scipy.stats import norm

    cols = {k: [] for k in ("ss_res", "ss_tot", "r2", "rmsd", "skew", "kurtosis", "fit_mean", "fit_std")}
    vec_r, vec_y = [], []
    for k, t in enumerate(thetas):
        residuals, y = residuals_of(t)
        ss_res = np.sum(residuals**2)                       # sn/pantheon.py:161
        ss_tot = np.sum((y - np.mean(y)) ** 2)              # :160,162
        mu, std = norm.fit(residuals)                       # sn/plotting.py:52
        for name, v in (("ss_res", ss_res), ("ss_tot", ss_tot), ("r2", 1 - (ss_res / ss_tot)),        # :163
                        ("rmsd", np.sqrt(np.mean(residuals**2))),                                     # :164
                        ("skew", stats.skew(residuals)), ("kurtosis", stats.kurtosis(residuals)),     # :157-158
                        ("fit_mean", mu), ("fit_std", std)):
            cols[name].append(v)
        if k < N_VECTOR_ROWS:
            vec_r.append(residuals)
            vec_y.append(y)
    out = {k: np.array(v) for k, v in cols.items()}
    out.update(thetas=thetas, residuals=np.array(vec_r), y=np.array(vec_y))
    return out


def case_sn_pantheon():
    gg._enter_reference()
    gg._inject_pantheon()
    import sn.pantheon as m

    def f(t):
        DM = m.DM_z(t, m.z_cmb)                              # :152
        mB_pred = m.mu_theory(DM) + t[0]                     # :153
        corrected_mags = m.mb_vals - m.mu_corr(t, DM)        # :154
        return corrected_mags - mB_pred, corrected_mags      # :155

    return _block(_box(m.bounds, np.random.default_rng(31)), f)


def case_sn_pantheon_and_sh0es():
    gg._enter_reference()
    import pandas as pd

    # the injection of generate_golden.case_sn_pantheon_and_sh0es: the real columns, the seeded synthetic covariance
    df = pd.read_csv(os.path.join(gg.REF, "y2022pantheonSHOES/raw-data/distances.txt"), sep=" ")
    zall = df["zHD"].to_numpy(np.float64)
    sel = np.where(((zall >= 0.0) & (df["IS_CALIBRATOR"] == 1)) | (zall > 0.01))[0]
    col = lambda name: df[name].to_numpy(np.float64)[sel]  # noqa: E731
    z, zh, mb, ceph, sig = col("zHD"), col("zHEL"), col("m_b_corr"), col("CEPH_DIST"), col("m_b_corr_err_DIAG")
    cov = gg.synthetic_cov(sig)
    pkg = types.ModuleType("y2022pantheonSHOES")
    pkg.__path__ = []
    mod = types.ModuleType("y2022pantheonSHOES.data_shoes")
    mod.get_data = lambda z_cut_ceph=0.0: ("Pantheon+ and SH0ES (synthetic cov)", z, zh, mb, ceph, cov)
    sys.modules["y2022pantheonSHOES"] = pkg
    sys.modules["y2022pantheonSHOES.data_shoes"] = mod
    import sn.pantheon_and_sh0es as m

    def f(t):
        dm_cmb = m.DM_z(m.z_cmb, t)                          # :157
        mu_pred = m.mu_theory(dm_cmb)                        # :158
        mB_corrected = m.mB_vals - m.mu_corr(t, dm_cmb)      # :159
        return mB_corrected - t[0] - np.where(m.ceph_mask, m.ceph_dists, mu_pred), mB_corrected  # :160

    return _block(_box(m.bounds, np.random.default_rng(32)), f)


def case_sn_union3_1():
    gg._enter_reference()
    import sn.union3_1 as m

    def f(t):
        DM_best = m.DM_z(m.z_cmb, t)                         # :105
        mu_pred = m.mu_theory(t, DM_best)                    # :106
        mu_corrected = m.mu_vals - m.mu_corr(t, DM_best)     # :107
        return mu_corrected - mu_pred, mu_corrected          # :108

    return _block(_box([(-1.0, 1.0), (0.1, 0.7), (-9.0, 9.0)], np.random.default_rng(33)), f)  # the prior of :73-75


def case_bao_desi_fs_lya():
    gg._enter_reference()
    import bao.desi_fs_lya as m

    def f(t):
        return m.data["value"] - m.bao_theory(m.data["z"], m.bao_qty, t), np.asarray(m.data["value"], dtype=np.float64)  # :99,101

    return _block(_box([(0.5, 0.8), (0.1, 0.8), (-1.0, 0.0)], np.random.default_rng(34)), f)  # the prior of :78-80


CASES = {f.__name__[5:]: f for f in (case_sn_pantheon, case_sn_pantheon_and_sh0es, case_sn_union3_1, case_bao_desi_fs_lya)}

if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--run":
        out = CASES[sys.argv[2]]()
        np.savez(sys.argv[3], **{k: np.asarray(v, dtype=np.float64) for k, v in out.items()})
        sys.exit(0)
    path = os.path.join(HERE, "residuals.npz")
    merged = dict(np.load(path)) if os.path.exists(path) and len(sys.argv) > 1 else {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in sys.argv[1:] or list(CASES):
            part = os.path.join(tmp, case + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--run", case, part], check=True)
            merged = {k: v for k, v in merged.items() if not k.startswith(case + "/")}
            merged.update({case + "/" + k: v for k, v in np.load(part).items()})
    np.savez_compressed(path, **merged)
    print("residuals.npz", sorted({k.split("/")[0] for k in merged}), "size", os.path.getsize(path))
