#!/usr/bin/env python3
"""
Generate tests/golden/derived.npz: the derived-parameter columns the reference's post-fit blocks compute from their samples,
by RUNNING THE REFERENCE's own functions on a few hundred in-box thetas per script.

Run from the repo root, in the build container only (needs the reference checkout):

    python tests/golden/generate_derived.py [case ...]

The post-fit blocks live inside each script's ``main()`` (they follow a sampler run), so the expressions of the cited lines are
evaluated here on a theta batch with the module's own functions and constants (``cmb.z_star``, ``cmb.r_drag``, ``cmb.z_drag``,
``q0``, ``j0``, ``Omnu_h2``, ``cmb.Omega_r_h2``); cmb/cmb.py's blobs are what its ``log_likelihood`` returns.  The helpers
(entering the reference under the numba stand-in, the Dovekie injection) are generate_golden.py's, unchanged.  Each case runs in
its own subprocess (``cmb.set_HZ`` is a process-wide global of the reference); the parent merges the cases into one file, keys
``<case>/<name>``.  Only numbers are stored.

    desi_cmb_thawing, desi_cmb_lcdm   bao/desi_cmb.py:196-199 (omh2, Om, z_star, rd) as shipped (thawing) and with the
                                      LambdaCDM line of its Ode_z (:22); H_z / DM_z / bao_theory curves of four rows
    desi_cmb_union3_fs8               bao/desi_cmb_union3_fs8.py:282-287 (omh2, Om, S8, rd, q0, j0)
    desi_union3_bbn                   bao/desi_union3_bbn.py:175-178 (omh2, rd, q0, j0), and q0 / j0 of its thawing variant with
                                      the derived wa = -1.5 (1 - w0^2) of :320
    desi_des5y_obh2_theta_star        bao/desi_des5y_obh2_theta_star.py:195-198 (omh2, Om, z_drag, z_star)
    cmb_cmb                           cmb/cmb.py:45-63 blobs (100 theta*, r*, D_M* / Gpc, z*) and :118-138 addDerived columns
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate_golden as gg  # noqa: E402

N_ROWS = 300
N_CURVE_ROWS = 4


def _box(box, rng, n=N_ROWS):
    box = np.asarray(box, dtype=np.float64)
    return rng.uniform(box[:, 0], box[:, 1], size=(n, len(box)))


def _desi_cmb(lcdm):
    gg._enter_reference()
    import bao.desi_cmb as m

    if lcdm:
        m.Ode_z = lambda z, w0: 1.0  # the "# return 1  # LCDM" line of bao/desi_cmb.py:22
    cmb = m.cmb
    s = _box(m.bounds, np.random.default_rng(11 + lcdm))
    if lcdm:
        s[:, 3] = -1.0
    omh2 = s[:, 1] + s[:, 2] + m.Omnu_h2                      # :196
    om = omh2 / (s[:, 0] / 100) ** 2                          # :197
    out = dict(thetas=s, omh2=omh2, Om=om, z_star=cmb.z_star(s[:, 1], omh2), rd=cmb.r_drag(s[:, 1], omh2),  # :198-199
               z_max=np.float64(m.z_grid[-1]))
    z = np.linspace(0, max(m.bao_data["z"]), 200)             # bao/plot_predictions.py:23
    rows = s[:N_CURVE_ROWS]
    with np.errstate(all="ignore"):
        out.update(curve_z=z, H=np.array([m.H_z(z, t) for t in rows]), DM=np.array([m.DM_z(z, t) for t in rows]),
                   **{name: np.array([m.bao_theory(z, np.full(z.size, code, dtype=np.int32), t) for t in rows])
                      for code, name in ((0, "DV_rd"), (1, "DM_rd"), (2, "DH_rd"))})
    return out


def case_desi_cmb_thawing():
    return _desi_cmb(False)


def case_desi_cmb_lcdm():
    return _desi_cmb(True)


def case_desi_cmb_union3_fs8():
    gg._enter_reference()
    import bao.desi_cmb_union3_fs8 as m

    cmb = m.cmb
    # the prior of :257-263
    s = _box([(-1, 1), (50, 90), (0.01, 0.03), (0.01, 0.25), (-8.5, 8.5), (0.5, 1.5)], np.random.default_rng(13))
    omh2 = s[:, 2] + s[:, 3] + m.Omnuh2                       # :282
    om = omh2 / (s[:, 1] / 100) ** 2                          # :283
    return dict(thetas=s, omh2=omh2, Om=om, S8=s[:, 5] * (om / 0.3) ** 0.5, rd=cmb.r_drag(s[:, 2], omh2),  # :284-285
                q0=m.q0(om), j0=m.j0(om))                     # :286-287


def case_desi_union3_bbn():
    gg._enter_reference()
    import bao.desi_union3_bbn as m

    # the prior of :152-156 (the BBN normal on omega_b as +-4 sigma)
    s = _box([(55, 80), (0.10, 0.65), (m.bbn.Obh2 - 4 * m.bbn.Obh2_sigma, m.bbn.Obh2 + 4 * m.bbn.Obh2_sigma), (-12.0, 5.0), (-1.0, 1.0)],
             np.random.default_rng(17))
    omh2 = s[:, 1] * (s[:, 0] / 100) ** 2                     # :175
    w0 = np.random.default_rng(18).uniform(-1.0, -1 / 3, N_ROWS)
    wa = -1.5 * (1 - w0**2)                                   # :320
    return dict(thetas=s, omh2=omh2, rd=m.r_drag(s[:, 2], omh2), q0=m.q0(s[:, 1]), j0=m.j0(s[:, 1]),  # :176-178
                thaw_w0=w0, thaw_wa=wa, thaw_q0=m.q0(s[:, 1], w0), thaw_j0=m.j0(s[:, 1], w0, wa))


def case_desi_des5y_obh2_theta_star():
    gg._enter_reference()
    gg._inject_dovekie()
    import bao.desi_des5y_obh2_theta_star as m

    cmb = m.cmb
    s = _box(m.bounds, np.random.default_rng(19))
    omh2 = s[:, 2] + s[:, 3] + m.Omnu_h2                      # :195
    return dict(thetas=s, bounds=np.asarray(m.bounds, dtype=np.float64), omh2=omh2, Om=omh2 / (s[:, 1] / 100) ** 2,  # :196
                z_drag=cmb.z_drag(wb=s[:, 2], wm=omh2), z_star=cmb.z_star(wb=s[:, 2], wm=omh2))  # :197-198


def case_cmb_cmb():
    gg._enter_reference()
    import cmb.cmb as m

    cmb = m.cmb
    s = _box(m.bounds, np.random.default_rng(23))
    blobs = np.array([m.log_likelihood(t)[1] for t in s])     # :45-63
    omh2 = s[:, 1] + s[:, 2] + m.Omnu_h2                      # :119
    return dict(thetas=s, blobs=blobs, omh2=omh2, Om=omh2 / (s[:, 0] / 100) ** 2,  # :122
                z_drag=cmb.z_drag(s[:, 1], omh2), r_drag=cmb.r_drag(s[:, 1], omh2),  # :125,130
                z_eq=-1 + (s[:, 1] + s[:, 2]) / cmb.Omega_r_h2(), zeq_or_h2=np.float64(cmb.Omega_r_h2()))  # :135


CASES = {f.__name__[5:]: f for f in (case_desi_cmb_thawing, case_desi_cmb_lcdm, case_desi_cmb_union3_fs8, case_desi_union3_bbn,
                                     case_desi_des5y_obh2_theta_star, case_cmb_cmb)}

if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--run":
        out = CASES[sys.argv[2]]()
        np.savez(sys.argv[3], **{k: np.asarray(v, dtype=np.float64) for k, v in out.items()})
        sys.exit(0)
    path = os.path.join(HERE, "derived.npz")
    merged = dict(np.load(path)) if os.path.exists(path) and len(sys.argv) > 1 else {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in sys.argv[1:] or list(CASES):
            part = os.path.join(tmp, case + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--run", case, part], check=True)
            merged = {k: v for k, v in merged.items() if not k.startswith(case + "/")}
            merged.update({case + "/" + k: v for k, v in np.load(part).items()})
    np.savez_compressed(path, **merged)
    print("derived.npz", sorted({k.split("/")[0] for k in merged}), "size", os.path.getsize(path))
