"""Shapes, rows and queries of the field tests (tests/test_field_cpu.py, tests/test_gpu_field_kernels.py), and the comparison
against the extended-precision restatement with the bars of the feature:

    phi(a_q), phi(t_q), phi_today, phi_max, own phi grid      abs <= 1e-10 phi_max(row)
    K(a), V(a)                                                abs <= 1e-10 rho_de(a)
    w(a)                                                      abs <= 1e-10
    V(phi_q), a(phi_q), t(a_q), a(t_q), t_today, t_max, Hubble time, own t grid      relative 1e-10

The sizes are the smallest at which the kernel takes another path: n_a below, at and above a wave (63, 64, 65), above half a
workgroup's threads (257), below one node per thread (16), the script's 5000 (16 nodes per thread, 313 threads, 5 waves of
carries) and the cap 8192 (every thread); S of 1, 2 and 65 rows; query counts around a wave and above 256."""
import numpy as np

import field_reference as fr

TOL = 1e-10
N_A = (16, 63, 64, 65, 257, 5000, 8192)
S_SIZES = (1, 2, 65)
N_Q = (1, 2, 65, 257)
ORH2 = 4.1835e-05

# name -> Model arguments
MODELS = {
    "thawing": dict(fde="thawing", columns={"H0": 0, "Om": 1, "w0": 2}),
    "thawing_h": dict(fde="thawing", columns={"H0": 3, "Om": 0, "w0": 4}, scale={"H0": 100.0}, ndim=5),  # theta holds h, two idle columns
    "wcdm": dict(fde="wcdm", columns={"H0": 0, "Om": 1, "w0": 2}),
    "wcdm_fixed": dict(fde="wcdm", columns={"H0": 0, "w0": 1}, fixed={"Om": 0.3}),
    "cpl": dict(fde="cpl", columns={"w0": 0, "wa": 1, "H0": 2, "Om": 3}),
}
PLANTED = {"phantom": 7, "invalid": 8, "nan": 9}  # rows of a 65-row batch


def physical(name, S, seed):
    """[S, 4] (H0, Om, w0, wa): seeded rows inside the model's canonical range, row 0 of a thawing model at w0 = -0.999, CPL with
    wa of both signs; in a 65-row batch the planted rows: a phantom one (w0 = -1.2; not in the thawing models, whose D changes
    sign there), one whose E^2 turns negative (Om = -5; H0 = -70 where Om is fixed) and one with a NaN."""
    rng = np.random.default_rng(seed)
    fde = MODELS[name]["fde"]
    p = np.zeros((S, 4))
    p[:, 0], p[:, 1] = rng.uniform(55, 85, S), rng.uniform(0.1, 0.6, S)
    if fde == "thawing":
        p[:, 2] = rng.uniform(-0.999, -0.34, S)
        p[0, 2] = -0.999
    elif fde == "wcdm":
        p[:, 2] = rng.uniform(-0.95, -0.4, S)
    else:
        pos = np.arange(S) % 2 == 0
        p[:, 2] = np.where(pos, rng.uniform(-0.8, -0.7, S), rng.uniform(-0.6, -0.5, S))
        p[:, 3] = np.where(pos, rng.uniform(0.01, 0.04, S), rng.uniform(-0.3, -0.1, S))
    if "Om" in MODELS[name].get("fixed", {}):
        p[:, 1] = MODELS[name]["fixed"]["Om"]
    if S >= 65:
        if fde != "thawing":
            p[PLANTED["phantom"], 2:] = (-1.2, 0.0)
        if "Om" in MODELS[name].get("fixed", {}):
            p[PLANTED["invalid"], 0] = -70.0
        else:
            p[PLANTED["invalid"], 1] = -5.0
        p[PLANTED["nan"], 0] = np.nan
    return p


def planted(name, S):
    """{row: status} of the planted rows of an S-row batch of `physical`."""
    if S < 65:
        return {}
    rows = {PLANTED["invalid"]: 2, PLANTED["nan"]: 2}
    if MODELS[name]["fde"] != "thawing":
        rows[PLANTED["phantom"]] = 1
    return rows


def theta_of(name, phys):
    """The sampler's rows for physical rows: columns placed, scales undone, idle columns filled with a number no one reads."""
    m = MODELS[name]
    ndim = m.get("ndim", max(m["columns"].values()) + 1)
    th = np.full((phys.shape[0], ndim), 123.456)
    for n, c in m["columns"].items():
        th[:, c] = phys[:, ("H0", "Om", "w0", "wa").index(n)] / m.get("scale", {}).get(n, 1.0)
    return th


def effective(name, theta):
    """The physical rows the kernel sees: scale * theta in float64, as the slot read-out."""
    m = MODELS[name]
    p = np.zeros((theta.shape[0], 4))
    for j, n in enumerate(("H0", "Om", "w0", "wa")):
        if n in m["columns"]:
            p[:, j] = m.get("scale", {}).get(n, 1.0) * theta[:, m["columns"][n]]
        elif n in m.get("fixed", {}):
            p[:, j] = m["fixed"][n]
    return p


def a_queries(n, n_a, a_min, a_max, seed):
    """Unsorted: below a_min, above a_max, exact nodes (the second, a middle one, the last), today, a NaN, and log-uniform
    points inside; the first n of a seeded shuffle that keeps the NaN when n >= 2."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(a_min, a_max, n_a)
    special = [np.nan, grid[1], a_min / 2, a_max * 1.5, grid[n_a // 2], grid[-1], 1.0, grid[0]]
    q = np.concatenate([special, np.exp(rng.uniform(np.log(a_min), np.log(a_max), max(n, 8)))])
    head, rest = q[:2], q[2:]
    rng.shuffle(rest)
    q = np.concatenate([head, rest])[:n] if n >= 2 else np.array([grid[n_a // 2]])
    rng.shuffle(q)
    return q


def x_queries(n, lo, hi, seed, negative):
    """Unsorted points in [lo, hi] with both ends, one NaN when n >= 2 and, when n >= 65, one point at `negative`."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(lo, hi, n)
    if n >= 2:
        q[0], q[1] = np.nan, hi
    if n >= 65:
        q[2], q[3] = lo, negative
    rng.shuffle(q)
    return q


def reference_rows(name, theta, n_a, a_q=None, phi_q=None, t_q=None, a_min=1e-8, a_max=5.0):
    fde = MODELS[name]["fde"]
    return [fr.row(fde, *p, orh2=ORH2, n_a=n_a, a_min=a_min, a_max=a_max, a_q=a_q, phi_q=phi_q, t_q=t_q) for p in effective(name, theta)]


_PHI_LIKE = ("phi_a", "phi_t", "phi_today", "phi_max", "phi_grid")
_RHO_LIKE = ("K_a", "V_a")
_REL = ("V_phi", "a_phi", "t_a", "a_t", "t_today", "t_max", "hubble_time", "t_grid")


def compare(got, refs, skip_rows=(), skip_points=None):
    """Largest error of every quantity in units of its bar: {name: max(err / bar)} (<= 1 passes).  `got`: numpy arrays [S, ...]
    of the device; refs: the restatement's rows.  NaNs must sit at the same places.  skip_points: {name: boolean mask [n]} of
    query points left out of the comparison of values."""
    worst = {}
    for i, ref in enumerate(refs):
        if i in skip_rows:
            continue
        for k in _PHI_LIKE + _RHO_LIKE + _REL + ("w_a",):
            if k not in got or k not in ref or got[k].ndim == 1 and k.endswith("_grid"):
                continue
            g, r = np.atleast_1d(got[k][i]).astype(np.longdouble), np.atleast_1d(ref[k])
            if skip_points and k in skip_points:
                g, r = g[~skip_points[k]], r[~skip_points[k]]
            assert np.array_equal(np.isnan(g), np.isnan(r)), (k, i)
            ok = ~np.isnan(r)
            if not ok.any():
                continue
            if k in _PHI_LIKE:
                bar = TOL * ref["phi_max"]
            elif k in _RHO_LIKE:
                bar = (TOL * ref["rho_a"])[~skip_points[k]] if skip_points and k in skip_points else TOL * ref["rho_a"]
                bar = bar[ok]
            elif k == "w_a":
                bar = TOL
            else:
                bar = TOL * np.abs(r[ok])
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.abs(g[ok] - r[ok]) / bar
            err = np.where((g[ok] == r[ok]), 0.0, err)  # an exact zero against a zero bar
            worst[k] = max(worst.get(k, 0.0), float(np.max(err)))
    return worst
