"""Seeded synthetic cases for the quasar kernel's shape sweep: one builder for tests/test_quasar_shapes_cpu.py (which proves
that the cases are fair) and tests/test_gpu_quasar_shapes.py (which runs them on the device).

A case is plain data: the sizes, the parameter layout (which slot is free, fixed or scaled), the synthetic catalogues and the
theta rows.  ``reference(case, dtype)`` evaluates it with the numpy restatement (tests/quasar_reference.py);
``engine_kwargs(case, Param)`` gives the keywords of ``LikelihoodEngine`` for the same case.

For the first 24 seeds every list below is walked by index, so that each value is reached whatever the generator draws;
later seeds (CF_TEST_RANDOM_SHAPES > 24) draw from the lists.
"""
import numpy as np

import quasar_reference as ref

N_GRID = [16, 17, 255, 256, 257, 1000, 3000, 4096, 4097, 8191, 8192]
N_QSR = [1, 2, 255, 256, 257, 1000, 2421, 65536]
N_SN = [0, 1, 15, 16, 17, 63, 64, 65, 257, 700]
N_BAO = [0, 1, 13, 64]
WALKERS = [1, 2, 31, 33, 100]
NKP = [(2, 2, 3), (4, 3, 4), (2, 3, 2), (2.5, 1.7, 3.3)]   # the three recipes of quasars.RECIPES and one non-integer triple
Z_TOP = ["max", "below", "above"]                          # qsr_z_top = max z, 3 % below, 3 % above
SN_GRID = ["own", "shared", "shared_above"]                # shared_above: some SNe beyond the quasar grid's top
BAO_Z = ["distinct", "equal", "pairs"]
FIXABLE = ["Om", "w0", "offset", "dM_qsr", "s"]
FIXED_VALUE = dict(Om=0.3, w0=-1.0, offset=-19.3, dM_qsr=0.1, s=0.4)
BOX = dict(dM_qsr=(-0.5, 0.5), s=(0.0, 2.5), offset=(-19.6, -19.0), rd=(110.0, 170.0), Om=(0.0, 1.0), w0=(-2.5, 0.0), H0=(60.0, 80.0))
SCALES = [100.0, 0.5, 0.01, 2.0]
N_DEFAULT = 24


def _sn(rng, n, z_hi):
    """The SN block of tests/test_gpu_random_shapes.py::_sn, with the covariance beside its factor."""
    z = np.sort(rng.uniform(0.01, z_hi, n))
    zh = z * (1 + 1e-3 * rng.standard_normal(n))
    sig = rng.uniform(0.1, 0.3, n)
    A = 0.02 * rng.standard_normal((n, min(n, 12)))
    cov = np.diag(sig**2) + A @ A.T
    obs = 25 + 5 * np.log10((1 + zh) * 4283.0 * z * (1 + 0.4 * z)) - 19.3 + 0.15 * rng.standard_normal(n)
    return z, zh, obs, cov


def build_case(seed, **force):
    """The case of a seed; ``force`` overrides drawn sizes and modes (the two fixed n_grid = 8192 cases)."""
    rng = np.random.default_rng(77000 + seed)

    def pick(name, lst, k):
        if name in force:
            return force[name]
        return lst[k % len(lst)] if seed < N_DEFAULT else lst[int(rng.integers(len(lst)))]

    c = dict(seed=seed)
    c["n_grid"] = G = int(pick("n_grid", N_GRID, seed))
    c["n_qsr"] = nq = int(pick("n_qsr", N_QSR, seed))
    c["n_sn"] = ns = int(pick("n_sn", N_SN, seed))
    c["n_bao"] = nb = int(pick("n_bao", N_BAO, seed + seed // 4))
    c["W"] = W = int(pick("W", WALKERS, seed))
    c["nkp"] = pick("nkp", NKP, seed // 2)
    c["z_top_mode"] = pick("z_top_mode", Z_TOP, seed)
    c["sn_grid_mode"] = pick("sn_grid_mode", SN_GRID, seed // 3) if ns else None
    c["sn_zhel"] = bool(pick("sn_zhel", [False, True], seed // 2)) and ns > 0
    c["bao_z_mode"] = pick("bao_z_mode", BAO_Z, seed // 2) if nb else None
    c["solve"] = ["auto", "blocked"][seed % 2]
    c["h0_free"] = bool(pick("h0_free", [True, False], seed))
    c["fixed"] = pick("fixed", FIXABLE, seed // 4) if seed % 4 == 1 else None
    if c["fixed"] == "offset" and not ns:
        c["fixed"] = "s"

    # parameter layout: the scripts' order, H0 appended where it is free
    names = ["dM_qsr", "s"] + (["offset"] if ns else []) + (["rd"] if nb else []) + ["Om", "w0"] + (["H0"] if c["h0_free"] else [])
    names = [n for n in names if n != c["fixed"]]
    c["names"] = names
    c["fixed_values"] = {} if c["fixed"] is None else {c["fixed"]: FIXED_VALUE[c["fixed"]]}
    c["h0_fixed"] = 70.0 if seed % 4 < 2 else 67.5
    c["scale"] = {}
    if seed % 3 == 0:  # one slot reads theta x scale
        c["scale"] = {names[(seed // 3) % len(names)]: SCALES[(seed // 3) % len(SCALES)]}
    sc = np.array([c["scale"].get(n, 1.0) for n in names])
    c["bounds"] = bounds = np.array([BOX[n] for n in names], dtype=np.float64) / sc[:, None]

    # quasars: a Hubble diagram with scatter; redshifts on node 1, on the top node, inside the first interval, repeated
    z_hi = float(rng.uniform(2.5, 6.5))
    sn_hi = float(rng.uniform(0.3, 2.3))
    if c["sn_grid_mode"] == "shared_above":
        z_hi = 0.7 * sn_hi
    z = np.sort(rng.uniform(0.02, z_hi, nq))
    top = float(z[-1]) * {"max": 1.0, "below": 0.97, "above": 1.03}[c["z_top_mode"]]
    nodes = np.linspace(0.0, top, G)
    special = [nodes[1], nodes[-1], 0.37 * nodes[1], float(z[nq // 2]), float(z[nq // 2])]
    if c["z_top_mode"] == "max":
        special[1] = nodes[-2]  # max z is the top node already: one on the node below it
    for k, v in enumerate(special[:max(0, nq - 1)]):
        z[k] = v  # the largest redshift (the last) stays
    c["qsr_specials"] = min(len(special), max(0, nq - 1))
    sig = rng.uniform(0.3, 1.5, nq)
    mu = 25 + 5 * np.log10((1 + z) * 4283.0 * z * (1 + 0.4 * z) / (1 + 0.1 * z * z)) + sig * rng.standard_normal(nq)
    c["qsr"] = (z, mu, sig)
    c["z_top"] = top

    c["sn"], c["sn_z_top"] = None, 0.0
    if ns:
        c["sn"] = _sn(rng, ns, sn_hi)
        if c["sn_grid_mode"] == "own":
            c["sn_z_top"] = float(np.max(c["sn"][0]))
    c["bao"] = None
    if nb:
        mode = c["bao_z_mode"]
        if mode == "equal":
            bz = np.full(nb, float(rng.uniform(0.2, 2.4)))
        elif mode == "pairs":  # the DESI pattern: D_M and D_H at the same redshift, a lone D_V first
            zs = np.sort(rng.uniform(0.2, 2.4, nb // 2 + 1))
            bz = np.concatenate([zs[:1], np.repeat(zs[1:], 2)])[:nb]
        else:
            bz = np.sort(rng.uniform(0.1, 2.4, nb))
        if mode != "equal" or seed % 2:
            bz[-1:] = 1.2 * top  # above the quasar grid: a BAO datum has a grid of its own
        qty = np.array([(1 + k) % 3 for k in range(nb)], dtype=np.int32)  # D_M, D_H, D_V in turn
        if mode == "pairs":
            qty = np.array([0] + [1 + k % 2 for k in range(nb - 1)], dtype=np.int32)[:nb]
        M = rng.standard_normal((nb, nb))
        cov = M @ M.T + nb * np.eye(nb)
        dm = 4283.0 * bz * (1 + 0.25 * bz) / (1 + 0.5 * bz)
        dh = 4283.0 / np.sqrt(0.3 * (1 + bz) ** 3 + 0.7)
        val = np.where(qty == 1, dm, np.where(qty == 2, dh, (bz * dh * dm * dm) ** (1 / 3))) / 147.0 + 0.3 * rng.standard_normal(nb)
        c["bao"] = (bz, val, qty, cov)

    theta = rng.uniform(bounds[:, 0], bounds[:, 1], size=(W, len(names)))
    c["row_out"] = c["row_om"] = None
    if W > 2:
        k = names.index("dM_qsr") if "dM_qsr" in names else names.index("s")
        theta[1, k] = bounds[k, 1] + 0.3 * (bounds[k, 1] - bounds[k, 0])  # outside the box, every block still finite
        c["row_out"] = 1
        if "Om" in names:
            theta[2, names.index("Om")] = -0.05 / c["scale"].get("Om", 1.0)  # E^2 < 0 past some z
            c["row_om"] = 2
    c["theta"] = theta
    return c


FIXED_CASES = {
    "one_grid_8192": dict(n_grid=8192, n_qsr=1000, n_sn=64, n_bao=13, W=33, sn_grid_mode="shared"),
    "two_grids_8192": dict(n_grid=8192, n_qsr=2421, n_sn=65, n_bao=1, W=31, sn_grid_mode="own"),
}


def fixed_case(name):
    return build_case(1000 + sorted(FIXED_CASES).index(name), **FIXED_CASES[name])


def filler(case, n, seed):
    """n more rows inside the box (the rest of a large batch)."""
    b = case["bounds"]
    return np.random.default_rng(88000 + seed).uniform(b[:, 0], b[:, 1], size=(n, b.shape[0]))


def nan_rows(case, n, seed):
    """n rows whose SN residuals and quasar terms are NaN: Om far below 0 where it is free, else a NaN coordinate."""
    th = filler(case, n, seed)
    if "Om" in case["names"]:
        th[:, case["names"].index("Om")] = -0.5 / case["scale"].get("Om", 1.0)
    else:
        th[:, 0] = np.nan
    return th


def recipe(case):
    return dict(theta=case["names"], nkp=case["nkp"], bounds=case["bounds"], sn_grid=case["sn_z_top"] > 0, sn_zhel=case["sn_zhel"])


def reference(case, dtype, thetas=None):
    return ref.evaluate(recipe(case), case["theta"] if thetas is None else thetas, case["qsr"], case["sn"], case["bao"],
                        n_grid=case["n_grid"], h0=case["h0_fixed"], z_top=case["z_top"],
                        sn_z_top=case["sn_z_top"] if case["sn"] is not None else None, fixed=case["fixed_values"],
                        scale=case["scale"], dtype=dtype)


def engine_kwargs(case, Param, solve_mode):
    names, fx, sc = case["names"], case["fixed_values"], case["scale"]

    def slot(n, default=None):
        if n in names:
            return Param(names.index(n), scale=sc.get(n, 1.0))
        return Param(fixed=fx[n] if n in fx else default)

    params = {"H0": slot("H0", case["h0_fixed"]), "Om": slot("Om"), "w0": slot("w0")}
    if case["sn"] is not None:
        params["offset"] = slot("offset")
    if case["bao"] is not None:
        params["rd"] = slot("rd")
    z, mu, sig = case["qsr"]
    quasar = dict(z=z, mu=mu, sigma=sig, offset=slot("dM_qsr"), scatter=slot("s"), nkp=case["nkp"], z_top=case["z_top"],
                  sn_z_top=case["sn_z_top"], sn_zhel=case["sn_zhel"])
    sn = None
    if case["sn"] is not None:
        sz, szh, sobs, scov = case["sn"]
        sn = dict(z_cmb=sz, z_hel=szh, obs=sobs, chol=np.linalg.cholesky(scov))
    if case["bao"] is not None:
        bz, bv, bq, bcov = case["bao"]
        quasar["bao"] = dict(z=bz, val=bv, qty=bq, inv_cov=np.linalg.inv(bcov))
    return dict(ndim=len(names), z_max=case["z_top"], n_grid=case["n_grid"], params=params, sn=sn, bounds=case["bounds"],
                prior_normalised=False, solve_mode=solve_mode, quasar=quasar)


def logl_scale(want):
    """The scale of the log L bar: |chi2_total| + |sum ln(sigma^2 + s^2)|, both from the reference."""
    return np.abs(want["chi2"]) + np.abs(want["lnsum"])


def describe(c):
    return (f"seed {c['seed']}: G={c['n_grid']} n_qsr={c['n_qsr']} n_sn={c['n_sn']} n_bao={c['n_bao']} W={c['W']} nkp={c['nkp']} "
            f"z_top={c['z_top_mode']} sn_grid={c['sn_grid_mode']} zhel={c['sn_zhel']} bao_z={c['bao_z_mode']} solve={c['solve']} "
            f"names={c['names']} fixed={c['fixed']} scale={c['scale']}")
