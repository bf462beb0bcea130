"""Cases of the per-walker SN stage sweep (tests/test_walker_shapes_cpu.py, tests/test_gpu_walker_shapes.py,
tests/walker_forms_worker.py): engines with an SN block over the models, grids, SN forms and data edges that walker_kernel,
walker_fast_kernel and walker_stream_kernel (csrc/cosmofit_kernels.hip) accept, with seeded synthetic data and 33 walker rows each.

A case is a plain dict (``CASES[name]``); ``engine_kwargs`` / ``model`` / ``oracle_likelihood`` / ``sn_data`` / ``rows`` turn it into
the LikelihoodEngine's keyword arguments, the long-double reference's Model and SN block (tests/walker_reference.py), the float64
oracle's descriptor (oracle/oracle_np.py), the data and the walkers.  Everything but ``engine`` is plain numpy.

theta columns of every case: offset, H0, Om, obh2, och2, w0, wa, v, s8 (a case maps the slots its model reads; column 7 is the
amplitude of the linear magnitude term in the "lin" form and unread in the "nov" form).

The streaming form's guard and the fragment order of the small-batch solve are restated here in Python (``fast_path``,
``frag_index``): from csrc/cosmofit_device.h (cf_stream_shift_bound against CF_STREAM_GUARD_NODES) and the comment above
delta_index in csrc/cosmofit_kernels.hip."""
import functools
import importlib
import os
import subprocess
import sys
import zlib

import numpy as np

import derived_reference as R
import walker_reference as WR
from oracle import oracle_np as onp

PKG_NAME = "cosmology-model-fit_amd"
LD = np.longdouble
C_KM_S = 299792.458
NDIM, N_ROWS = 9, 33  # 33 walkers = 8 x 4 + 1 = 2 x 16 + 1: ragged for the four-wave streaming workgroup and the 16-walker panel
COLS = ("offset", "H0", "Om", "obh2", "och2", "w0", "wa", "v", "s8")
COL_V = 7
Z_MAX = 2.4
LATE_FLAT, PHYSICAL = R.LATE_FLAT, R.PHYSICAL
LCDM, WCDM, THAWING, CPL = R.LCDM, R.WCDM, R.THAWING, R.CPL
FDE_NAMES = {LCDM: "lcdm", WCDM: "wcdm", THAWING: "thawing", CPL: "cpl"}
SEG, HALO, GUARD_NODES, MAX_SEGS = 512, 64, 64 // 2 - 4, 8  # csrc/cosmofit_device.h

# the strict box of the prior, and the box the ordinary rows are drawn from (E^2 > 0 on every grid, w0 + wa <= 0)
BOUNDS = np.array([(-20.0, -19.0), (50.0, 90.0), (0.05, 0.7), (0.019, 0.026), (0.09, 0.15), (-1.5, -0.4), (-2.0, 1.0), (-3.0, 3.0),
                   (0.5, 1.1)])
BOX = dict(offset=(-19.5, -19.1), H0=(60.0, 80.0), Om=(0.2, 0.45), obh2=(0.020, 0.025), och2=(0.10, 0.14), w0=(-1.2, -0.6),
           wa=(-1.5, 0.6), v=(-2.9, 2.9), s8=(0.7, 0.9))
V_EDGE_MAX = 0.4  # edges cases: ordinary rows keep z_cosmo of the SN at z = 2e-4 above 0 (100 v / c < 2e-4)
Z_SN_MIN = 0.004  # four times the largest in-box |z_pec| = 300 km/s / c
Z_LOW = (2e-4, 5e-4)  # the two SNe of the edges cases below that

# the special rows of every case
ROW_IN, ROW_OUT, ROW_FAR, ROW_ZNEG, ROW_NAN, ROW_OOB, ROW_WA_ZERO = 3, 10, 17, 24, 31, 20, 5
SPECIAL_ROWS = (ROW_IN, ROW_OUT, ROW_FAR, ROW_ZNEG, ROW_NAN, ROW_OOB)
A_CAP, A_FAR_CAP = 0.12, 0.13  # |z_pec| of the guard rows on grids whose guard is wider: every SN above z_turn keeps z_cosmo > 0

GRIDS = (4, 8, 9, 64, 511, 512, 513, 1024, 1025, 3585, 4095, 4096)
GRIDS_GENERIC = (4097, 8192)  # chunk_shift 4: the generic kernel only
N_SN_SET = (1, 63, 64, 65, 129, 513)
SN_FORMS = ("pm1", "weights", "lin", "nov")
EDGE_NODES = (0, 1, 448, 479, 480, 511, 512, 513, -2, -1)  # -2, -1: G - 2, G - 1
EMPTY_SEGMENT = 5  # edges, 4096 nodes: no SN is packed for this segment

# one fresh process per string (CF_TUNE is read once per process): mode -> (CF_TUNE, walker_form, frag order at 33 walkers)
FORMS = {
    "stream": ("walker_stream=1,small_frag=0,sn_parts=1", 1, 0),
    "wg_default": ("walker_stream=0", 0, 1),
    "wg_rows": ("walker_stream=0,small_frag=0,sn_parts=1", 0, 0),
    "generic": ("walker_generic=1", 2, 0),
}
OWN_KEYS = ("walker_stream=", "small_frag=", "sn_parts=", "walker_generic=", "small_max=")
W_BACK_TO_BACK = (176, 100, 5, 33)  # row layout; fragment order with 2 parts; with 4 parts, one partly filled panel; the case rows
W_AUTO = 4096
AUTO_CASES = ("model_physical_thawing", "model_late_wcdm")


def _case(name, group, ez=LATE_FLAT, fde=LCDM, n_sn=130, n_grid=1000, form="pm1", z_max=Z_MAX, edges=False, n_bao=0, growth=False):
    return dict(name=name, group=group, ez_model=ez, fde=fde, n_sn=n_sn, n_grid=n_grid, form=form, z_max=z_max, edges=edges,
                n_bao=n_bao, growth=growth)


def _cases():
    out = []
    for ez in (LATE_FLAT, PHYSICAL):
        for fde in (LCDM, WCDM, THAWING, CPL):
            out.append(_case(f"model_{'physical' if ez else 'late'}_{FDE_NAMES[fde]}", "model", ez, fde))
    for tag, ez, fde in (("thawing", LATE_FLAT, THAWING), ("physwcdm", PHYSICAL, WCDM)):
        for g in GRIDS:
            out.append(_case(f"grid_{tag}_g{g}", "grid", ez, fde, n_sn=70, n_grid=g))
        for g in GRIDS_GENERIC:
            out.append(_case(f"gridgen_{tag}_g{g}", "grid_generic", ez, fde, n_sn=70, n_grid=g))
    for form in SN_FORMS:
        for n in N_SN_SET:
            out.append(_case(f"form_{form}_n{n}", "form", n_sn=n, form=form))
    for g in (1000, 4096):  # the same node spacing on both grids: the SNe next to node 1 stay above z = 2e-3
        out.append(_case(f"edges_g{g}", "edges", n_grid=g, z_max=Z_MAX * (g - 1) / 999, edges=True))
    out.append(_case("aux_physical_cpl", "aux", PHYSICAL, CPL, n_grid=1100, n_bao=8))
    out.append(_case("aux_growth", "growth", growth=True))
    return {c["name"]: c for c in out}


CASES = _cases()
RESIDUAL_CASES = tuple(n for n, c in CASES.items() if c["group"] not in ("aux", "growth"))  # judged row by row
CHI2_CASES = tuple(n for n, c in CASES.items() if c["group"] != "growth")                  # judged against oracle_np


def streamable(name):
    """Does the production (workgroup / streaming) form take this case?  Grids above 4096 nodes keep the generic kernel."""
    return CASES[name]["n_grid"] <= SEG * MAX_SEGS


def expected_form(name, mode):
    """(walker_form, frag order) a 33-walker batch of this case reports under FORMS[mode]."""
    _, form, frag = FORMS[mode]
    return (form, frag) if streamable(name) else (2, 0)


def _pkg():
    return importlib.import_module(PKG_NAME)


def _seed(name):
    return zlib.crc32(name.encode())


def _physical():
    comp = _pkg().cmb_data.PLANCK_ACT
    return {k: comp[k] for k in ("or_h2", "omnu_h2", "o_gamma_h2", "nu_m0", "nu_rho0", "nu_qs_sq", "nu_ws")}


def _slots(case):
    """slot name -> theta column of the slots this case reads."""
    s = dict(offset=0, H0=1)
    s.update(dict(obh2=3, och2=4) if case["ez_model"] == PHYSICAL else dict(Om=2))
    if case["fde"] != LCDM:
        s.update(w0=5)
    if case["fde"] == CPL:
        s.update(wa=6)
    if case["form"] in ("pm1", "weights"):
        s.update(v=COL_V)
    elif case["form"] == "lin":
        s.update(lin=COL_V)
    if case["growth"]:
        s.update(s8=8)
    return s


@functools.lru_cache(maxsize=None)
def model(name) -> R.Model:
    case = CASES[name]
    params = {k: (i, 1.0) for k, i in _slots(case).items()}
    if case["n_bao"]:
        params["rd"] = ("fixed", 147.0)
    return R.Model(ndim=NDIM, params=params, z_max=case["z_max"], ez_model=case["ez_model"], fde=case["fde"], n_grid=case["n_grid"],
                   comp=_physical() if case["ez_model"] == PHYSICAL else None)


def grid_of(name):
    case = CASES[name]
    return np.linspace(0, case["z_max"], num=case["n_grid"])


# ---- the SN block ---------------------------------------------------------------------------------------------------------------
def _edge_redshifts(case, rng):
    """Within 1 ulp and within 1e-3 of a node spacing on either side of the EDGE_NODES (node 0: the two SNe at z = 2e-4 and 5e-4,
    inside its interval), z_max itself and 2 % above it, the two ordinary low SNe, and a bulk that leaves segment EMPTY_SEGMENT of
    the 4096-node grid without an SN."""
    zg, G = np.linspace(0, case["z_max"], num=case["n_grid"]), case["n_grid"]
    step = zg[1]
    z = list(Z_LOW) + [Z_SN_MIN, 0.012, case["z_max"], 1.02 * case["z_max"]]
    for n in EDGE_NODES[1:]:
        zn = zg[n]
        z += [np.nextafter(zn, -np.inf), np.nextafter(zn, np.inf), zn - 1e-3 * step, zn + 1e-3 * step]
    bulk = np.exp(rng.uniform(np.log(0.08), np.log(0.96 * case["z_max"]), 4 * case["n_sn"]))
    if G > SEG * (EMPTY_SEGMENT + 1):  # packed by (node + HALO / 2) / SEG: keep two nodes clear of the segment's range
        lo, hi = zg[SEG * EMPTY_SEGMENT - HALO // 2 - 2], zg[SEG * (EMPTY_SEGMENT + 1) - HALO // 2 + 2]
        bulk = bulk[(bulk < lo) | (bulk > hi)]
    return np.array(z + list(bulk[: case["n_sn"] - len(z)]))


@functools.lru_cache(maxsize=None)
def sn_data(name) -> dict:
    """z_cmb (unsorted), z_hel, obs, chol, step (+-1, general weights or None), lin_coef (or None), max_step, zp1_max."""
    case = CASES[name]
    rng = np.random.default_rng(_seed(name))
    n = case["n_sn"]
    if case["edges"]:
        z = _edge_redshifts(case, rng)
    else:
        z = np.concatenate([[Z_SN_MIN, 0.012], np.exp(rng.uniform(np.log(0.08), np.log(2.3), max(n - 2, 0)))])[:n]
    assert z.size == n
    lowest = np.argsort(z)[:2]
    weights = rng.uniform(-0.95, 0.95, n)
    weights[lowest[0]] = 0.95   # the lowest SN carries the largest weight: ROW_ZNEG is sized by it
    if n > 1:
        weights[lowest[1]] = 0.9
    p = rng.permutation(n)
    z, weights = z[p], weights[p]
    z_hel = z * (1 + 1e-3 * rng.standard_normal(n))
    obs = 25 + 5 * np.log10((1 + z_hel) * 4283.0 * z * (1 + 0.4 * z)) - 19.3 + 0.15 * rng.standard_normal(n)
    if n == 1:  # chi^2 is one squared residual: keep it a magnitude from 0, or its relative error is the residual's, amplified
        obs = obs + 1.0
    A = 0.02 * rng.standard_normal((n, 12))
    chol = np.linalg.cholesky(np.diag(rng.uniform(0.1, 0.3, n) ** 2) + A @ A.T)
    form = case["form"]
    step = np.where(z <= 0.15, 1.0, -1.0) if form == "pm1" else (weights if form == "weights" else None)  # sn/pantheon.py:46
    lin_coef = 0.1 * rng.standard_normal(n) if form == "lin" else None
    out = dict(z_cmb=z, z_hel=z_hel, obs=obs, chol=chol, step=step, lin_coef=lin_coef,
               max_step=0.0 if step is None else float(np.max(np.abs(step))), zp1_max=max(1.0, 1.0 + float(np.max(z))))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the streaming form's guard, restated ---------------------------------------------------------------------------------------
def shift_bound(name, v):
    """(a, shift in nodes) of cf_stream_shift_bound for the velocity column v [100 km/s], in float64 as the kernel forms them."""
    case, sn = CASES[name], sn_data(name)
    inv_step = (case["n_grid"] - 1) / case["z_max"]
    v100 = 100.0 * np.asarray(v, dtype=np.float64) if case["form"] in ("pm1", "weights") else np.zeros(np.shape(v))
    a = np.abs(v100) * sn["max_step"] / C_KM_S
    with np.errstate(all="ignore"):
        return a, sn["zp1_max"] * (a / (1.0 - a)) * inv_step


def fast_path(name, theta=None):
    """[rows] bool: the walker passes the streaming kernel's guard (its SNe are evaluated from the windows they were packed for);
    False: the slow path, every SN looked at in every segment.  NaN fails the guard."""
    a, shift = shift_bound(name, (rows(name) if theta is None else theta)[:, COL_V])
    return (a < 0.5) & (shift <= float(GUARD_NODES))


def a_star(name):
    """|z_pec| at which the shift bound equals the guard: K a / (1 - a) = GUARD_NODES, K = (1 + max z_cmb) (G - 1) / z_max."""
    case, sn = CASES[name], sn_data(name)
    K = sn["zp1_max"] * (case["n_grid"] - 1) / case["z_max"]
    return GUARD_NODES / (K + GUARD_NODES)


@functools.lru_cache(maxsize=None)
def rows(name) -> np.ndarray:
    """[33, 9] float64.  Ordinary rows inside BOX (CPL: w0 + wa <= 0, ROW_WA_ZERO with wa = 0 exactly); ROW_IN / ROW_OUT just inside
    / outside the streaming guard and ROW_FAR three times beyond it (negative v: the SNe below z_turn move up, those above it down,
    none below 0; capped at A_CAP / A_FAR_CAP on grids whose guard is wider than that); ROW_ZNEG puts z_cosmo of the lowest SN
    below 0; ROW_NAN has NaN in column 7; ROW_OOB has H0 = 95, outside the box."""
    case, sn = CASES[name], sn_data(name)
    rng = np.random.default_rng(_seed(name) + 1)
    th = np.stack([rng.uniform(*BOX[c], N_ROWS) for c in COLS], axis=1)
    th[:, 6] = np.minimum(th[:, 6], -th[:, 5])  # w0 + wa <= 0
    th[ROW_WA_ZERO, 6] = 0.0
    th[ROW_WA_ZERO + 1, 6], th[ROW_WA_ZERO + 2, 6] = 0.4, -0.9
    if case["edges"]:
        th[:, COL_V] = rng.uniform(-2.9, V_EDGE_MAX, N_ROWS)
    max_step = sn["max_step"] if sn["max_step"] > 0 else 1.0
    a_g = a_star(name)
    to_v = C_KM_S / max_step / 100.0  # |z_pec| of the largest weight -> the sampler's units of 100 km/s
    a_edge = min(a_g, A_CAP)
    th[ROW_IN, COL_V] = -a_edge * (1 - 1e-9) * to_v
    th[ROW_OUT, COL_V] = -a_edge * (1 + 1e-9) * to_v
    th[ROW_FAR, COL_V] = -min(3 * a_g, A_FAR_CAP) * to_v
    i_low = int(np.argmin(sn["z_cmb"]))
    z_low = float(sn["z_cmb"][i_low])
    w_low = 1.0 if sn["step"] is None else float(sn["step"][i_low])
    th[ROW_ZNEG, COL_V] = ((1.0 + 2.0 * z_low) * z_low * C_KM_S / 100.0 / abs(w_low) + 0.2) * np.sign(w_low)  # z_pec > z_low
    th[ROW_NAN, COL_V] = np.nan
    th[ROW_OOB, 1] = 95.0
    th.setflags(write=False)
    return th


# ---- the other blocks of the two joint cases --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bao_data(name):
    """Eight BAO data whose six-node stencils (two nodes below the datum's interval, cf. aux_node_base of csrc/cosmofit_api.hip)
    start at node 0, straddle nodes 512 and 1024 and end at G - 1; the rest anywhere."""
    case = CASES[name]
    if not case["n_bao"]:
        return None
    rng = np.random.default_rng(_seed(name) + 2)
    zg = grid_of(name)
    step, G = zg[1], case["n_grid"]
    z = np.array([0.3 * step, 510.5 * step, 1022.5 * step, zg[G - 1] - 0.4 * step] + list(rng.uniform(0.1, 2.0, case["n_bao"] - 4)))
    qty = (np.arange(z.size) + 1) % 4
    lk = onp.Likelihood(ndim=NDIM, z_max=case["z_max"], n_grid=G, ez_model=case["ez_model"], fde=case["fde"], bao_z=z, bao_qty=qty,
                        **_oracle_slots(case), **{k: (np.asarray(v) if np.ndim(v) else v) for k, v in _physical().items()})
    fid = np.array([0.5 * (lo + hi) for lo, hi in (BOX[c] for c in COLS)])
    val = onp.bao_theory(lk, fid) * (1 + 0.01 * rng.standard_normal(z.size))
    u = rng.standard_normal(z.size)
    s = 1.0 / (0.02 * np.abs(val))
    inv_cov = np.outer(s, s) * (np.eye(z.size) + 0.3 * np.outer(u, u) / (u @ u))
    return dict(z=z, val=val, qty=qty.astype(np.int32), inv_cov=(inv_cov + inv_cov.T) / 2)


def bao_stencils(name):
    """[n_bao, 2]: first and last table node of each datum's stencil (restated from aux_node_base: interval i with
    z_i < z <= z_{i+1}, two nodes below, clamped into the grid)."""
    zg, G = grid_of(name), CASES[name]["n_grid"]
    i = np.clip(np.searchsorted(zg, bao_data(name)["z"], side="left") - 1, 0, G - 2)
    b = np.clip(i - 2, 0, G - 6)
    return np.stack([b, b + 5], axis=1)


def _fs8_data(name):
    rng = np.random.default_rng(_seed(name) + 3)
    z = np.array([0.07, 0.3, 0.6, 0.85, 1.4])
    hd = 70.0 * np.sqrt(0.3 * (1 + z) ** 3 + 0.7) * 4283.0 * z * (1 + 0.4 * z) / (1 + z)
    return dict(z=z, val=0.45 * (1 + 0.1 * rng.standard_normal(z.size)), inv_cov=np.eye(z.size) / 0.05**2, fid=hd, a_init=1e-3)


# ---- engine, oracle, reference ------------------------------------------------------------------------------------------------------
def engine_kwargs(pkg, name) -> dict:
    case, sn = CASES[name], sn_data(name)
    P = pkg.Param
    params = {k: P(i) for k, i in _slots(case).items()}
    block = dict(z_cmb=sn["z_cmb"], z_hel=sn["z_hel"], obs=sn["obs"], chol=sn["chol"], z_turn=0.15)
    if case["form"] == "weights":
        block["step"] = sn["step"]
    if case["form"] == "lin":
        block["lin_coef"] = sn["lin_coef"]
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    kw = dict(ndim=NDIM, z_max=case["z_max"], n_grid=case["n_grid"], ez_model=case["ez_model"], fde=case["fde"], params=params,
              sn=block, bounds=BOUNDS, solve_mode=eng_mod.solve_mode_of("inverse"))
    if case["ez_model"] == PHYSICAL:
        kw["physical"] = _physical()
    if case["n_bao"]:
        params["rd"] = P(fixed=147.0)
        kw["bao"] = dict(bao_data(name))
    if case["growth"]:
        kw["fs8"] = _fs8_data(name)
    return kw


def engine(pkg, name):
    return pkg.LikelihoodEngine(**engine_kwargs(pkg, name))


def _oracle_slots(case):
    s = {k: onp.Slot(i) for k, i in _slots(case).items()}
    if case["n_bao"]:
        s["rd"] = onp.Slot(fixed=147.0)
    return s


@functools.lru_cache(maxsize=None)
def oracle_likelihood(name) -> onp.Likelihood:
    """The float64 oracle's descriptor of the same case (not for the growth case: the growth sweep holds that block's reference)."""
    case, sn = CASES[name], sn_data(name)
    assert not case["growth"]
    kw = dict(ndim=NDIM, z_max=case["z_max"], n_grid=case["n_grid"], ez_model=case["ez_model"], fde=case["fde"], bounds=BOUNDS,
              z_cmb=sn["z_cmb"], z_hel=sn["z_hel"], obs=sn["obs"], chol=sn["chol"], z_turn=0.15, step=sn["step"],
              has_vstep=case["form"] in ("pm1", "weights"), lin_coef=sn["lin_coef"], **_oracle_slots(case))
    if case["ez_model"] == PHYSICAL:
        kw.update({k: (np.asarray(v) if np.ndim(v) else v) for k, v in _physical().items()})
    if case["n_bao"]:
        b = bao_data(name)
        kw.update(bao_z=b["z"], bao_val=b["val"], bao_qty=b["qty"], bao_inv_cov=b["inv_cov"])
    return onp.Likelihood(**kw)


@functools.lru_cache(maxsize=None)
def reference(name) -> dict:
    """walker_reference.residuals of the case's 33 rows plus tol = 1e-12 + 4 env (computed once per process; read-only)."""
    ref = WR.residuals(model(name), sn_data(name), rows(name), bounds=BOUNDS)
    ref["tol"] = LD(1e-12) + 4 * ref["env"]
    # compared by finite / non-finite alone: z_cosmo <= 0, and the NaN row where the block reads the NaN (not in the "nov" form)
    ref["class_only"] = ref["nonpos"] | ~np.isfinite(ref["delta"].astype(np.float64))
    return ref


@functools.lru_cache(maxsize=None)
def oracle_values(name) -> dict:
    """chi_squared and log_probability of oracle_np for the 33 rows, and its residual rows [33, n_sn] (float64).  A row with a NaN
    parameter is NaN in chi^2 and residuals without a call (the oracle's interval search has no index for a NaN abscissa); its
    log_probability is the oracle's own: outside the box, -inf."""
    lk, th = oracle_likelihood(name), rows(name)
    ok = np.all(np.isfinite(th[:, sorted(_slots(CASES[name]).values())]), axis=1)  # (the "nov" form does not read column 7)
    with np.errstate(all="ignore"):
        chi2 = np.array([onp.chi_squared(lk, r) if k else np.nan for r, k in zip(th, ok)])
        logp = np.array([onp.log_probability(lk, r) for r in th])
        delta = np.stack([onp.sn_parts(lk, r)[3] if k else np.full(lk.z_cmb.size, np.nan) for r, k in zip(th, ok)])
    return dict(chi2=chi2, logp=logp, delta=delta)


# ---- the residual buffer ----------------------------------------------------------------------------------------------------------
def n_ld_of(n_sn):
    return (n_sn + 63) // 64 * 64


def frag_index(w, i, n_ld):
    """Flat index of element (walker w, row i) in the fragment order: panel w / 16 of 16 n_ld doubles, K-step pair i / 8 of 128,
    lane group i / 2 % 4 of 32, column w % 16, then the row's parity."""
    return (w >> 4) * 16 * n_ld + (i >> 3) * 128 + ((i >> 1) & 3) * 32 + 2 * (w & 15) + (i & 1)


def rows_of_buffer(buf, layout, W, n_sn):
    """[W, n_ld] walker rows of the raw residual buffer of LikelihoodEngine.last_residuals (layout 0: as stored; 1: un-permuted)."""
    n_ld = n_ld_of(n_sn)
    flat = np.ascontiguousarray(buf).reshape(-1)
    assert flat.size == (W + 15) // 16 * 16 * n_ld and layout in (0, 1)
    if layout == 0:
        return flat.reshape(-1, n_ld)[:W].copy()
    w, i = np.meshgrid(np.arange(W), np.arange(n_ld), indexing="ij")
    return flat[frag_index(w, i, n_ld)]


def scatter(W):
    """Where the 33 case rows go in a W-walker batch: at its start, across streaming-workgroup (4) and panel (16, 32) boundaries in
    the middle, and at its end."""
    return np.concatenate([np.arange(11), W // 2 - 5 + np.arange(11), W - 11 + np.arange(11)])


B2B_CASE = "model_late_lcdm"
B2B_FIVE = (0, 5, 11, 22, 32)  # ordinary in-box rows: the five of the 5-walker batch, present in every batch of the sequence


def b2b_rows(W):
    """Which of the 33 case rows a batch of the back-to-back sequence holds, walker by walker."""
    return np.array(B2B_FIVE) if W == len(B2B_FIVE) else np.arange(W) % N_ROWS


def run_workers(jobs, out_dir, timeout=600):
    """tests/walker_forms_worker.py once per (mode, CF_TUNE string), side by side (at most five processes) ->
    {mode: dict of its arrays}.  The worker's own keys are stripped from an inherited CF_TUNE.  A worker that does not exit with
    status 0 fails the caller with its output; nothing is retried."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "walker_forms_worker.py")
    inherited = [kv for kv in os.environ.get("CF_TUNE", "").split(",") if kv and not kv.startswith(OWN_KEYS)]
    procs, results = [], {}
    for mode, tune in jobs:
        out = os.path.join(str(out_dir), f"walker_{mode}.npz")
        env = dict(os.environ, CF_TUNE=",".join(inherited + ([tune] if tune else [])))
        p = subprocess.Popen([sys.executable, worker, out, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        procs.append((mode, tune, out, p))
    try:
        for mode, tune, out, p in procs:
            log, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, f"worker {mode!r} under CF_TUNE={tune!r} failed ({p.returncode}):\n{log}"
            results[mode] = dict(np.load(out))
            results[mode]["log"] = log
    finally:
        for *_, p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    return results
