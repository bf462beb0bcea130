"""Cases of the small-blocks sweep (tests/test_blocks_cpu.py, tests/test_gpu_blocks_shapes.py, tests/blocks_forms_worker.py):
engines without an SN block over the launch forms, block sizes, models and options small_blocks_kernel accepts
(csrc/cosmofit_kernels.hip), with seeded synthetic data and 33 walker rows each.

A case is a plain dict (``CASES[name]``); ``engine_kwargs`` / ``model`` / ``oracle_likelihood`` / ``data`` / ``rows`` turn it into
the LikelihoodEngine's keyword arguments, the long-double reference's Model (tests/blocks_reference.py), the float64 oracle's
descriptor (oracle/oracle_np.py), the block data and the walkers.  Everything but ``engine`` is plain numpy.

theta columns of every case: H0, Om, obh2, och2, w0, wa, rd, fcc (a case maps the slots its model reads)."""
import functools
import importlib
import os
import subprocess
import sys

import numpy as np

import blocks_reference as B
import derived_reference as R
from oracle import oracle_np as onp

PKG_NAME = "cosmology-model-fit_amd"
LD = np.longdouble
NDIM, N_ROWS = 8, 33  # 33 walkers: ragged for every form (2 x 16 + 1, 8 x 4 + 1, 16 x 2 + 1 walkers per workgroup)
COLS = ("H0", "Om", "obh2", "och2", "w0", "wa", "rd", "fcc")
Z_MAX = 2.5
ROW_WA_ZERO = 5          # CPL: wa = 0 exactly (the exponent's second term is -0.0 there)
ROW_NAN, ROW_BAD = 16, 17  # test of the neighbours of a bad row
LATE_FLAT, PHYSICAL = R.LATE_FLAT, R.PHYSICAL
LCDM, WCDM, THAWING, CPL = R.LCDM, R.WCDM, R.THAWING, R.CPL
FDE_NAMES = {LCDM: "lcdm", WCDM: "wcdm", THAWING: "thawing", CPL: "cpl"}

# the box the rows are drawn from: E^2 > 0 everywhere, (1 + w0) + (1 - w0)(1 + z)^3 > 0, w0 + wa <= 0, positive bases of every power
BOX = dict(H0=(60.0, 80.0), Om=(0.2, 0.45), obh2=(0.020, 0.025), och2=(0.10, 0.14), w0=(-1.2, -0.6), wa=(-1.5, 0.6), rd=(130.0, 160.0),
           fcc=(0.8, 1.25))

# forced launch forms: (lanes, waves per walker) -> CF_TUNE string (one fresh process each: the string is read once per process)
FORMS = {(16, 1): "sb_wide_max=0", (64, 1): "sb_wide_max=1000000,sb_roles_max=0", (64, 2): "sb_wide_max=1000000,sb_roles_max=1000000"}
FORM_CODE = {(16, 1): 272, (64, 1): 320, (64, 2): 576}
W_SHAPES = (1, 2, 3, 5, 15, 16, 17)  # batch-shape test: the first W rows alone
W_LARGE = 2049                       # one walker past the default switch to sixteen lanes

SIZE_SWEEP = ((1, 1, 1), (8, 15, 2), (9, 16, 16), (16, 17, 17), (17, 32, 63), (33, 48, 64), (49, 64, 65), (64, 1, 128), (1, 64, 255),
              (64, 64, 256))  # (n_bao, n_cc, n_gl)
N_BAO_SET = {1, 8, 9, 16, 17, 33, 49, 64}
N_CC_SET = {1, 15, 16, 17, 32, 48, 64}
N_GL_SET = {1, 2, 16, 17, 63, 64, 65, 128, 255, 256}


def _case(name, ez, fde, n_bao=0, n_cc=0, n_gl=0, cmb_mode=0, rd="slot", dh_exact=False, f_inverse=False, n_grid=1000, edges=False,
          group="options"):
    return dict(name=name, ez_model=ez, fde=fde, n_bao=n_bao, n_cc=n_cc, n_gl=n_gl if cmb_mode else 0, cmb_mode=cmb_mode, rd=rd,
                dh_exact=dh_exact, f_inverse=f_inverse, n_grid=n_grid, edges=edges, group=group)


def _cases():
    out = []
    for nb, nc, ng in SIZE_SWEEP:  # PHYSICAL + CPL, BAO + CC + CMB mode 1
        out.append(_case(f"size_b{nb}_c{nc}_g{ng}", PHYSICAL, CPL, nb, nc, ng, cmb_mode=1, rd="fit", group="size"))
    for ez in (LATE_FLAT, PHYSICAL):  # every (ez_model, fde) pair; cf_create rejects a CMB block on LATE_FLAT
        for fde in (LCDM, WCDM, THAWING, CPL):
            phys = ez == PHYSICAL
            out.append(_case(f"model_{'physical' if phys else 'late'}_{FDE_NAMES[fde]}", ez, fde, 17, 33, 65, cmb_mode=1 if phys else 0,
                             rd="fit" if phys else "slot", group="model"))
    out += [
        _case("opt_cmb_mode2", PHYSICAL, THAWING, 17, 33, 65, cmb_mode=2, rd="fit"),
        _case("opt_cmb_mode3", PHYSICAL, WCDM, 17, 33, 65, cmb_mode=3, rd="fit"),
        _case("opt_rd_slot_physical", PHYSICAL, LCDM, 17, 33, 65, cmb_mode=1, rd="slot"),
        _case("opt_rd_fit_late", LATE_FLAT, WCDM, 17, 33, rd="fit_late"),
        _case("opt_dh_exact", PHYSICAL, CPL, 17, 33, 65, cmb_mode=1, rd="fit", dh_exact=True),
        _case("opt_dh_exact_late", LATE_FLAT, THAWING, 17, 33, dh_exact=True),
        _case("opt_f_inverse", LATE_FLAT, THAWING, 17, 33, f_inverse=True),
        _case("opt_bao_only", LATE_FLAT, LCDM, 17),
        _case("opt_cc_only", LATE_FLAT, CPL, 0, 33),
        _case("opt_cmb_only", PHYSICAL, WCDM, 0, 0, 65, cmb_mode=1),
    ]
    for g in (6, 64, 4000):  # BAO data at the ends of the grid and at a node
        out.append(_case(f"edge_grid{g}", PHYSICAL, CPL, 8, 9, 16, cmb_mode=1, rd="fit", n_grid=g, edges=True, group="edges"))
    return {c["name"]: c for c in out}


CASES = _cases()
LARGEST_SIZE_CASE = "size_b64_c64_g256"
SWITCH_CASES = (LARGEST_SIZE_CASE, "model_late_cpl")  # automatic switch 64 x 2 -> 16 x 1
EDGE_CASES = tuple(n for n, c in CASES.items() if c["group"] == "edges")


def _pkg():
    return importlib.import_module(PKG_NAME)


def comp_of(case):
    """The compression whose constants fill the radiation / neutrino fields (and the CMB prior): EARLY_LCDM for mode 3."""
    cd = _pkg().cmb_data
    return cd.EARLY_LCDM if case["cmb_mode"] == 3 else cd.PLANCK_ACT


def _slots(case):
    """slot name -> theta column of the slots this case's model reads."""
    s = dict(H0=0, fcc=7)
    if case["ez_model"] == PHYSICAL:
        s.update(obh2=2, och2=3)
    else:
        s.update(Om=1)
        if case["rd"] == "fit_late":
            s.update(obh2=2)
    if case["fde"] != LCDM:
        s.update(w0=4)
    if case["fde"] == CPL:
        s.update(wa=5)
    if case["rd"] == "slot":
        s.update(rd=6)
    return s


def rd_fit_of(case):
    if case["rd"] == "slot":
        return None
    cd = _pkg().cmb_data
    return (1.0, 1.0) + cd.RDRAG_A if case["rd"] == "fit_late" else tuple(comp_of(case)["rd_fit"])  # bao/desi_union3_bbn.py: b = m = 1


def _physical(case):
    comp = comp_of(case)
    return {k: comp[k] for k in ("or_h2", "omnu_h2", "o_gamma_h2", "nu_m0", "nu_rho0", "nu_qs_sq", "nu_ws")}


@functools.lru_cache(maxsize=None)
def model(name) -> R.Model:
    case = CASES[name]
    comp = None
    if case["ez_model"] == PHYSICAL:
        comp = dict(_physical(case), zstar_fit=comp_of(case)["zstar_fit"])
    return R.Model(ndim=NDIM, params={k: (i, 1.0) for k, i in _slots(case).items()}, z_max=Z_MAX, ez_model=case["ez_model"],
                   fde=case["fde"], n_grid=case["n_grid"], rd_fit=rd_fit_of(case), rd_wm_late=case["rd"] == "fit_late",
                   dh_exact=case["dh_exact"], comp=comp, zstar_consts=_pkg().cmb_data.ZSTAR_CONSTS, n_gl=max(case["n_gl"], 1))


def fiducial():
    return np.array([[0.5 * (lo + hi) for lo, hi in (BOX[c] for c in COLS)]])


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2**32)


@functools.lru_cache(maxsize=None)
def rows(name) -> np.ndarray:
    """[33, 8] float64 inside BOX; CPL cases hold wa > 0, wa < 0 and ROW_WA_ZERO with wa = 0 exactly."""
    rng = np.random.default_rng(_seed(name) + 1)
    th = np.stack([rng.uniform(*BOX[c], N_ROWS) for c in COLS], axis=1)
    th[:, 5] = np.minimum(th[:, 5], -th[:, 4])  # w0 + wa <= 0
    th[ROW_WA_ZERO, 5] = 0.0
    th[ROW_WA_ZERO + 1, 5], th[ROW_WA_ZERO + 2, 5] = 0.4, -0.9
    th.setflags(write=False)
    return th


def bad_rows(name) -> np.ndarray:
    """rows() with NaN in H0 of ROW_NAN and, in ROW_BAD, values outside every positive-base assumption (negative densities and
    Hubble constant, E^2 < 0, a phantom w0 far outside the box)."""
    th = rows(name).copy()
    th[ROW_NAN, 0] = np.nan
    th[ROW_BAD] = [-70.0, -0.3, -0.02, -0.5, 5.0, 7.0, -150.0, -1.0]
    return th


def inv_spd(C):
    """Inverse of a symmetric positive-definite float64 matrix by Cholesky in long double, rounded to float64 and symmetrised."""
    n = C.shape[0]
    A = np.asarray(C, dtype=np.float64).astype(LD)
    Lc = np.zeros((n, n), dtype=LD)
    for j in range(n):
        Lc[j, j] = np.sqrt(A[j, j] - Lc[j, :j] @ Lc[j, :j])
        if j + 1 < n:
            Lc[j + 1:, j] = (A[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
    Li = np.zeros((n, n), dtype=LD)
    for j in range(n):  # L Li = I, column by column
        Li[j, j] = 1 / Lc[j, j]
        for i in range(j + 1, n):
            Li[i, j] = -(Lc[i, j:i] @ Li[j:i, j]) / Lc[i, i]
    K = (Li.T @ Li).astype(np.float64)
    return (K + K.T) / 2


def _cov(rng, val):
    """Correlated SPD covariance: sigma_i = (1..3) % of |val_i|, correlation 0.6 I + 0.4 x (a rank-3 correlation matrix)."""
    n = val.size
    sig = np.abs(val) * rng.uniform(0.01, 0.03, n)
    Bm = rng.standard_normal((n, 3))
    G = Bm @ Bm.T
    s = np.sqrt(np.diag(G))
    corr = 0.6 * np.eye(n) + 0.4 * G / np.outer(s, s)
    return corr * np.outer(sig, sig)


def _bao_z(case, rng):
    n, g = case["n_bao"], case["n_grid"]
    if not case["edges"]:
        return np.sort(rng.uniform(0.05, Z_MAX - 0.1, n))
    zg = np.linspace(0, Z_MAX, num=g)
    node = zg[g // 2]
    z = [0.3 * zg[1], node - 5e-10, node + 5e-10, Z_MAX - 0.4 * (zg[-1] - zg[-2]), Z_MAX, 1.05 * Z_MAX]  # first interval ... above z_max
    z += list(rng.uniform(0.05, Z_MAX - 0.1, n - len(z)))
    return np.array(z)


@functools.lru_cache(maxsize=None)
def data(name) -> dict:
    """dict(bao=..., cc=..., cmb=...) (absent blocks None): val / h = the reference's theory at the fiducial theta x (1 + 0.01 normal)."""
    case, m = CASES[name], model(name)
    rng = np.random.default_rng(_seed(name))
    fid = fiducial()
    out = dict(bao=None, cc=None, cmb=None)
    if case["n_bao"]:
        z = _bao_z(case, rng)
        qty = (np.arange(z.size) + int(rng.integers(4))) % 4  # codes 0-3 mixed within the engine
        val = (B.bao_theory(m, fid, z, qty)[0] * (1 + 0.01 * rng.standard_normal(z.size))).astype(np.float64)
        out["bao"] = dict(z=z, val=val, qty=qty.astype(np.int32), inv_cov=inv_spd(_cov(rng, val)))
    if case["n_cc"]:
        z = np.sort(rng.uniform(0.05, 2.0, case["n_cc"]))
        th, c = R._cosmo(m, fid)
        h = (R.H_of_z(m, R._col(c), z.astype(LD))[0] * (1 + 0.01 * rng.standard_normal(z.size))).astype(np.float64)
        cov = _cov(rng, h)
        out["cc"] = dict(z=z, h=h, inv_cov=inv_spd(cov), f_inverse=case["f_inverse"], logdet=float(np.linalg.slogdet(cov)[1]))
    if case["cmb_mode"]:
        comp = comp_of(case)
        out["cmb"] = dict(mode=case["cmb_mode"], prior=np.asarray(comp["cmb_prior"], dtype=np.float64),
                          inv_cov=np.asarray(comp["cmb_inv_cov"], dtype=np.float64), zstar_fit=tuple(comp["zstar_fit"]), n_gl=case["n_gl"])
    return out


def engine_kwargs(pkg, name) -> dict:
    case, d = CASES[name], data(name)
    P = pkg.Param
    kw = dict(ndim=NDIM, z_max=Z_MAX, n_grid=case["n_grid"], ez_model=case["ez_model"], fde=case["fde"],
              params={k: P(i) for k, i in _slots(case).items()})
    if case["ez_model"] == PHYSICAL:
        kw["physical"] = _physical(case)
    if d["bao"] is not None:
        kw["bao"] = dict(d["bao"], dh_exact=case["dh_exact"], rd_fit=rd_fit_of(case), rd_wm_late=case["rd"] == "fit_late")
    if d["cc"] is not None:
        kw["cc"] = dict(d["cc"])
    if d["cmb"] is not None:
        kw["cmb"] = dict(d["cmb"])
    return kw


def engine(pkg, name):
    return pkg.LikelihoodEngine(**engine_kwargs(pkg, name))


def oracle_likelihood(name) -> onp.Likelihood:
    """The float64 oracle's descriptor of the same case."""
    case, d = CASES[name], data(name)
    kw = dict(ndim=NDIM, z_max=Z_MAX, n_grid=case["n_grid"], ez_model=case["ez_model"], fde=case["fde"],
              **{k: onp.Slot(i) for k, i in _slots(case).items()})
    if case["ez_model"] == PHYSICAL:
        kw.update({k: (np.asarray(v) if np.ndim(v) else v) for k, v in _physical(case).items()})
    if d["bao"] is not None:
        b = d["bao"]
        kw.update(bao_z=b["z"], bao_val=b["val"], bao_qty=b["qty"], bao_inv_cov=b["inv_cov"], bao_dh_exact=case["dh_exact"],
                  rd_fit=rd_fit_of(case), rd_wm_late=case["rd"] == "fit_late")
    if d["cc"] is not None:
        c = d["cc"]
        kw.update(cc_z=c["z"], cc_h=c["h"], cc_inv_cov=c["inv_cov"], cc_f_inverse=case["f_inverse"])
    if d["cmb"] is not None:
        c = d["cmb"]
        gx, gw = np.polynomial.legendre.leggauss(case["n_gl"])
        kw.update(cmb_mode=c["mode"], cmb_prior=c["prior"], cmb_inv_cov=c["inv_cov"], zstar_fit=c["zstar_fit"], gl_x=gx, gl_w=gw)
    return onp.Likelihood(**kw)


@functools.lru_cache(maxsize=None)
def reference(name) -> dict:
    """blocks_reference.reference of the case's 33 rows (computed once per process; treat as read-only)."""
    return B.reference(model(name), data(name), rows(name))


# ---- what the kernel delivers, in one flat dict of float64 arrays (the workers save exactly this) -----------------------------------
OUTPUTS = ("chi2", "chi2_bao", "chi2_cmb", "chi2_cc", "cmb_vector", "z_star", "r_drag", "bao_theory")


def evaluate(eng, theta) -> dict:
    """Every output of parts() and chi_squared for a batch, through the production launch path (no SN block: the lean per-walker
    kernel, then small_blocks_kernel in the form cf_small_blocks_form reports for this batch size)."""
    theta = np.ascontiguousarray(theta)
    p = eng.parts(theta)
    out = dict(chi2=np.array(eng.chi_squared(theta)), chi2_bao=p["chi2_blocks"][:, 1].copy(), chi2_cmb=p["chi2_blocks"][:, 2].copy(),
               chi2_cc=p["chi2_cc"].copy(), cmb_vector=p["cmb_vector"].copy(), z_star=p["z_star"].copy(), r_drag=p["r_drag"].copy())
    if p["bao_theory"] is not None:
        out["bao_theory"] = p["bao_theory"].copy()
    return out


def judged(name):
    """(output name, reference key, scale key or None) of the outputs this case's reference judges."""
    case = CASES[name]
    out = []
    if case["n_bao"]:
        out += [("bao_theory", "bao_theory", None), ("chi2_bao", "chi2_bao", "scale_bao"), ("r_drag", "r_drag", None)]
    if case["cmb_mode"]:
        out += [("cmb_vector", "cmb_vector", None), ("chi2_cmb", "chi2_cmb", "scale_cmb"), ("z_star", "z_star", None)]
    if case["n_cc"]:
        out += [("chi2_cc", "chi2_cc", "scale_cc")]
    return out


def ratios(name, got, ref=None, sel=None, bar=1e-10) -> dict:
    """{output: worst |got - ref| / (bar x scale)} over the rows `sel` (default all): scale = |ref| for the theory outputs, the
    chi^2's own scale (blocks_reference) for a chi^2.  A value below 1 meets the bar."""
    ref = reference(name) if ref is None else ref
    sel = slice(None) if sel is None else sel
    out = {}
    for key, rkey, skey in judged(name):
        r = ref[rkey][sel]
        scale = np.abs(r) if skey is None else ref[skey][sel]
        err = np.abs(np.asarray(got[key], dtype=np.float64).astype(LD) - r)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(err == 0, 0, err / (LD(bar) * scale))
        out[key] = float(np.max(np.where(np.isnan(q), np.inf, q)))
    return out


def run_workers(jobs, out_dir, timeout=600):
    """tests/blocks_forms_worker.py once per (mode, CF_TUNE string), at most four processes side by side ->
    {(mode, tune): dict of its arrays}."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "blocks_forms_worker.py")
    results, jobs = {}, list(jobs)
    for first in range(0, len(jobs), 4):
        procs = []
        for k, (mode, tune) in enumerate(jobs[first:first + 4]):
            out = os.path.join(str(out_dir), f"blocks_{first + k}.npz")
            env = dict(os.environ)
            env.pop("CF_TUNE", None)
            if tune:
                env["CF_TUNE"] = tune
            p = subprocess.Popen([sys.executable, worker, out, mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            procs.append((mode, tune, out, p))
        try:
            for mode, tune, out, p in procs:
                log, _ = p.communicate(timeout=timeout)
                assert p.returncode == 0, f"worker {mode!r} under CF_TUNE={tune!r} failed ({p.returncode}):\n{log}"
                results[(mode, tune)] = dict(np.load(out))
        finally:
            for *_, p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
    return results
