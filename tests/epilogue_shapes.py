"""Cases of the prior / output epilogue sweep (tests/test_epilogue_cpu.py, tests/test_gpu_epilogue.py): a dozen tiny engines that
between them fill every field of cf_epilogue (csrc/cosmofit_device.h) to its limit, 41 base rows each with named special rows, and
the batches that put those rows on every route finalize_value (csrc/cosmofit_kernels.hip) is reached by.

A case is a plain dict (``CASES[name]``) that tests/epilogue_reference.py reads directly; ``engine_kwargs`` / ``twin_kwargs`` /
``oracle_likelihood`` turn it into the LikelihoodEngine's keywords, those of its twin (the same blocks without priors, bounds, wall,
Gaussian terms or logl_const: the engine's own plain chi^2) and the float64 oracle's descriptor.  Everything here is plain numpy:
importing this module needs neither the library nor a GPU.

Column 0 of every case is Om (a row with Om = -0.5 has E^2 < 0 below z = 1.5: chi^2 is NaN, and the box admits it).  ``names`` lists
the slot each theta column feeds (None: a column no slot reads, which then appears in the box and in the Gaussian terms only)."""
import dataclasses

import numpy as np

import solve_shapes
from oracle import oracle_np as onp

N_SN, N_GRID, Z_HI, Z_TURN = 65, 513, 1.5, 0.15  # two row blocks
Z_MAX = Z_HI + 0.1
LCDM, CPL = onp.FDE_LCDM, onp.FDE_CPL
CF_MAX_NDIM, CF_MAX_GAUSS = 16, 8

# per slot: the range of the ordinary rows and the strict box of the prior around it (in the slot's own units)
BOX = dict(Om=(0.2, 0.45), H0=(60.0, 80.0), offset=(-19.5, -19.1), v=(-1.0, 1.0), w0=(-1.2, -0.6), wa=(-1.5, 0.5), fcc=(0.8, 1.3),
           fs8err=(0.8, 1.3), s8=(0.7, 0.9), rd=(140.0, 155.0), dM_qsr=(-0.3, 0.3), s=(0.3, 1.0), u=(-0.8, 0.8))
BOUNDS = dict(Om=(-1.0, 0.9), H0=(50.0, 90.0), offset=(-20.0, -19.0), v=(-3.0, 3.0), w0=(-1.5, 0.5), wa=(-2.0, 1.5), fcc=(0.5, 2.0),
              fs8err=(0.5, 2.0), s8=(0.5, 1.1), rd=(110.0, 170.0), dM_qsr=(-0.5, 0.5), s=(0.1, 2.5), u=(-1.0, 1.0))
FIXED = dict(H0=70.0, offset=-19.3, rd=147.0)  # what a small ndim cannot hold
OM_NAN, OM_NAN_OUT, OM_OUT = -0.5, -1.5, 0.95  # E^2 < 0 inside the box; the same outside it; outside with a finite chi^2
W0_WALL, WA_WALL, W0_PAST = -0.75, 0.75, -0.5  # w0 + wa == 0.0 exactly; -0.5 + 0.75 > 0
WA_FIXED = WA_WALL                             # the case with wa fixed: the same w0 on and past the wall

B, STRIDE = 41, 7  # base rows; rows[i] = base[(7 i) mod 41]
ROUTES = ("finalize", "blocked", "inverse")
W_LIST = dict(finalize=(1, 255, 256, 257), blocked=(1, 17, 33, 161), inverse=(1, 17, 96, 97, 160, 161, 512, 513, 545))
# (kernel, panel_width, tpw) of cf_solve_form that each W of the inverse route is listed under
INVERSE_FORMS = {1: (0, 16, 1), 17: (0, 16, 1), 96: (0, 16, 1), 97: (0, 16, 2), 160: (0, 16, 2), 161: (1, 16, 0), 512: (1, 16, 0),
                 513: (1, 32, 0), 545: (1, 32, 0)}
ROUTE_TABLE = (  # (route of the issue's table, this sweep's route, the W that reach it)
    ("finalize_kernel", "finalize", W_LIST["finalize"]),
    ("trsm_chi2_kernel", "blocked", W_LIST["blocked"]),
    ("tri_gemm_small_kernel TPW 1", "inverse", (1, 17, 96)),
    ("tri_gemm_small_kernel TPW 2", "inverse", (97, 160)),
    ("tri_gemm_chi2_kernel panel_last_arriver<1>", "inverse", (161, 512)),
    ("tri_gemm_chi2_kernel panel_last_arriver<2>", "inverse", (513, 545)),
)


def batch_rows(W):
    return (STRIDE * np.arange(W)) % B


def panel_width(route, W):
    return 256 if route == "finalize" else (16 if route == "blocked" else INVERSE_FORMS[W][1])


def tail_rows(route):
    """Base rows that sit in a partly filled last panel of some batch of the route."""
    out = set()
    for W in W_LIST[route]:
        pw = panel_width(route, W)
        if W % pw:
            out |= set(batch_rows(W)[W - W % pw:].tolist())
    return out


def lane_rows(route, lane):
    """Base rows on lane `lane` (-1: the last) of a full panel of some batch of the route."""
    out = set()
    for W in W_LIST[route]:
        pw = panel_width(route, W)
        full = W // pw
        if full:
            out |= set(batch_rows(W)[np.arange(full) * pw + (lane % pw)].tolist())
    return out


# The special rows.  The walkers alone in a partly filled last panel of the solve routes are i = 16, 32, 96, 160, 512, 544, and
# i = 256 for finalize_kernel; i = 0 is the whole batch of W = 1.  Their base rows (7 i mod 41) = 30, 19, 16, 13, 17, 36, 29, 0 hold
# the specials that a wrong stride or a copy that stops short would hit first; the others sit elsewhere.
SPECIALS = dict(nan_in=0, wall_zero=30, out_last=19, nan_unread=16, face_lo=13, wall_nan=17, nan_out=36, wall_out=29,
                face_hi=6, ulp_lo=5, ulp_hi=9, out_col0=12, wall_past=20, in_box=1)  # on first and last lanes of 16-walker panels
ORDINARY = tuple(i for i in range(B) if i not in set(SPECIALS.values()) - {SPECIALS["in_box"]})


def _terms(kind, ndim, n, names, scale, nan_col):
    """n Gaussian terms: entry 0 on column ndim - 1, entries 1 and 2 both on column 0, the rest over the other columns (never
    nan_col); every entry with its own mean and sigma.  The mean lies 0.1 .. 0.31 box widths beyond the ordinary rows' range and
    sigma is 0.5 .. 0.99 widths, so every term is at least (0.1 / 0.99)^2 > 1e-2 (5e-3 halved) on an ordinary row."""
    cols = [ndim - 1, 0, 0] + [c for c in range(ndim - 2, 0, -1) if c != nan_col] * 8
    out = []
    for g in range(n):
        c = cols[g] if g < len(cols) else 0
        lo, hi = _col_range(BOX, names[c], scale)
        w = hi - lo
        if kind == "gauss":
            out.append((c, hi + (0.1 + 0.03 * g) * w, (0.5 + 0.07 * g) * w))
        else:
            out.append((c, lo - (0.1 + 0.03 * g) * w, (0.6 + 0.05 * g) * w))
    return tuple(out)


def _col_range(table, name, scale):
    lo, hi = table["u" if name is None else name]
    s = scale.get(name, 1.0)
    return lo / s, hi / s


def _case(name, names, *, fde=LCDM, gauss=0, chi2_gauss=0, box="bounds", wall=False, fixed=None, scale=None, logl_const=0.0,
          cc=None, fs8=False, sn=True, bao=False, quasar=False):
    ndim, scale = len(names), dict(scale or {})
    fixed = dict(fixed or {})
    unread = [k for k, n in enumerate(names) if n is None]
    nan_col = unread[0] if len(unread) > 1 or (unread and unread[0] != ndim - 1) else None
    slots = {n: (k, scale.get(n, 1.0)) for k, n in enumerate(names) if n is not None}
    for n in ("H0", "offset", "rd"):
        if n not in slots and n not in fixed:
            fixed[n] = FIXED[n]
    slots.update({n: ("fixed", v) for n, v in fixed.items()})
    bounds = None if box == "none" else np.array([_col_range(BOUNDS, n, scale) for n in names])
    return dict(name=name, ndim=ndim, names=tuple(names), slots=slots, scale=scale, fde=fde, nan_col=nan_col, bounds=bounds,
                prior_normalised=box != "unnormalised", gauss=_terms("gauss", ndim, gauss, names, scale, nan_col),
                chi2_gauss=_terms("chi2_gauss", ndim, chi2_gauss, names, scale, nan_col), cpl_wall=wall, logl_const=logl_const,
                cc=cc, n_cc=5 if cc else 0, cc_f_inverse=cc == "inverse", cc_logdet=_cc_data()["logdet"] if cc else 0.0,
                n_fs8=3 if fs8 else 0, sn=sn, bao=bao, quasar=quasar, routes=("inverse", "blocked") if sn else ("finalize",))


def _cases():
    U = None
    out = [
        _case("n1_gauss1", ["Om"], gauss=1),
        _case("n3_unnormalised", ["Om", "H0", "offset"], chi2_gauss=1, box="unnormalised", logl_const=-41.25),
        _case("n4_wall_free", ["Om", "H0", "w0", "wa"], fde=CPL, gauss=8, chi2_gauss=8, wall=True),
        _case("n5_wall_wa_fixed", ["Om", "H0", "offset", "w0", "v"], fde=CPL, gauss=8, wall=True, fixed=dict(wa=WA_FIXED)),
        _case("n8_cc_nobox", ["Om", "H0", "offset", "v", "fcc", U, U, U], chi2_gauss=8, box="none", cc="direct"),
        _case("n9_cc_inverse_cpl", ["Om", "H0", "offset", "v", "w0", "wa", "fcc", U, U], fde=CPL, gauss=1, chi2_gauss=1, cc="inverse"),
        _case("n15_wall_scaled", ["Om", "H0", "offset", "v", "w0", "wa"] + [U] * 9, fde=CPL, gauss=8, chi2_gauss=1, wall=True,
              scale=dict(w0=0.5), logl_const=12.5),
        _case("n16_growth", ["Om", "H0", "offset", "v", "s8", "fs8err"] + [U] * 10, gauss=1, chi2_gauss=8, fs8=True),
        _case("n16_wall_full", ["Om", "H0", "offset", "v", "w0", "wa", "fcc"] + [U] * 9, fde=CPL, gauss=8, chi2_gauss=8, wall=True,
              box="unnormalised", cc="direct", logl_const=3.0),
        _case("n8_no_sn_wall", ["Om", "H0", "rd", U, "fcc", "w0", "wa", U], fde=CPL, gauss=8, chi2_gauss=8, wall=True, cc="inverse",
              sn=False, bao=True, logl_const=-7.5),
        _case("n3_no_sn_nobox", ["Om", "H0", "fcc"], gauss=1, box="none", cc="direct", sn=False),
        _case("n5_quasar", ["Om", "w0", "offset", "dM_qsr", "s"], gauss=8, chi2_gauss=1, quasar=True, fixed=dict(H0=70.0)),
    ]
    return {c["name"]: c for c in out}


# ---- data (seeded, computed once) -------------------------------------------------------------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def sn_block():
    def make():
        z, zh, obs, chol = solve_shapes.sn_data(np.random.default_rng(6500), N_SN, Z_HI)
        return dict(z_cmb=z, z_hel=zh, obs=obs, chol=chol)
    return _once("sn", make)


def _cc_data():
    def make():
        rng = np.random.default_rng(6501)
        z = np.array([0.2, 0.5, 0.9, 1.2, 1.45])
        h = 70.0 * np.sqrt(0.3 * (1 + z) ** 3 + 0.7) * (1 + 0.05 * rng.standard_normal(z.size))
        A = rng.standard_normal((z.size, 2))
        cov = np.diag((0.08 * h) ** 2) + 4.0 * A @ A.T
        return dict(z=z, h=h, inv_cov=np.linalg.inv(cov), logdet=float(np.linalg.slogdet(cov)[1]))
    return _once("cc", make)


def _bao_data():
    def make():
        rng = np.random.default_rng(6502)
        z, qty = np.array([0.4, 0.7, 1.0, 1.3]), np.array([0, 1, 2, 3], dtype=np.int32)
        lk = onp.Likelihood(ndim=2, z_max=Z_MAX, n_grid=N_GRID, Om=onp.Slot(0), H0=onp.Slot(1), rd=onp.Slot(fixed=147.0), bao_z=z, bao_qty=qty)
        val = onp.bao_theory(lk, np.array([0.3, 70.0])) * (1 + 0.01 * rng.standard_normal(z.size))
        s = 1.0 / (0.02 * np.abs(val))
        return dict(z=z, val=val, qty=qty, inv_cov=np.outer(s, s) * (np.eye(z.size) + 0.1))
    return _once("bao", make)


def _fs8_data():
    def make():
        rng = np.random.default_rng(6503)
        z = np.array([0.3, 0.6, 1.0])
        hd = 70.0 * np.sqrt(0.3 * (1 + z) ** 3 + 0.7) * 4283.0 * z * (1 + 0.4 * z) / (1 + z)
        return dict(z=z, val=0.45 * (1 + 0.1 * rng.standard_normal(z.size)), inv_cov=np.eye(z.size) / 0.05**2, fid=hd, a_init=1e-3)
    return _once("fs8", make)


def _qsr_data():
    def make():
        rng = np.random.default_rng(6504)
        z = np.sort(rng.uniform(0.05, 2.0, 50))
        sig = rng.uniform(0.3, 1.5, z.size)
        mu = 25 + 5 * np.log10((1 + z) * 4283.0 * z * (1 + 0.4 * z) / (1 + 0.1 * z * z)) + sig * rng.standard_normal(z.size)
        return dict(z=z, mu=mu, sigma=sig, z_top=float(z[-1]))
    return _once("qsr", make)


# ---- base rows --------------------------------------------------------------------------------------------------------------------
def present(case):
    """name -> base row of the special rows this case can form: the wall rows need the wall, nan_unread a column that neither a slot
    nor a Gaussian term reads.  (The rows of an absent special stay ordinary.)"""
    out = dict(SPECIALS)
    if not case["cpl_wall"]:
        for k in ("wall_zero", "wall_past", "wall_nan", "wall_out"):
            out.pop(k)
    if case["nan_col"] is None:
        out.pop("nan_unread")
    return out


def nan_chi2_rows(name):
    """[41] bool: the base rows whose chi^2 is NaN, from the rows alone: Om <= -0.5 (E^2 < 0 somewhere below the highest datum)."""
    return base_rows(name)[:, 0] <= OM_NAN


def face_col(case):
    """The column of the face rows: column 1 (a finite chi^2 on either face), column 0 where there is no other."""
    return min(1, case["ndim"] - 1)


def base_rows(name):
    """[41, ndim] float64, read-only: ordinary rows inside BOX (w0 + wa <= -0.1 where either is a column), the specials of
    ``present(case)`` at their SPECIALS rows."""
    def make():
        case = CASES[name]
        names, scale, ndim = case["names"], case["scale"], case["ndim"]
        rng = np.random.default_rng(sum(name.encode()) + 6600)
        th = np.stack([rng.uniform(*_col_range(BOX, n, scale), B) for n in names], axis=1)
        col = {n: k for k, n in enumerate(names) if n is not None}

        def put(r, slot_name, value):
            th[r, col[slot_name]] = value / scale.get(slot_name, 1.0)

        wa_of = (lambda r: th[r, col["wa"]]) if "wa" in col else (lambda r: case["slots"].get("wa", ("fixed", 0.0))[1])
        if "w0" in col and case["fde"] == CPL:
            for r in range(B):  # ordinary: w0 + wa <= -0.1
                w0 = th[r, col["w0"]] * scale.get("w0", 1.0)
                put(r, "w0", min(w0, -0.1 - wa_of(r)))
        sp = present(case)
        lim = np.array([_col_range(BOUNDS, n, scale) for n in names])
        fc, last = face_col(case), ndim - 1
        th[sp["face_lo"], fc], th[sp["face_hi"], fc] = lim[fc, 0], lim[fc, 1]
        th[sp["ulp_lo"], fc], th[sp["ulp_hi"], fc] = np.nextafter(lim[fc, 0], np.inf), np.nextafter(lim[fc, 1], -np.inf)
        put(sp["out_col0"], "Om", OM_OUT)
        th[sp["out_last"], last] = lim[last, 1] + 0.3 * (lim[last, 1] - lim[last, 0])
        put(sp["nan_in"], "Om", OM_NAN)
        put(sp["nan_out"], "Om", OM_NAN_OUT)
        if "nan_unread" in sp:
            th[sp["nan_unread"], case["nan_col"]] = np.nan
        if case["cpl_wall"]:
            free_wa = "wa" in col
            for key, w0 in (("wall_zero", W0_WALL), ("wall_past", W0_PAST), ("wall_nan", W0_WALL), ("wall_out", W0_WALL)):
                if key not in sp:
                    continue
                r = sp[key]
                if free_wa:
                    put(r, "w0", w0)
                    put(r, "wa", WA_WALL)
                else:
                    put(r, "w0", w0)
            put(sp["wall_nan"], "Om", OM_NAN)
            if "wall_out" in sp:
                put(sp["wall_out"], "H0", 95.0)
        th.setflags(write=False)
        return th
    return _once(("rows", name), make)


# ---- engine, twin, oracle ---------------------------------------------------------------------------------------------------------
def _blocks(case):
    kw = {}
    if case["sn"]:
        kw["sn"] = dict(z_turn=Z_TURN, step=None, **sn_block())
    if case["cc"]:
        d = _cc_data()
        kw["cc"] = dict(z=d["z"], h=d["h"], inv_cov=d["inv_cov"], logdet=d["logdet"], f_inverse=case["cc_f_inverse"])
    if case["bao"]:
        kw["bao"] = dict(_bao_data())
    if case["n_fs8"]:
        kw["fs8"] = dict(_fs8_data())
    return kw


def _params(case, Param, skip=()):
    out = {}
    for n, (a, b) in case["slots"].items():
        if n not in skip:
            out[n] = Param(fixed=b) if a == "fixed" else Param(a, scale=b)
    return out


def twin_kwargs(pkg, name, route):
    """The same blocks, slots and route with nothing for the epilogue to do: CHI2 of it is the engine's own plain chi^2 (for the
    quasar engine -2 LOGL is the plain chi^2 of its LOGL / LOGP, which carries sum ln(sigma^2 + s^2))."""
    case = CASES[name]
    kw = dict(ndim=case["ndim"], z_max=Z_MAX, n_grid=N_GRID, fde=case["fde"], **_blocks(case))
    if case["sn"]:
        kw["solve_mode"] = pkg.engine.solve_mode_of(route)
    if case["quasar"]:
        q = _qsr_data()
        p = _params(case, pkg.Param)
        kw.update(z_max=q["z_top"], params={k: v for k, v in p.items() if k not in ("dM_qsr", "s")},
                  quasar=dict(z=q["z"], mu=q["mu"], sigma=q["sigma"], offset=p["dM_qsr"], scatter=p["s"], nkp=(2, 2, 3), z_top=q["z_top"]))
    else:
        kw["params"] = _params(case, pkg.Param)
    return kw


def engine_kwargs(pkg, name, route):
    case = CASES[name]
    return dict(twin_kwargs(pkg, name, route), bounds=case["bounds"], prior_normalised=case["prior_normalised"], gauss=case["gauss"],
                chi2_gauss=case["chi2_gauss"], cpl_wall=case["cpl_wall"], logl_const=case["logl_const"])


def oracle_likelihood(name, with_blocks=True):
    """oracle_np's descriptor of the case.  with_blocks=False (and always for the quasar case, which oracle_np has no blocks for):
    priors, wall, Gaussian terms and the normalisations only; chi2_fs8 is then up to the caller."""
    case = CASES[name]
    slots = {n: (onp.Slot(fixed=b) if a == "fixed" else onp.Slot(a, b)) for n, (a, b) in case["slots"].items() if n not in ("dM_qsr", "s")}
    kw = dict(ndim=case["ndim"], z_max=Z_MAX, n_grid=N_GRID, fde=case["fde"], bounds=case["bounds"], gauss=case["gauss"],
              chi2_gauss=case["chi2_gauss"], cpl_wall=case["cpl_wall"], prior_normalised=case["prior_normalised"],
              logl_const=case["logl_const"], has_vstep="v" in case["names"], z_turn=Z_TURN, **slots)
    if case["quasar"]:
        return onp.Likelihood(**kw)
    if case["sn"] and with_blocks:
        kw.update(sn_block())
    if case["cc"]:
        d = _cc_data()
        kw.update(cc_z=d["z"], cc_h=d["h"], cc_inv_cov=d["inv_cov"], cc_logdet=d["logdet"], cc_f_inverse=case["cc_f_inverse"])
    if case["bao"]:
        d = _bao_data()
        kw.update(bao_z=d["z"], bao_val=d["val"], bao_qty=d["qty"], bao_inv_cov=d["inv_cov"])
    if case["n_fs8"]:
        d = _fs8_data()
        kw.update(fs8_z=d["z"], fs8_val=d["val"], fs8_inv_cov=d["inv_cov"], fs8_fid=d["fid"])
    return onp.Likelihood(**kw)


def without_chi2_gauss(lk):
    return dataclasses.replace(lk, chi2_gauss=())


# ---- the struct walk ----------------------------------------------------------------------------------------------------------------
def epilogue_layout():
    """[(field, byte offset, bytes)] of cf_epilogue restated from csrc/cosmofit_device.h (int32 4, double 8, cf_dev_slot = int32 idx +
    padding, double scale, double fixed = 24 bytes; natural alignment)."""
    fields = [(n, 4, 4) for n in ("ndim", "has_bounds", "n_gauss", "n_chi2_gauss", "cpl_wall", "n_fs8", "n_cc", "cc_f_inverse")]
    fields += [(n, 8, 8) for n in ("log_norm", "logl_const", "cc_logdet")]
    fields += [(n, 24, 8) for n in ("w0", "wa", "fs8err", "fcc")]
    fields += [("lo", 8 * CF_MAX_NDIM, 8), ("hi", 8 * CF_MAX_NDIM, 8)]
    for kind in ("gauss", "chi2_gauss"):
        fields += [(kind + "_idx", 4 * CF_MAX_GAUSS, 4), (kind + "_mean", 8 * CF_MAX_GAUSS, 8), (kind + "_sigma", 8 * CF_MAX_GAUSS, 8)]
    out, off = [], 0
    for n, size, align in fields:
        off = -(-off // align) * align
        out.append((n, off, size))
        off += size
    return out, -(-off // 8) * 8


CASES = _cases()
ORACLE_CASES = tuple(n for n, c in CASES.items() if not c["n_fs8"] and not c["quasar"])  # end to end against oracle_np
