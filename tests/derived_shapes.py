"""
The engines behind the cases of tests/golden/derived.npz, stated once for the CPU and the GPU tests of ``derived``.

``engine_kwargs(pkg, case)`` are the keyword arguments of ``LikelihoodEngine`` for the script the case was generated from (the
slot mapping, model and blocks of the matching mirror in ``likelihoods``; the BAO data are bao_desi_cmb.npz's, which only has
to be there: no derived quantity reads a datum).  ``consts(pkg, case)`` are the ``derived.Spec`` constants, ``columns(case)``
the fixture's column names as ``Spec`` names, and ``model(pkg, case)`` the long-double restatement's ``Model`` of the same
keyword arguments.
"""
import numpy as np

import derived_reference as R
from conftest import golden

CASES = ("desi_cmb_thawing", "desi_cmb_lcdm", "desi_cmb_union3_fs8", "desi_union3_bbn", "desi_union3_bbn_thaw",
         "desi_des5y_obh2_theta_star", "cmb_cmb")

# fixture column -> Spec name, per case (the fixture's own key where they differ)
COLUMNS = {
    "desi_cmb_thawing": ("omh2", "Om", "z_star", "rd"),
    "desi_cmb_lcdm": ("omh2", "Om", "z_star", "rd"),
    "desi_cmb_union3_fs8": ("omh2", "Om", "S8", "rd", "q0", "j0"),
    "desi_union3_bbn": ("omh2", "rd", "q0", "j0"),
    "desi_union3_bbn_thaw": ("wa", "q0", "j0"),
    "desi_des5y_obh2_theta_star": ("omh2", "Om", "z_drag", "z_star"),
    "cmb_cmb": ("omh2", "Om", "z_drag", "r_drag", "z_eq", "theta_star100", "rs_star", "DM_star", "z_star"),
}
ZERO_CROSSING = ("q0", "j0")  # absolute bar 1e-12 instead of the relative 1e-10


def _bao(dh_exact=True, **kw):
    g = golden("bao_desi_cmb")
    return dict(z=g["bao_z"], val=g["bao_val"], qty=g["bao_qty"], inv_cov=g["bao_inv_cov"], dh_exact=dh_exact, **kw)


def _physical(comp):
    return {k: comp[k] for k in ("or_h2", "omnu_h2", "o_gamma_h2", "nu_m0", "nu_rho0", "nu_qs_sq", "nu_ws")}


def _cmb(comp):
    return dict(mode=comp["cmb_mode"], prior=comp["cmb_prior"], inv_cov=comp["cmb_inv_cov"], zstar_fit=comp["zstar_fit"])


def comp_of(pkg, case):
    cd = pkg.cmb_data
    return {"desi_cmb_thawing": cd.EARLY_LCDM, "desi_cmb_lcdm": cd.EARLY_LCDM, "desi_cmb_union3_fs8": cd.PLANCK_ACT,
            "desi_des5y_obh2_theta_star": cd.PLANCK_ACT, "cmb_cmb": cd.PLANCK_ACT}.get(case)


def engine_kwargs(pkg, case, n_grid=4000):
    P, L, cd = pkg.Param, pkg._lib, pkg.cmb_data
    comp = comp_of(pkg, case)
    z_max = float(golden("derived")["desi_cmb_thawing/z_max"])
    if case in ("desi_cmb_thawing", "desi_cmb_lcdm"):  # likelihoods.DesiCmb; the LambdaCDM line of bao/desi_cmb.py:22
        return dict(ndim=4, z_max=z_max, n_grid=n_grid, ez_model=L.CF_EZ_PHYSICAL,
                    fde=L.CF_FDE_THAWING if case == "desi_cmb_thawing" else L.CF_FDE_LCDM,
                    params=dict(H0=P(0), obh2=P(1), och2=P(2), w0=P(3)), bao=_bao(rd_fit=comp["rd_fit"]), cmb=_cmb(comp),
                    physical=_physical(comp))
    if case == "desi_cmb_union3_fs8":  # likelihoods.DesiCmbUnion3Fs8 without its SN and growth data
        return dict(ndim=6, z_max=z_max, n_grid=n_grid, ez_model=L.CF_EZ_PHYSICAL, fde=L.CF_FDE_LCDM,
                    params=dict(H0=P(1), obh2=P(2), och2=P(3), s8=P(5)), bao=_bao(rd_fit=comp["rd_fit"]), cmb=_cmb(comp),
                    physical=_physical(comp))
    if case in ("desi_union3_bbn", "desi_union3_bbn_thaw"):  # bao/desi_union3_bbn.py: late-time flat, r_drag(wb, Om h^2) with b = m = 1
        thaw = case.endswith("thaw")
        params = dict(H0=P(0), Om=P(1), obh2=P(2))
        if thaw:
            params["w0"] = P(5)
        return dict(ndim=6 if thaw else 5, z_max=z_max, n_grid=n_grid, fde=L.CF_FDE_THAWING if thaw else L.CF_FDE_LCDM, params=params,
                    bao=_bao(rd_fit=(1.0, 1.0) + cd.RDRAG_A, rd_wm_late=True))
    if case == "desi_des5y_obh2_theta_star":
        return dict(ndim=5, z_max=z_max, n_grid=n_grid, ez_model=L.CF_EZ_PHYSICAL, fde=L.CF_FDE_LCDM,
                    params=dict(H0=P(1), obh2=P(2), och2=P(3)), bao=_bao(rd_fit=comp["rd_fit"]), cmb=_cmb(comp), physical=_physical(comp))
    if case == "cmb_cmb":  # likelihoods.CmbOnly
        return dict(ndim=3, z_max=1.0, n_grid=n_grid, ez_model=L.CF_EZ_PHYSICAL, fde=L.CF_FDE_LCDM,
                    params=dict(H0=P(0), obh2=P(1), och2=P(2)), cmb=_cmb(comp), physical=_physical(comp))
    raise KeyError(case)


def consts(pkg, case):
    """Spec constants: the case's compression (z_drag coefficients, Omega_r h^2, and r_drag's for cmb/cmb.py, whose engine has
    no BAO block)."""
    comp = comp_of(pkg, case)
    return {} if comp is None else dict(comp=comp)


def model(pkg, case, n_grid=4000):
    comp = comp_of(pkg, case)
    extra = {}
    if comp is not None:
        extra = dict(comp=comp, zdrag_fit=comp["zdrag_fit"], zeq_or_h2=comp["zeq_or_h2"], rdrag_fit=comp["rd_fit"])
    return R.model_of(engine_kwargs(pkg, case, n_grid), **extra)


def thetas(case):
    g = golden("derived")
    if case == "desi_union3_bbn_thaw":
        return np.ascontiguousarray(np.hstack([g["desi_union3_bbn/thetas"], g["desi_union3_bbn/thaw_w0"][:, None]]))
    return np.ascontiguousarray(g[case + "/thetas"])


def expected(case):
    """[n, len(COLUMNS[case])] float64: the fixture's columns in COLUMNS order."""
    g = golden("derived")
    if case == "desi_union3_bbn_thaw":
        return np.stack([g["desi_union3_bbn/thaw_wa"], g["desi_union3_bbn/thaw_q0"], g["desi_union3_bbn/thaw_j0"]], axis=1)
    if case == "cmb_cmb":
        b = g["cmb_cmb/blobs"]  # (100 theta*, r*, D_M* / Gpc, z*)
        return np.stack([g["cmb_cmb/omh2"], g["cmb_cmb/Om"], g["cmb_cmb/z_drag"], g["cmb_cmb/r_drag"], g["cmb_cmb/z_eq"],
                         b[:, 0], b[:, 1], 1000 * b[:, 2], b[:, 3]], axis=1)
    return np.stack([g[case + "/" + name] for name in COLUMNS[case]], axis=1)


def applicable_scalars(pkg, case):
    """Every scalar name the case's engine accepts (with the case's constants), in _lib.DERIVED_CODES order, plus two at-z H."""
    info = pkg.engine.model_info(**engine_kwargs(pkg, case))
    D = pkg.derived
    comp = comp_of(pkg, case) or {}
    c = dict(zdrag_fit=comp.get("zdrag_fit"), rdrag_fit=comp.get("rd_fit"), zeq_or_h2=comp.get("zeq_or_h2"))
    names = [n for n in pkg._lib.DERIVED_CODES if n != "H@" and D._missing(info, n, c) is None]
    return names + ["H@0.51", "H@2.33"]
