"""
Long-double numpy restatement of what small_blocks_kernel (csrc/cosmofit_kernels.hip) computes -- the z* / r_drag fitting
formulae, the compressed-CMB vector and its chi^2, the cosmic-chronometer quadratic form, the BAO theory vector and its
quadratic form -- built on tests/derived_reference.py (Model, H_of_z, z_star, r_drag, _gl, table, _cubic, pchip_slopes), which
is written from the reference's expressions.  Shared by tests/test_blocks_cpu.py (against the fixtures and oracle/oracle_np.py)
and tests/test_gpu_blocks_shapes.py (against the kernel).

``reference(model, data, theta)``: ``data`` is a dict with the optional entries
    bao = dict(z, val, qty (0 D_V / r_d, 1 D_M / r_d, 2 D_H / r_d, 3 D_M / D_H), inv_cov)    [D_H: model.dh_exact; r_d: model.rd_fit]
    cc  = dict(z, h, inv_cov[, f_inverse])                                                   [f: the model's "fcc" slot, default 1]
    cmb = dict(mode (1 (R, l_A, wb), 2 l_A only, 3 (theta*, wb, wm)), prior[3], inv_cov[3, 3])
and the result holds, per theta row, in np.longdouble: bao_theory [n, n_bao], chi2_bao, cmb_vector [n, 3], chi2_cmb, chi2_cc,
z_star, r_drag, and for each chi^2 its ``scale_*``.

The scale of a chi^2 = d^T K d (d = data - theory t, K the inverse covariance, g = K d) is
    sum_ij |d_i| |K_ij| |d_j|  +  2 sum_i |g_i| |t_i|,
times f^2 (or f^-2) for the cosmic chronometers: the first term is what rounding the products of the quadratic form can move
relative to 1 ulp, the second what a relative error of the theory vector propagates to (d chi^2 = -2 g . dt).  A theory vector
within 1e-10 relative therefore leaves chi^2 within 1e-10 x scale, which is the bar the tests hold the kernel to.
"""
import numpy as np

import derived_reference as R

LD = np.longdouble


def _quad(d, K, t, factor=None):
    """(chi^2 [n], scale [n]) of residual rows d [n, k], theory rows t [n, k] and the inverse covariance K [k, k]."""
    K = np.asarray(K, dtype=np.float64).astype(LD)
    g = d @ K
    chi2 = np.sum(g * d, axis=1)
    scale = np.sum((np.abs(d) @ np.abs(K)) * np.abs(d), axis=1) + 2 * np.sum(np.abs(g) * np.abs(t), axis=1)
    if factor is not None:
        chi2, scale = chi2 * factor, scale * np.abs(factor)
    return chi2, scale


def rd_of(m: R.Model, c, th):
    """r_d of the BAO block: the "rd" slot, or the fitting formula with wm = wb + wc + w_nu (or Omega_m h^2: rd_wm_late)."""
    return R._rd(m, c, th)


def bao_theory(m: R.Model, theta, z, qty):
    """[n, len(z)] long double: bao/desi.py:38-56, bao/desi_cmb_des5y.py:82-100 (D_M by Hermite on the trapezoid table, D_H by
    PCHIP on the c / H grid or exactly as c / H(z); clamped / linearly continued outside the grid as interpolator.py does)."""
    th, c = R._cosmo(m, theta)
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    qty = np.asarray(qty).astype(int)
    zl = z.astype(LD)
    rd = rd_of(m, c, th)
    zg, cum, dh = R.table(m, th)
    Hq = R.H_of_z(m, R._col(c), zl) if m.dh_exact else None
    out = np.empty((th.shape[0], z.size), dtype=LD)
    for r in range(th.shape[0]):
        DM = R._cubic(z, zg, cum[r], dh[r], True)
        DH = LD(m.c) / Hq[r] if m.dh_exact else R._cubic(z, zg, dh[r], R.pchip_slopes(zg, dh[r]), False)
        with np.errstate(invalid="ignore"):
            DV = (zl * DH * DM**2) ** (LD(1) / 3)
        out[r] = np.where(qty == 2, DH / rd[r], np.where(qty == 1, DM / rd[r], np.where(qty == 0, DV / rd[r], DM / DH)))
    return out


def cmb_vector(m: R.Model, theta, mode):
    """(vector [n, 3], z* [n]): cmb/data_planck_act_compression.py:209-212 (modes 1, 2), cmb/data_early_lcdm_compression.py:206-207."""
    th, c = R._cosmo(m, theta)
    zs, rs, dm = R._gl(m, c)
    wm = c["wc"] + c["wb"] + LD(m.comp["omnu_h2"])
    if mode == 3:
        v = np.stack([rs / dm, c["wb"], wm], axis=1)
    else:
        v = np.stack([100 * np.sqrt(wm) * dm / LD(m.c), LD(np.pi) * dm / rs, c["wb"]], axis=1)
    return v, zs


def reference(m: R.Model, data: dict, theta) -> dict:
    th, c = R._cosmo(m, theta)
    n = th.shape[0]
    out = {}
    bao, cc, cmb = data.get("bao"), data.get("cc"), data.get("cmb")
    if bao is not None:
        t = bao_theory(m, th, bao["z"], bao["qty"])
        d = np.asarray(bao["val"], dtype=np.float64).astype(LD)[None, :] - t
        out["bao_theory"] = t
        out["chi2_bao"], out["scale_bao"] = _quad(d, bao["inv_cov"], t)
        out["r_drag"] = rd_of(m, c, th)
    if cmb is not None:
        mode = int(cmb["mode"])
        v, zs = cmb_vector(m, th, mode)
        d = np.asarray(cmb["prior"], dtype=np.float64).astype(LD)[None, :] - v
        K = np.asarray(cmb["inv_cov"], dtype=np.float64).reshape(3, 3)
        if mode == 2:  # bao/desi_des5y_bbn_theta_star.py:110-111
            out["chi2_cmb"], out["scale_cmb"] = _quad(d[:, 1:2], K[1:2, 1:2], v[:, 1:2])
        else:
            out["chi2_cmb"], out["scale_cmb"] = _quad(d, K, v)
        out["cmb_vector"], out["z_star"] = v, zs
    if cc is not None:
        t = R.H_of_z(m, R._col(c), np.asarray(cc["z"], dtype=np.float64).astype(LD))
        d = np.asarray(cc["h"], dtype=np.float64).astype(LD)[None, :] - t
        f = m.slot("fcc", th) if "fcc" in m.params else np.ones(n, dtype=LD)
        # ohd/cc_pantheon.py:64 / bao/desi_union3_cc_theta_star.py:130
        out["chi2_cc"], out["scale_cc"] = _quad(d, cc["inv_cov"], t, factor=1 / f**2 if cc.get("f_inverse", False) else f**2)
        out["cc_theory"] = t
    return out


def from_oracle(lk, zstar_consts):
    """(Model, data) of a float64 oracle descriptor (oracle/oracle_np.Likelihood): its slots, model, block options and data."""
    params = {}
    for name in ("H0", "Om", "obh2", "och2", "w0", "wa", "rd", "fcc"):
        s = getattr(lk, name)
        params[name] = (s.idx, s.scale) if s.idx >= 0 else ("fixed", s.fixed)
    comp = None
    if lk.ez_model == R.PHYSICAL or lk.cmb_mode:
        comp = dict(or_h2=lk.or_h2, omnu_h2=lk.omnu_h2, o_gamma_h2=lk.o_gamma_h2, nu_m0=lk.nu_m0, nu_rho0=lk.nu_rho0,
                    nu_qs_sq=lk.nu_qs_sq, nu_ws=lk.nu_ws, zstar_fit=lk.zstar_fit)
    m = R.Model(ndim=lk.ndim, params=params, z_max=lk.z_max, ez_model=lk.ez_model, fde=lk.fde, n_grid=lk.n_grid, om_mode=lk.om_mode,
                rd_fit=None if lk.rd_fit is None else tuple(lk.rd_fit), rd_wm_late=lk.rd_wm_late, dh_exact=lk.bao_dh_exact, comp=comp,
                zstar_consts=zstar_consts, n_gl=len(lk.gl_x) if lk.gl_x is not None else 100, c=lk.c)
    data = dict(bao=None, cc=None, cmb=None)
    if lk.bao_z is not None:
        data["bao"] = dict(z=lk.bao_z, val=lk.bao_val, qty=lk.bao_qty, inv_cov=lk.bao_inv_cov)
    if lk.cc_z is not None:
        data["cc"] = dict(z=lk.cc_z, h=lk.cc_h, inv_cov=lk.cc_inv_cov, f_inverse=lk.cc_f_inverse)
    if lk.cmb_mode:
        data["cmb"] = dict(mode=lk.cmb_mode, prior=lk.cmb_prior, inv_cov=lk.cmb_inv_cov)
    return m, data


def finite_box(m: R.Model, data: dict, theta) -> np.ndarray:
    """[n] bool: the row lies where every expression of the reference is finite -- E^2 > 0 on the grid, at the data and at the
    Gauss-Legendre nodes, a positive thawing denominator, positive bases of every power."""
    th, c = R._cosmo(m, theta)
    zs = [np.linspace(0, m.z_max, num=m.n_grid)]
    for key in ("bao", "cc"):
        if data.get(key) is not None:
            zs.append(np.asarray(data[key]["z"], dtype=np.float64))
    ok = c["H0"] > 0
    if data.get("cmb") is not None or m.rd_fit is not None:
        ok &= c["wb"] > 0
        ok &= (R._wm_drag(m, c) if m.rd_fit is not None else c["wb"] + c["wc"]) > 0
    if data.get("cmb") is not None:
        zstar = R.z_star(m.comp["zstar_fit"], m.zstar_consts, c["wb"], c["wc"] + c["wb"] + LD(m.comp["omnu_h2"]))
        ok &= np.isfinite(zstar) & (zstar > 0)
        x = np.polynomial.legendre.leggauss(m.n_gl)[0]
        zmaxgl = float(np.nanmax(np.where(ok, zstar, 0)))
        zs.append(zmaxgl / 2 * x + zmaxgl / 2)
        a = 1 / (1 + zmaxgl) / 2 * x + 1 / (1 + zmaxgl) / 2
        zs.append(1 / a - 1)
    z = np.concatenate(zs).astype(LD)
    cc_ = R._col(c)
    zp1 = 1 + z
    with np.errstate(all="ignore"):
        if m.fde == R.THAWING:
            ok &= np.all((1 + cc_["w0"]) + (1 - cc_["w0"]) * zp1**3 > 0, axis=1)
        f = R._f_de(m, cc_, z)
        if m.ez_model == R.LATE_FLAT:
            e2 = cc_["Om"] * zp1**3 + (1 - cc_["Om"]) * f
        else:
            e2 = cc_["Or"] * zp1**4 + cc_["Obc"] * zp1**3 + cc_["Ode"] * f + cc_["Onu"] * R._omnu_z(m.comp, z)
        ok &= np.all(np.isfinite(e2) & (e2 > 0), axis=1)
    return np.asarray(ok, dtype=bool)
