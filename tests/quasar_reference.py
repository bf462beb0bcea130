"""
numpy restatement of the quasar Hubble-diagram likelihoods (the reference's quasars/qsr_*.py), vectorised over walkers.

Stated from the scripts' formulas, not from the engine: a recipe is (theta order, (n, k, p), which blocks, the box), the
data are the fixtures' arrays.  Used by tests/test_quasars_cpu.py against the fixtures and by the GPU tests as a second
opinion.
"""
import numpy as np

C = 299792.458
H0 = 70.0
N_GRID = 3000


def linspace(top, n=N_GRID, dtype=np.float64):
    """The scripts' grid: float64 nodes (they are data of the algorithm), held in the dtype of the run."""
    return np.linspace(0.0, float(top), n).astype(dtype)


def inv_e(z, om, w0, nkp):
    """1 / E(z) for walkers: om, w0 [W] -> [W, len(z)], in the dtype of z."""
    n, k, p = nkp  # Python scalars: they take the dtype of the arrays they meet
    zp1 = 1.0 + z
    x = zp1 ** k
    f = (n * x / (1.0 + (n - 1.0) * x))[None, :] ** (p * (1.0 + w0))[:, None]
    return 1.0 / np.sqrt(om[:, None] * (zp1 ** 3)[None, :] + (1.0 - om)[:, None] * f)


def cum_trapezoid(y, x):
    out = np.zeros_like(y)
    out[:, 1:] = np.cumsum(np.diff(x)[None, :] * (y[:, 1:] + y[:, :-1]) / 2.0, axis=1)
    return out


def interp_rows(zq, x, tab):
    """np.interp of every row of tab at zq.  np.interp computes in float64 whatever it is given, so any other dtype takes
    numpy's formula written out: fp[j] + (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j]), fp[j] itself on a node,
    the end values outside the grid."""
    if tab.dtype == np.float64:
        return np.stack([np.interp(zq, x, t) for t in tab])
    j = np.clip(np.searchsorted(x, zq, side="right") - 1, 0, len(x) - 2)
    t, h = zq - x[j], x[j + 1] - x[j]
    val = (tab[:, j + 1] - tab[:, j]) / h[None, :] * t[None, :] + tab[:, j]
    val = np.where((t == 0)[None, :], tab[:, j], val)
    val = np.where((zq >= x[-1])[None, :], tab[:, -1:], val)
    return np.where((zq <= x[0])[None, :], tab[:, :1], val)


def mu_at(zq, zp1, x, tab, c_h0=C / H0):
    """c_h0: c / H0, a number or one value per walker [W, 1]."""
    return 25.0 + 5.0 * np.log10(zp1[None, :] * c_h0 * interp_rows(zq, x, tab))


def solve_lower(L, r):
    """y of L y = r for every row of r, by forward substitution in the dtype of r (np.linalg stops at float64)."""
    y = np.zeros_like(r)
    for i in range(L.shape[0]):
        y[:, i] = (r[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
    return y


def evaluate(recipe, thetas, qsr, sn=None, bao=None, *, n_grid=N_GRID, h0=H0, z_top=None, sn_z_top=None, fixed=None,
             scale=None, dtype=np.float64):
    """recipe: dict(theta=names, nkp, bounds, sn_grid, sn_zhel).  qsr = (z, mu, sigma); sn = (z, z_hel, obs, cov);
    bao = (z, val, qty, cov).  Returns dict(logp, logl, chi2, lnsum, chi2_parts [W, 3], mu_sn, mu_qsr, bao_theory), float64.

    The defaults are the scripts: 3000 nodes, H0 = 70, the quasar grid to max z, the SN grid (recipe["sn_grid"]) to max z_sn.
    n_grid: nodes of every grid.  h0: the fixed H0; a theta column named "H0" takes its place.  z_top: top of the quasar grid.
    sn_z_top: top of the SN grid of its own, 0 = the SNe read the quasar grid (None: what the recipe says).
    fixed: {name: value} for any of Om, w0, offset, dM_qsr, s, rd that is not a theta column.  scale: {name: factor}, the
    parameter is theta x factor (the box is on theta itself).  dtype: the arithmetic runs in it (np.longdouble: the judge of
    the GPU tests); the grids' nodes, the Cholesky factor and the inverse BAO covariance are float64 data in every dtype,
    as the engine receives them."""
    th64 = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    th = th64.astype(dtype)
    idx = {name: k for k, name in enumerate(recipe["theta"])}
    fixed, scale = fixed or {}, scale or {}
    W = th.shape[0]

    def par(name):
        if name in idx:
            return th[:, idx[name]] * dtype(scale[name]) if name in scale else th[:, idx[name]]
        return np.full(W, fixed[name], dtype=dtype)

    om, w0, dmq, s = par("Om"), par("w0"), par("dM_qsr"), par("s")
    c_h0 = (dtype(C) / par("H0"))[:, None] if "H0" in idx else dtype(C) / dtype(h0)
    nkp = recipe["nkp"]
    qz, qmu, qsig = (np.asarray(a, dtype=np.float64).astype(dtype) for a in qsr)
    out = dict(chi2_parts=np.zeros((W, 3), dtype=dtype), mu_sn=None, bao_theory=None)
    with np.errstate(all="ignore"):
        xq = linspace(np.max(qz) if z_top is None else z_top, n_grid, dtype)
        tab_q = cum_trapezoid(inv_e(xq, om, w0, nkp), xq)
        mu_q = mu_at(qz, 1.0 + qz, xq, tab_q, c_h0)
        out["mu_qsr"] = mu_q
        var = qsig[None, :] ** 2 + (s ** 2)[:, None]
        d = qmu[None, :] - dmq[:, None] - mu_q
        # the scripts hold the quasar data as pandas Series, whose sum skips NaN terms (E^2 < 0 past some z, outside the box)
        out["chi2_parts"][:, 1] = np.nansum(d ** 2 / var, axis=1)
        lnsum = np.sum(np.log(var), axis=1)
        if sn is not None:
            sz, szh, sobs = (np.asarray(a, dtype=np.float64).astype(dtype) for a in sn[:3])
            own = recipe.get("sn_grid") if sn_z_top is None else sn_z_top > 0
            if own:
                xs = linspace(np.max(sz) if sn_z_top is None else sn_z_top, n_grid, dtype)
                tab_s = cum_trapezoid(inv_e(xs, om, w0, nkp), xs)
            else:
                xs, tab_s = xq, tab_q
            mu_s = mu_at(sz, 1.0 + (szh if recipe.get("sn_zhel") else sz), xs, tab_s, c_h0)
            out["mu_sn"] = mu_s
            r = sobs[None, :] - par("offset")[:, None] - mu_s
            L = np.linalg.cholesky(np.asarray(sn[3], dtype=np.float64))
            ok = np.all(np.isfinite(r), axis=1)
            y = np.full_like(r, np.nan)
            if ok.any():
                y[ok] = np.linalg.solve(L, r[ok].T).T if dtype == np.float64 else solve_lower(L.astype(dtype), r[ok])
            out["chi2_parts"][:, 0] = np.sum(y ** 2, axis=1)
        if bao is not None:
            bz, bv, bq, bcov = bao
            rd = par("rd")
            h0v = par("H0") if "H0" in idx else dtype(h0)
            pred = np.empty((W, len(bz)), dtype=dtype)
            seen = {}
            for k, (z, q) in enumerate(zip(bz, bq)):
                # a repeated redshift gives the same numbers again: kept from its first datum, only to spare the long-double
                # run the repeated quadrature (the scripts recompute it per datum)
                if float(z) not in seen:
                    xb = linspace(z, n_grid, dtype)
                    seen[float(z)] = (dtype(C) / h0v * cum_trapezoid(inv_e(xb, om, w0, nkp), xb)[:, -1],
                                      dtype(C) / (h0v / inv_e(np.array([z], dtype=dtype), om, w0, nkp)[:, 0]))
                dm, dh = seen[float(z)]
                pred[:, k] = (dm if q == 1 else dh if q == 2 else (dtype(z) * dh * dm ** 2) ** (1.0 / 3.0)) / rd
            out["bao_theory"] = pred
            dv = np.asarray(bv, dtype=np.float64).astype(dtype)[None, :] - pred
            out["chi2_parts"][:, 2] = np.einsum("wi,ij,wj->w", dv, np.linalg.inv(np.asarray(bcov, dtype=np.float64)).astype(dtype), dv)
        chi2 = out["chi2_parts"].sum(axis=1)
        out["chi2"] = chi2
        out["lnsum"] = lnsum
        out["logl"] = -0.5 * (out["chi2_parts"][:, 0] + out["chi2_parts"][:, 2]) - 0.5 * (out["chi2_parts"][:, 1] + lnsum)
        b = np.asarray(recipe["bounds"], dtype=np.float64)
        inbox = np.all((b[:, 0] < th64) & (th64 < b[:, 1]), axis=1)
        out["logp"] = np.where(inbox, out["logl"], -np.inf)
    return {k: (v if v is None else np.asarray(v, dtype=np.float64)) for k, v in out.items()}


SCRIPTS = {"qsr_pantheon": "quasars/qsr_pantheon.py", "qsr_des5y": "quasars/qsr_des5y.py", "qsr_union3": "quasars/qsr_union3.py",
           "qsr_desi": "quasars/qsr_desi.py", "qsr_des5y_desi": "quasars/qsr_des5y_desi.py",
           "qsr_union3_unbinned": "quasars/qsr_union3.py"}
CASES = list(SCRIPTS)


def fixture_data(g, synthetic_cov):
    """(qsr, sn, bao) of a fixture: sn = (z, z_hel, obs, cov) with the stored or the regenerated synthetic covariance,
    bao = (dict(z, value, quantity), cov)."""
    qsr = (g["qsr_z"], g["qsr_mu"], g["qsr_sigma"])
    sn = bao = None
    if "sn_z" in g:
        cov = g["sn_cov"] if "sn_cov" in g else synthetic_cov(g["sn_sigma"])
        sn = (g["sn_z"], g["sn_zhel"], g["sn_obs"], cov)
    if "bao_z" in g:
        bao = (dict(z=g["bao_z"], value=g["bao_val"], quantity=g["bao_qty"]), g["bao_cov"])
    return qsr, sn, bao
