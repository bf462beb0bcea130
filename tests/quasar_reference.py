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


def linspace(top, n=N_GRID):
    return np.linspace(0.0, top, n)


def inv_e(z, om, w0, nkp):
    """1 / E(z) for walkers: om, w0 [W] -> [W, len(z)]."""
    n, k, p = nkp
    zp1 = 1.0 + z
    x = zp1 ** k
    f = (n * x / (1.0 + (n - 1.0) * x))[None, :] ** (p * (1.0 + w0))[:, None]
    return 1.0 / np.sqrt(om[:, None] * (zp1 ** 3)[None, :] + (1.0 - om)[:, None] * f)


def cum_trapezoid(y, x):
    out = np.zeros_like(y)
    out[:, 1:] = np.cumsum(np.diff(x)[None, :] * (y[:, 1:] + y[:, :-1]) / 2.0, axis=1)
    return out


def interp_rows(zq, x, tab):
    return np.stack([np.interp(zq, x, t) for t in tab])


def mu_at(zq, zp1, x, tab):
    return 25.0 + 5.0 * np.log10(zp1[None, :] * (C / H0) * interp_rows(zq, x, tab))


def evaluate(recipe, thetas, qsr, sn=None, bao=None):
    """recipe: dict(theta=names, nkp, bounds, sn_grid, sn_zhel).  qsr = (z, mu, sigma); sn = (z, z_hel, obs, cov);
    bao = (z, val, qty, cov).  Returns dict(logp, logl, chi2_parts [W, 3], mu_sn, mu_qsr, bao_theory)."""
    th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    idx = {name: k for k, name in enumerate(recipe["theta"])}
    om, w0 = th[:, idx["Om"]], th[:, idx["w0"]]
    dmq, s = th[:, idx["dM_qsr"]], th[:, idx["s"]]
    nkp = recipe["nkp"]
    qz, qmu, qsig = (np.asarray(a, dtype=np.float64) for a in qsr)
    W = th.shape[0]
    out = dict(chi2_parts=np.zeros((W, 3)), mu_sn=None, bao_theory=None)
    with np.errstate(all="ignore"):
        xq = linspace(np.max(qz))
        tab_q = cum_trapezoid(inv_e(xq, om, w0, nkp), xq)
        mu_q = mu_at(qz, 1.0 + qz, xq, tab_q)
        out["mu_qsr"] = mu_q
        var = qsig[None, :] ** 2 + (s ** 2)[:, None]
        d = qmu[None, :] - dmq[:, None] - mu_q
        # the scripts hold the quasar data as pandas Series, whose sum skips NaN terms (E^2 < 0 past some z, outside the box)
        out["chi2_parts"][:, 1] = np.nansum(d ** 2 / var, axis=1)
        lnsum = np.sum(np.log(var), axis=1)
        if sn is not None:
            sz, szh, sobs, scov = (np.asarray(a, dtype=np.float64) for a in sn)
            if recipe.get("sn_grid"):
                xs = linspace(np.max(sz))
                tab_s = cum_trapezoid(inv_e(xs, om, w0, nkp), xs)
            else:
                xs, tab_s = xq, tab_q
            mu_s = mu_at(sz, 1.0 + (szh if recipe.get("sn_zhel") else sz), xs, tab_s)
            out["mu_sn"] = mu_s
            r = sobs[None, :] - th[:, idx["offset"]][:, None] - mu_s
            L = np.linalg.cholesky(scov)
            ok = np.all(np.isfinite(r), axis=1)
            y = np.full_like(r, np.nan)
            if ok.any():
                y[ok] = np.linalg.solve(L, r[ok].T).T
            out["chi2_parts"][:, 0] = np.sum(y ** 2, axis=1)
        if bao is not None:
            bz, bv, bq, bcov = bao
            rd = th[:, idx["rd"]]
            pred = np.empty((W, len(bz)))
            for k, (z, q) in enumerate(zip(bz, bq)):
                xb = linspace(z)
                dm = C / H0 * cum_trapezoid(inv_e(xb, om, w0, nkp), xb)[:, -1]
                dh = C / (H0 / inv_e(np.array([z]), om, w0, nkp)[:, 0])
                pred[:, k] = (dm if q == 1 else dh if q == 2 else (z * dh * dm ** 2) ** (1.0 / 3.0)) / rd
            out["bao_theory"] = pred
            dv = np.asarray(bv)[None, :] - pred
            out["chi2_parts"][:, 2] = np.einsum("wi,ij,wj->w", dv, np.linalg.inv(bcov), dv)
        chi2 = out["chi2_parts"].sum(axis=1)
        out["chi2"] = chi2
        out["logl"] = -0.5 * (out["chi2_parts"][:, 0] + out["chi2_parts"][:, 2]) - 0.5 * (out["chi2_parts"][:, 1] + lnsum)
        b = np.asarray(recipe["bounds"], dtype=np.float64)
        inbox = np.all((b[:, 0] < th) & (th < b[:, 1]), axis=1)
        out["logp"] = np.where(inbox, out["logl"], -np.inf)
    return out


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
