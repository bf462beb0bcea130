"""
Long-double numpy restatement of the SN residual rows of the per-walker stage (walker_kernel, walker_fast_kernel,
walker_stream_kernel of csrc/cosmofit_kernels.hip), written from the reference's expressions (sn/pantheon.py:43-61,
bao/desi_cmb_pantheon_H0trgb.py:102-106; the lines cited next to each), not from the kernels:

    z_pec = 100 v step_i / c,  z_cosmo = -1 + (1 + z_cmb) / (1 + z_pec)                      sn/pantheon.py:46-48
    mu_corr = 5 log10(DM(z_cosmo) / DM(z_cmb)),  mu_theory = 25 + 5 log10((1 + z_hel) DM(z_cmb))    :49, :52-54
    delta = obs - offset_i - mu_corr - mu_theory,  offset_i = offset (+ lin coef_i)          :60, H0trgb:104-105

The trapezoid table is tests/derived_reference.table (long double); the Hermite cubic is evaluated here at a LONG-DOUBLE
abscissa (the kernels and the float64 oracle round z_cosmo to float64 first, which is what moves a residual at very low
redshift: ``env``), with the reference's linear extrapolation at and below node 0 and at and above z_max (interpolator.py:87-92).

An ``sn`` dict says what the SN block says: z_cmb, z_hel, obs, step (+-1 or general weights; None: no velocity step at all),
lin_coef (None, or the coefficients of the linear magnitude term; then there is no velocity step).  The Model carries the slots
"offset" and "v" / "lin" beside the cosmology's.
"""
import numpy as np

import derived_reference as R

LD = np.longdouble
ENV_UNIT = LD(2.0) ** -52 * 5 / np.log(LD(10))  # one ulp of 1 + z in z_cosmo, in magnitudes per unit of (1 + z) / |z_cosmo|


def hermite(xq, zg, y, d):
    """interpolator.py:71-108 with exact=True for one row: y, d [G] long double, xq [n] LONG DOUBLE."""
    xl = zg.astype(LD)
    i = np.clip(np.searchsorted(xl, xq, side="left") - 1, 0, len(xl) - 2)  # x[i] < xq <= x[i + 1], interpolator.py:94
    h = xl[i + 1] - xl[i]
    t = (xq - xl[i]) / h
    t2, t3 = t * t, t * t * t
    out = (2 * t3 - 3 * t2 + 1) * y[i] + (t3 - 2 * t2 + t) * h * d[i] + (-2 * t3 + 3 * t2) * y[i + 1] + (t3 - t2) * h * d[i + 1]
    out = np.where(xq <= xl[0], y[0] + d[0] * (xq - xl[0]), out)
    return np.where(xq >= xl[-1], y[-1] + d[-1] * (xq - xl[-1]), out)


def residuals(m: R.Model, sn: dict, theta, bounds=None) -> dict:
    """For theta [W, ndim] float64:
    delta [W, n] long double (NaN / inf where the reference's own expression gives them), z_cosmo [W, n] long double,
    env [W, n]: what one ulp of 1 + z in z_cosmo moves the residual by, 2^-52 (5 / ln 10) (1 + z_i) / |z_cosmo_i|,
    nonpos [W, n]: z_cosmo <= 0 (the distance is <= 0 there and its logarithm not a number),
    bad_row [W]: a non-finite parameter, out_of_box [W]: outside the strict box `bounds` [ndim, 2] (None: no box)."""
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    z_cmb, z_hel, obs = (np.asarray(sn[k], dtype=np.float64).astype(LD) for k in ("z_cmb", "z_hel", "obs"))
    W, n = th.shape[0], z_cmb.size
    zg, cum, dh = R.table(m, th)
    offset = m.slot("offset", th)[:, None] * np.ones(n, dtype=LD)
    if sn.get("lin_coef") is not None:
        offset = offset + m.slot("lin", th)[:, None] * np.asarray(sn["lin_coef"], dtype=np.float64).astype(LD)
    if sn.get("step") is not None and sn.get("lin_coef") is None:
        v_km_s = 100 * m.slot("v", th)[:, None] * np.asarray(sn["step"], dtype=np.float64).astype(LD)
        z_pec = v_km_s / LD(m.c)
        z_cosmo = -1 + (1 + z_cmb) / (1 + z_pec)
    else:  # bao/desi_des5y_bbn_theta_star.py:94-97: no step term at all
        z_cosmo = np.broadcast_to(z_cmb, (W, n)).copy()
    delta = np.empty((W, n), dtype=LD)
    with np.errstate(all="ignore"):
        for r in range(W):
            DM = hermite(z_cmb, zg, cum[r], dh[r])
            mu_corr = 5 * np.log10(hermite(z_cosmo[r], zg, cum[r], dh[r]) / DM)
            mu_theory = 25 + 5 * np.log10((1 + z_hel) * DM)
            delta[r] = obs - offset[r] - mu_corr - mu_theory
        env = ENV_UNIT * (1 + z_cmb) / np.abs(z_cosmo)
    finite_row = np.all(np.isfinite(th), axis=1)
    box = np.ones(W, dtype=bool)
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.float64)
        box = np.all((b[:, 0] < th) & (th < b[:, 1]), axis=1)  # sn/pantheon.py:82; False for a NaN
    return dict(delta=delta, z_cosmo=z_cosmo, env=env, nonpos=z_cosmo <= 0, bad_row=~finite_row, out_of_box=~box & finite_row)
