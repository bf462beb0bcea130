"""Extended-precision (numpy longdouble) restatement of the reference's field.py for one row, the yardstick of the field tests.

It follows the script line by line -- the grid, the two integrands, scipy's cumulative trapezoid, ``interp1d`` (linear,
extrapolating) and ``np.interp`` -- with one deliberate difference: 1 + w is formed directly (thawing: 2 (1 + w0) a^3 / D), not
as 1 + (-1 + x), which in float64 keeps seven digits of x at a = 1e-3 and none at the first node.  The sums are sequential."""
import numpy as np

LD = np.longdouble
GYR = LD("9.77813")
THAWING, WCDM, CPL = "thawing", "wcdm", "cpl"


def linspace(lo, hi, n):
    """np.linspace in float64 (the grids are float64 objects in the script and on the device)."""
    return np.linspace(np.float64(lo), np.float64(hi), int(n))


def de(fde, a, w0, wa=0.0):
    """(1 + w, rho_de) at a, longdouble."""
    a, w0, wa = np.asarray(a, dtype=LD), LD(w0), LD(wa)
    if fde == THAWING:
        D = (1 + w0) * a**3 + 1 - w0
        return 2 * (1 + w0) * a**3 / D, 4 / D**2
    if fde == WCDM:
        return np.full(a.shape, 1 + w0, dtype=LD), a ** (-3 * (1 + w0))
    if fde == CPL:
        return 1 + w0 + wa * (1 - a), a ** (-3 * (1 + w0 + wa)) * np.exp(-3 * wa * (1 - a))
    raise ValueError(fde)


def cumtrapz(y, x):
    """scipy.integrate.cumulative_trapezoid(y, x, initial=0), sequential."""
    out = np.zeros(y.shape, dtype=LD)
    out[1:] = np.cumsum(np.diff(x) * (y[1:] + y[:-1]) / 2)
    return out


def interp1d_extrap(xq, x, y):
    """scipy.interpolate.interp1d(x, y, kind="linear", fill_value="extrapolate")(xq): searchsorted left, clipped to 1..n-1."""
    xq = np.asarray(xq, dtype=LD)
    i = np.clip(np.searchsorted(x, xq, side="left"), 1, x.size - 1)
    lo, hi = i - 1, i
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])
    out = slope * (xq - x[lo]) + y[lo]
    out[np.isnan(xq)] = np.nan
    return out


def np_interp(xq, x, y):
    """np.interp(xq, x, y): clamped outside, x[j] <= xq < x[j + 1] inside, the node's value at a node."""
    xq = np.asarray(xq, dtype=LD)
    j = np.clip(np.searchsorted(x, xq, side="right") - 1, 0, x.size - 2)
    slope = (y[j + 1] - y[j]) / (x[j + 1] - x[j])
    out = slope * (xq - x[j]) + y[j]
    out = np.where(xq <= x[0], y[0], np.where(xq >= x[-1], y[-1], out))
    out[np.isnan(xq)] = np.nan
    return out


def status_of(fde, H0, Om, w0, wa, orh2, a):
    """0 ok, 1 phantom (1 + w < 0 at a node), 2 invalid (non-finite parameter, H0 <= 0, E^2 <= 0 or non-finite at a node)."""
    pars = [H0, Om, w0] + ([wa] if fde == CPL else [])
    if not np.all(np.isfinite(pars)) or not H0 > 0:
        return 2
    with np.errstate(all="ignore"):
        opw, rho = de(fde, a, w0, wa)
        al = a.astype(LD)
        Or = LD(orh2) / (LD(H0) / 100) ** 2
        e2 = LD(Om) * al**-3 + Or * al**-4 + (1 - LD(Om) - Or) * rho
    if not np.all(np.isfinite(e2)) or not np.all(e2 > 0) or not np.all(np.isfinite(rho)):
        return 2
    return 1 if np.any(opw < 0) else 0


def row(fde, H0, Om, w0, wa=0.0, *, orh2=4.1835e-05, n_a=5000, a_min=1e-8, a_max=5.0, a_q=None, phi_q=None, t_q=None):
    """Everything the kernel returns for one row, longdouble.  phi_q / t_q: an array (given) or an int (the row's own grid)."""
    a64 = linspace(a_min, a_max, n_a)
    st = status_of(fde, H0, Om, w0, wa, orh2, a64)
    out = dict(status=st)
    nan = LD("nan")
    n_of = lambda v: 0 if v is None else (int(v) if np.isscalar(v) else len(v))
    if st == 2:
        for k in ("phi_today", "t_today", "hubble_time", "phi_max", "t_max"):
            out[k] = nan
        for names, v in ((("phi_a", "t_a", "w_a", "K_a", "V_a"), a_q), (("phi_grid", "a_phi", "V_phi"), phi_q),
                         (("t_grid", "a_t", "phi_t"), t_q)):
            for k in names:
                if v is not None:
                    out[k] = np.full(n_of(v), nan)
        return out
    a = a64.astype(LD)
    H0l, Oml = LD(H0), LD(Om)
    h = H0l / 100
    Or = LD(orh2) / h**2
    with np.errstate(all="ignore"):
        opw, rho = de(fde, a, w0, wa)
        E = np.sqrt(Oml * a**-3 + Or * a**-4 + (1 - Oml - Or) * rho)
        phi = cumtrapz(np.sqrt(np.maximum(opw * rho, 0)) / (a * H0l * E), a)
    hub = GYR / h
    t = cumtrapz(1 / (a * E), a) * hub
    if st == 1:
        phi = np.full(phi.shape, nan)
    out.update(phi=phi, t=t, a=a64, rho=rho, hubble_time=hub, phi_max=phi[-1], t_max=t[-1],
               phi_today=np_interp([1.0], a, phi)[0], t_today=np_interp([1.0], a, t)[0])
    with np.errstate(all="ignore"):
        if a_q is not None:
            aq = np.asarray(a_q, dtype=np.float64)
            o, r = de(fde, aq, w0, wa)
            o = np.where(np.isnan(aq), nan, o)  # a NaN query is NaN in every output, also where w does not depend on a
            out.update(phi_a=np_interp(aq, a, phi), t_a=np_interp(aq, a, t), w_a=o - 1, K_a=o * r / 2, V_a=(2 - o) * r / 2, rho_a=r)
        if phi_q is not None:
            own = np.isscalar(phi_q)
            pq = linspace(phi[0], phi[-1], phi_q) if own else np.asarray(phi_q, dtype=np.float64)
            if st == 1:
                out.update(phi_grid=np.full(pq.size, nan), a_phi=np.full(pq.size, nan), V_phi=np.full(pq.size, nan))
            else:
                ap = interp1d_extrap(pq, phi, a)
                o, r = de(fde, ap, w0, wa)
                out.update(phi_grid=pq.astype(LD), a_phi=ap, V_phi=(2 - o) * r / 2)
        if t_q is not None:
            own = np.isscalar(t_q)
            tq = linspace(t[min(10, n_a - 1)], min(1.5 * out["t_today"], 0.95 * t[-1]), t_q) if own else np.asarray(t_q, dtype=np.float64)
            out.update(t_grid=tq.astype(LD), a_t=interp1d_extrap(tq, t, a),
                       phi_t=np.full(tq.size, nan) if st == 1 else np_interp(tq, t, phi))
    return out
