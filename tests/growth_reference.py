"""
Long-double numpy restatement of the growth-rate block f sigma_8 (growth_kernel in csrc/cosmofit_kernels.hip and the host tables
of csrc/cosmofit_api.hip), written from the equations of the kernel's header comment and of include/cosmofit.h, not from its code:

    delta'' = -(3 / a + E_a / E) delta' + (3/2) Om delta / (a^5 E^2),   E_a / E = -(dE^2/dz) / (2 a^2 E^2),
    from a_init (delta = a_init, delta' = 1) to a = 1;   theory_k = (sigma_8 / delta(1)) a_k delta'(a_k).

In x = ln a, with y = (delta, delta'), the equation is dy/dx = A(x) y, A = [[0, a], [s, -p]], s = (3/2) Om / (a^4 E^2),
p = 3 - (dE^2/dz) / (2 a E^2).  The library takes S classical RK4 steps of h = -ln a_init / S; the restatement does the same at
the same S -- the step matrix M = I + (h/6)(K1 + 2 K2 + 2 K3 + K4) built for all steps at once, then applied ONE STEP AFTER THE
OTHER to y (the scan's association is the kernel's business) -- and reads delta' out the library's way: cubic Hermite inside the
step that contains ln a_k from (delta', d delta'/dx = s delta - p delta') at the step boundaries, either at the datum itself
(n_agrid = 0) or at the nodes of np.logspace(log10 a_init, 0, N) followed by interp_pchip's rule (interpolator.py:5-108).

Everything runs in the dtype asked for: np.longdouble (64-bit mantissa on the hosts this runs on) is the judge, np.float64 is what
tests/test_growth_shapes_cpu.py compares it with to show that the cases are well conditioned.  E^2 and the neutrino density are
derived_reference's (``Model``, ``_cosmo``, ``_f_de``); their z-derivatives are stated here.  ``defect`` switches on one of the
wrong formulae the CPU file uses to show that the GPU bar would see them; ``converged`` is the independent truth (scipy DOP853 on
the second-order equation in a, rtol 1e-13), used by the CPU file only.
"""
import numpy as np

import derived_reference as R

LD = np.longdouble
DEFECTS = ("cpl_drop_wa_za", "wcdm_zp1_for_a", "interior_slopes_at_ends", "midpoint_at_step_start")


def effective_steps(requested: int) -> int:
    """include/cosmofit.h: fs8_steps is rounded up to 256, 512, 1024 (0 = default) or 2048."""
    want = requested if requested > 0 else 1024
    return next(s for s in (256, 512, 1024, 2048) if s >= want)


# ---- E^2 and dE^2/dz ---------------------------------------------------------------------------------------------------------
def _cast(c, dt):
    return {k: v.astype(dt) for k, v in c.items()}


def _nu(comp, zp1, dt):
    """(nu(z), d nu/dz): nu = (1 + z)^4 sum_i w_i sqrt(q_i^2 + m0^2 / (1 + z)^2) / rho0 (cmb/data_planck_act_compression.py:53-66),
    d nu/dz = nu 3 (1 + w_nu) / (1 + z) with w_nu = (1/3)(1 - m_z^2 sum(w_i / f_i) / sum(w_i f_i)) (:70-83)."""
    mz_sq = (dt(comp["nu_m0"]) / zp1) ** 2
    f = [np.sqrt(dt(comp["nu_qs_sq"][i]) + mz_sq) for i in range(5)]
    den = sum(dt(comp["nu_ws"][i]) * f[i] for i in range(5))
    num = sum(dt(comp["nu_ws"][i]) / f[i] for i in range(5))
    nu = zp1**4 * den / dt(comp["nu_rho0"])
    w_nu = (1 - mz_sq * num / den) / 3
    return nu, nu * 3 * (1 + w_nu) / zp1


def e2_and_slope(m: R.Model, c, zp1, dt=LD, defect=None):
    """(E^2, dE^2/dz) at 1 + z = zp1 [P] for the rows of c ([W, 1] entries): fs8/fs8.py:26-56, bao/desi_cmb_union3_fs8.py:46-66,127-140."""
    z = zp1 - 1
    w0, wa = c["w0"], c["wa"]
    f = R._f_de(m, c, z)
    if m.fde == R.LCDM:
        df = np.zeros_like(f)
    elif m.fde == R.WCDM:                              # f = (1 + z)^(3 (1 + w0))
        df = f * 3 * (1 + w0) * zp1 if defect == "wcdm_zp1_for_a" else f * 3 * (1 + w0) / zp1
    elif m.fde == R.THAWING:                           # f = (2 u / D)^2, u = (1 + z)^3, D = (1 + w0) + (1 - w0) u
        df = f * 6 * (1 + w0) / (zp1 * ((1 + w0) + (1 - w0) * zp1**3))
    else:                                              # f = (1 + z)^(3 (1 + w0 + wa)) exp(-3 wa z / (1 + z))
        df = f * 3 * (1 + w0) / zp1 if defect == "cpl_drop_wa_za" else f * 3 * (1 + w0 + wa * z / zp1) / zp1
    if m.ez_model == R.LATE_FLAT:
        om = c["Om"]
        return om * zp1**3 + (1 - om) * f, 3 * om * zp1**2 + (1 - om) * df
    nu, dnu = _nu(m.comp, zp1, dt)
    e2 = c["Or"] * zp1**4 + c["Obc"] * zp1**3 + c["Ode"] * f + c["Onu"] * nu
    return e2, 4 * c["Or"] * zp1**3 + 3 * c["Obc"] * zp1**2 + c["Ode"] * df + c["Onu"] * dnu


def _matter(m: R.Model, c):
    """Omega_m of the source term: slot OM (late-time flat) or (omega_b + omega_c) / h^2 (physical), include/cosmofit.h."""
    return c["Om"] if m.ez_model == R.LATE_FLAT else c["Obc"]


def _coefficients(m, c, a, dt, defect):
    zp1 = 1 / a
    e2, de2 = e2_and_slope(m, c, zp1, dt, defect)
    return 1.5 * _matter(m, c) / (a**4 * e2), 3 - de2 / (2 * a * e2)


# ---- integration -------------------------------------------------------------------------------------------------------------
def step_matrices(m: R.Model, theta, a_init, S, dt=LD, defect=None):
    """(x0, h, s [W, 2 S + 1], p [W, 2 S + 1], M [W, S, 2, 2]): A's entries at the boundaries and midpoints, the RK4 step matrices"""
    _, c = R._cosmo(m, theta)
    c = _cast(R._col(c), dt)
    x0 = np.log(dt(a_init))
    h = -x0 / S
    a = np.exp(x0 + np.arange(2 * S + 1).astype(dt) * (h / 2))
    a[-1] = 1                                          # the last point is a = 1 exactly
    s, p = _coefficients(m, c, a, dt, defect)          # [W, 2 S + 1]
    W = s.shape[0]

    def A(j):                                          # [W, n, 2, 2]
        out = np.zeros((W, len(j), 2, 2), dtype=dt)
        out[..., 0, 1], out[..., 1, 0], out[..., 1, 1] = a[j], s[:, j], -p[:, j]
        return out

    start, end = 2 * np.arange(S), 2 * np.arange(S) + 2
    mid = start if defect == "midpoint_at_step_start" else start + 1
    eye = np.eye(2, dtype=dt)
    A0, Ah, A1 = A(start), A(mid), A(end)
    K1 = A0
    K2 = Ah @ (eye + (h / 2) * K1)
    K3 = Ah @ (eye + (h / 2) * K2)
    K4 = A1 @ (eye + h * K3)
    return x0, h, s, p, eye + (h / 6) * (K1 + 2 * K2 + 2 * K3 + K4)


def integrate(m: R.Model, theta, a_init, S, dt=LD, defect=None):
    """S RK4 steps from ln a_init to 0.  Returns (x0, h, dprime [W, S + 1], slope [W, S + 1], delta1 [W]): delta' and
    d delta'/dx at the step boundaries, delta at a = 1."""
    x0, h, s, p, M = step_matrices(m, theta, a_init, S, dt, defect)
    W = s.shape[0]
    y1, y2 = np.empty((W, S + 1), dtype=dt), np.empty((W, S + 1), dtype=dt)
    y1[:, 0], y2[:, 0] = dt(a_init), 1                 # fs8/fs8.py:79-82
    for i in range(S):
        y1[:, i + 1] = M[:, i, 0, 0] * y1[:, i] + M[:, i, 0, 1] * y2[:, i]
        y2[:, i + 1] = M[:, i, 1, 0] * y1[:, i] + M[:, i, 1, 1] * y2[:, i]
    b = 2 * np.arange(S + 1)
    return x0, h, y2, s[:, b] * y1 - p[:, b] * y2, y1[:, -1]


def _hermite(x0, h, S, dprime, slope, ln_a):
    """delta' at ln_a [n] by the cubic Hermite of the step that contains it -> [W, n]"""
    i = np.clip(np.floor((ln_a - x0) / h).astype(np.int64), 0, S - 1)
    t = (ln_a - (x0 + i * h)) / h
    t2, t3 = t * t, t * t * t
    return ((2 * t3 - 3 * t2 + 1) * dprime[:, i] + (t3 - 2 * t2 + t) * h * slope[:, i]
            + (-2 * t3 + 3 * t2) * dprime[:, i + 1] + (t3 - t2) * h * slope[:, i + 1])


# ---- interp_pchip (interpolator.py:5-108) in the dtype of y --------------------------------------------------------------------
def pchip_slopes(x, y, interior_at_ends=False):
    h = np.diff(x)
    sec = np.diff(y) / h
    d = np.zeros(len(x), dtype=y.dtype)
    dl, dr, hl, hr = sec[:-1], sec[1:], h[:-1], h[1:]
    w1, w2 = 2 * hr + hl, hr + 2 * hl
    with np.errstate(all="ignore"):
        d[1:-1] = np.where((dl != 0) & (dr != 0) & (dl * dr > 0), (w1 + w2) / (w1 / dl + w2 / dr), 0)   # :25-40

    def end(h0, h1, d0, d1):                                                                            # :41-66
        e = ((2 * h0 + h1) * d0 - h0 * d1) / (h0 + h1)
        if d0 == 0 or np.sign(e) != np.sign(d0):
            return 0
        if np.sign(d0) != np.sign(d1) and abs(e) > abs(3 * d0):
            return 3 * d0
        return e

    if interior_at_ends:  # the defect: the harmonic mean of a node's two nearest secants where the three-point formula belongs
        d[0], d[-1] = d[1], d[-2]
    else:
        d[0], d[-1] = end(h[0], h[1], sec[0], sec[1]), end(h[-1], h[-2], sec[-1], sec[-2])
    return d


def pchip(xq64, x64, y, interior_at_ends=False):
    """interp_pchip(xq, x, y) for one row: x64, xq64 float64 (searchsorted sees the caller's bits), y in the working dtype."""
    dt = y.dtype.type
    x, xq = x64.astype(dt), xq64.astype(dt)
    d = pchip_slopes(x, y, interior_at_ends)
    i = np.clip(np.searchsorted(x64, xq64, side="left") - 1, 0, len(x64) - 2)     # :94
    h = x[i + 1] - x[i]
    t = (xq - x[i]) / h
    t2, t3 = t * t, t * t * t
    out = (2 * t3 - 3 * t2 + 1) * y[i] + (t3 - 2 * t2 + t) * h * d[i] + (-2 * t3 + 3 * t2) * y[i + 1] + (t3 - t2) * h * d[i + 1]
    return np.where(xq64 <= x64[0], y[0], np.where(xq64 >= x64[-1], y[-1], out))  # :80-85


def a_grid(a_init, n_agrid):
    """the scripts' a_span (fs8/fs8.py:79), numpy's float64 bits"""
    return np.logspace(np.log10(a_init), 0, n_agrid)


# ---- theory, chi^2, log L ----------------------------------------------------------------------------------------------------
def theory(m: R.Model, theta, z, *, a_init, S, n_agrid=0, dt=LD, defect=None):
    """[W, n] f sigma_8 before the Alcock-Paczynski division, at the effective step count S."""
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    x0, h, dprime, slope, delta1 = integrate(m, th, a_init, S, dt, None if defect == "interior_slopes_at_ends" else defect)
    a = 1 / (1 + z.astype(dt))
    if n_agrid == 0:
        dp = _hermite(x0, h, S, dprime, slope, np.log(a))
    else:
        nodes = a_grid(a_init, n_agrid)
        ln_nodes = np.log(nodes.astype(dt))
        ln_nodes[-1] = 0
        at_nodes = _hermite(x0, h, S, dprime, slope, ln_nodes)
        a64 = 1.0 / (1.0 + z)                          # the query the library hands its interpolant
        dp = np.stack([pchip(a64, nodes, at_nodes[r], defect == "interior_slopes_at_ends") for r in range(th.shape[0])])
    s8 = m.slot("s8", th).astype(dt)
    return (s8 / delta1)[:, None] * a * dp


def ap_factor(m: R.Model, theta, z, fid):
    """q_k = H(z_k) D_M(z_k) / fid_k, long double [W, n]"""
    return R.curves(m, theta, z, "H") * R.curves(m, theta, z, "DM") / np.asarray(fid, dtype=np.float64).astype(LD)


def chi2(m: R.Model, theta, fs8, *, S, dt=LD, q=None):
    """[W] f_err^2 Delta^T C^-1 Delta, Delta = val - theory / q, for the ``fs8`` dict of a LikelihoodEngine (q: ap_factor)."""
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    t = theory(m, th, fs8["z"], a_init=fs8["a_init"], S=S, n_agrid=fs8.get("a_grid", 0), dt=dt)
    q = ap_factor(m, th, fs8["z"], fs8["fid"]) if q is None else q
    inv = np.asarray(fs8["inv_cov"], dtype=np.float64).astype(dt)
    ferr = m.slot("fs8err", th).astype(dt) if "fs8err" in m.params else np.ones(th.shape[0], dtype=dt)
    with np.errstate(divide="ignore", invalid="ignore"):   # q = 0 at z = 0: chi^2 is then not a number, by the equations
        delta = np.asarray(fs8["val"], dtype=np.float64).astype(dt) - t / q.astype(dt)
        quad = np.array([delta[r] @ (inv @ delta[r]) for r in range(th.shape[0])], dtype=dt)
    return ferr**2 * quad


def logl_terms(m: R.Model, theta, n_fs8, logl_const=0.0):
    """what log L adds to -0.5 chi^2 for the growth block: n ln f_err + logl_const (fs8/fs8.py:123-125)"""
    th = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    ferr = m.slot("fs8err", th) if "fs8err" in m.params else np.ones(th.shape[0], dtype=LD)
    return n_fs8 * np.log(ferr) + LD(logl_const)


# ---- the truth: the second-order equation in a, integrated to convergence -------------------------------------------------------
def converged(m: R.Model, theta_row, z, *, a_init, rtol=1e-13):
    """f sigma_8 [n] of ONE theta from scipy's DOP853 on the equation of the header comment (float64, dense output)."""
    from scipy.integrate import solve_ivp

    th = np.atleast_2d(np.asarray(theta_row, dtype=np.float64))
    _, c = R._cosmo(m, th)
    c = _cast(R._col(c), np.float64)
    om = float(_matter(m, c)[0, 0])

    def rhs(a, y):
        e2, de2 = e2_and_slope(m, c, np.array([1.0 / a]), np.float64)
        e2, de2 = float(e2[0, 0]), float(de2[0, 0])
        ea_over_e = -de2 / (2 * a * a * e2)
        return [y[1], -(3 / a + ea_over_e) * y[1] + 1.5 * om * y[0] / (a**5 * e2)]

    a = 1.0 / (1.0 + np.atleast_1d(np.asarray(z, dtype=np.float64)))
    out = np.empty(a.size)
    y, a_at = np.array([a_init, 1.0]), a_init
    for k in list(np.argsort(a)) + [-1]:  # no dense output (7th order only): integrate to each datum in ascending a, then to a = 1
        stop = 1.0 if k < 0 else a[k]
        if stop > a_at:
            seg = solve_ivp(rhs, (a_at, stop), y, method="DOP853", rtol=rtol, atol=1e-16)
            y, a_at = seg.y[:, -1], stop
        if k >= 0:
            out[k] = a[k] * y[1]
    return float(m.slot("s8", th)[0]) * out / y[0]
