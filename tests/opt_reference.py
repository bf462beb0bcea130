"""numpy restatement of the optimizer's kernels (csrc/cosmofit_opt.hip) for tests/test_optimize_cpu.py and
tests/test_gpu_optimize.py: the stencil forms and rows, the gradient, the projection, the BFGS update, the direction, the trial
rows and the accept step of one problem, in float64 with the kernels' operation order, and a driver that runs the whole
iteration on a numpy objective."""
import math

import numpy as np

DELTA = 2.0 ** -40
RUNNING, CONVERGED, NOISE_FLOOR, ITER_CAP, NONFINITE_START, NONFINITE_STENCIL = range(6)
NEED_RESET, HAS_PAIR, FRESH, HAS_STEP = 1, 2, 4, 8


class Params:
    def __init__(self, bounds, free=None, h=1e-6, n_trials=4, gtol=1e-5, gtol_rel=None, max_iter=200, c1=1e-4, delta=DELTA):
        b = np.asarray(bounds, dtype=np.float64)
        self.ndim = b.shape[0]
        self.free = list(range(self.ndim)) if free is None else sorted(free)
        self.lo, self.width = b[:, 0].copy(), b[:, 1] - b[:, 0]
        self.h, self.delta, self.c1, self.gtol = h, delta, c1, gtol
        self.gtol_rel = 16.0 * 2.0 ** -52 / h if gtol_rel is None else gtol_rel
        self.K, self.max_iter = n_trials, max_iter


class Problem:
    """One problem's state: u [ndim], f, g / g_prev / s / d [n_free], H [n_free, n_free], forms, flags, status, n_iter."""

    def __init__(self, p, u, f):
        nf = len(p.free)
        self.u, self.f = np.array(u, dtype=np.float64), float(f)
        self.g, self.g_prev, self.s, self.d = (np.zeros(nf) for _ in range(4))
        self.H = np.zeros((nf, nf))
        self.form = np.zeros(nf, dtype=np.int64)
        self.gnorm, self.flags, self.n_iter = math.inf, NEED_RESET, 0
        self.status = RUNNING if math.isfinite(self.f) else NONFINITE_START


def clamp(v, delta):
    return min(max(v, delta), 1.0 - delta)


def trial_u(u, d, k, delta):
    return clamp(u + math.ldexp(1.0, -2 * k) * d, delta)


def form(u, h, delta):
    h2 = 2.0 * h
    return 1 if (u - delta) < h2 else (-1 if (1.0 - delta) - u < h2 else 0)


def theta(p, u):
    return p.lo + u * p.width


def start_u(p, x0):
    return np.array([clamp(v, p.delta) for v in (np.asarray(x0, dtype=np.float64) - p.lo) / p.width])


def stencil(p, st):
    """The 2 n_free rows (theta) of the problem; sets st.form."""
    rows = []
    h, h2 = p.h, 2.0 * p.h
    for j, c in enumerate(p.free):
        uc = st.u[c]
        fm = form(uc, h, p.delta)
        st.form[j] = fm
        for side in (0, 1):
            v = st.u.copy()
            if fm == 0:
                v[c] = uc - h if side else uc + h
            elif fm > 0:
                v[c] = uc + h2 if side else uc + h
            else:
                v[c] = uc - h2 if side else uc - h
            rows.append(theta(p, v))
    return np.array(rows)


def _sum(v):
    s = 0.0
    for x in v:
        s = s + x
    return s


def _max_abs(v):
    s = 0.0
    for x in v:
        s = float(np.fmax(s, abs(x)))
    return s


def direction(p, st, fs):
    """Gradient, convergence test, BFGS update, direction; returns the K trial rows (theta)."""
    nf, f0, h2, delta = len(p.free), st.f, 2.0 * p.h, p.delta
    g = np.zeros(nf)
    bad = False
    with np.errstate(invalid="ignore"):
        for i in range(nf):
            f1, f2 = fs[2 * i], fs[2 * i + 1]
            bad = bad or not (math.isfinite(f1) and math.isfinite(f2))
            fm = st.form[i]
            g[i] = (f1 - f2) / h2 if fm == 0 else (((4.0 * f1 - 3.0 * f0) - f2) / h2 if fm > 0 else ((3.0 * f0 - 4.0 * f1) + f2) / h2)
    ui = np.array([st.u[c] for c in p.free])
    held = np.array([(ui[i] <= delta and g[i] < 0.0) or (ui[i] >= 1.0 - delta and g[i] > 0.0) for i in range(nf)])
    pg = np.where(held, 0.0, g)
    gnorm = _max_abs(pg)
    conv = not bad and gnorm <= p.gtol + p.gtol_rel * abs(f0)
    flags, d, H = st.flags, np.zeros(nf), st.H.copy()
    if not bad and not conv:
        reset = bool(flags & NEED_RESET)
        if not reset and flags & HAS_PAIR:
            s, y = st.s.copy(), np.where(held, 0.0, st.g_prev - g)
            sy, ss, yy = _sum(s * y), _sum(s * s), _sum(y * y)
            if sy > 0.0 and sy * sy > (1e-20 * ss) * yy:
                hy = np.array([_sum(H[i] * y) for i in range(nf)])
                yhy = _sum(y * hy)
                rho = 1.0 / sy
                b = (1.0 + rho * yhy) * rho
                Hn = np.empty_like(H)
                for i in range(nf):
                    for j in range(nf):
                        t = hy[i] * s[j] + s[i] * hy[j]
                        Hn[i, j] = (H[i, j] - rho * t) + b * (s[i] * s[j])
                H = Hn
        if not reset:
            v = np.array([_sum(H[i] * pg) for i in range(nf)])
            d = np.where(held, 0.0, v)
            reset = not (_sum(pg * d) > 0.0)
        if reset:
            dmax = _max_abs(st.d)  # the failed search's direction (0 before the first search)
            after_fail = bool(flags & NEED_RESET) and dmax > 0.0
            m = min(0.1, 4.0 * _max_abs(st.s)) if flags & HAS_STEP else 0.1
            if after_fail:
                m = min(m, math.ldexp(dmax, -2 * p.K))  # the backtracking sequence continued
            sigma = m / gnorm
            H = np.diag(np.full(nf, sigma))
            d = sigma * pg
            flags = (flags & ~(NEED_RESET | FRESH)) | (FRESH if after_fail else 0)
        else:
            flags &= ~FRESH
        st.H = H
    st.g, st.d, st.gnorm, st.flags = g, d, gnorm, flags
    if bad:
        st.status = NONFINITE_STENCIL
    elif conv:
        st.status = CONVERGED
    rows = []
    for k in range(p.K):
        v = st.u.copy()
        for i, c in enumerate(p.free):
            v[c] = trial_u(st.u[c], d[i], k, delta)
        rows.append(theta(p, v))
    return np.array(rows)


def accept(p, st, ft):
    if st.status != RUNNING:
        return
    nf, f0 = len(p.free), st.f
    floor = f0 + math.ldexp(abs(f0), -50)  # a trial must beat f by more than its rounding noise, 4 eps |f|
    pick = -1
    for k in range(p.K):
        dec = 0.0
        for j, c in enumerate(p.free):
            dec = dec + st.g[j] * (trial_u(st.u[c], st.d[j], k, p.delta) - st.u[c])
        if math.isfinite(ft[k]) and ft[k] >= f0 + p.c1 * dec and ft[k] > floor:
            pick = k
            break
    if pick < 0:
        best = floor
        for k in range(p.K):
            if math.isfinite(ft[k]) and ft[k] > best:
                best, pick = ft[k], k
    flags, status = st.flags, RUNNING
    if pick >= 0:
        s = np.zeros(nf)
        for j, c in enumerate(p.free):
            un = trial_u(st.u[c], st.d[j], pick, p.delta)
            s[j] = un - st.u[c]
            st.u[c] = un
        st.s, st.g_prev, st.f = s, st.g.copy(), float(ft[pick])
        flags = (flags | HAS_PAIR | HAS_STEP) & ~(NEED_RESET | FRESH)
    elif flags & FRESH:
        status = NOISE_FLOOR
    else:
        flags = (flags | NEED_RESET) & ~HAS_PAIR
    st.n_iter += 1
    if status == RUNNING and st.n_iter >= p.max_iter:
        status = ITER_CAP
    st.flags, st.status = flags, status


def run(p, fun, x0):
    """The whole iteration on a numpy objective fun(theta [W, ndim]) -> [W] from one start row; returns the Problem."""
    u = start_u(p, x0)
    st = Problem(p, u, fun(theta(p, u)[None, :])[0])
    while st.status == RUNNING:
        fs = fun(stencil(p, st))
        tr = direction(p, st, fs)
        ft = fun(tr)
        accept(p, st, ft)
    return st
