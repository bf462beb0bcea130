"""GPU (-m gpu): the batched maximizer (optimize.py, csrc/cosmofit_opt.hip).

* The kernels against the numpy restatement (tests/opt_reference.py) on random states: stencil and trial rows and the accept
  step bit for bit, gradient / H^-1 / direction within 1e-13.
* Analytic problems: a correlated Gaussian (free and with active bounds), Rosenbrock, 1-D and 2-D Gaussian profiles.
* Real data: sn/union3_1.py and bao/desi.py against scipy's L-BFGS-B on the CPU oracle, and against the published chi^2.
* Determinism: a problem's bits do not depend on the batch; the same seed gives the same bits.
* Edge cases: non-finite starts and stencils, the iteration cap.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import opt_reference as ref
from conftest import golden
from test_optimize_cpu import _corr_precision, kkt_box_max

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def opt(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.optimize


def _quad(mu, a):
    """Row-wise f = -1/2 (theta - mu)^T A (theta - mu) as elementwise torch ops summed in a fixed order (batch-invariant)."""
    mu, a = [float(v) for v in mu], np.asarray(a, dtype=np.float64).tolist()
    d = len(mu)

    def f(theta):
        x = [theta[:, i] - mu[i] for i in range(d)]
        v = torch.zeros(theta.shape[0], dtype=torch.float64, device=theta.device)
        for i in range(d):
            for j in range(d):
                v = v + (a[i][j] * x[i]) * x[j]
        return -0.5 * v

    return f


# ---- 1. kernels against the restatement ------------------------------------------------------------------------------
# (ndim, free, K, B, n_active): the shape the scripts use, then the ends of the ranges the C entry points accept -- one lane
# live and one trial, all sixteen lanes live with ndim = 16 (lane c also writes trial coordinate c) and eight trials, a single
# free coordinate in the last of sixteen, and more than 1024 active problems (the second pass of the compaction's chunk loop)
KERNEL_SHAPES = [(5, [0, 2, 3, 4], 4, 64, 50), (1, [0], 1, 64, 64), (16, list(range(16)), 8, 200, 150), (16, [15], 2, 64, 33),
                 (7, [1, 3, 5], 8, 3000, 2500)]


@pytest.mark.parametrize("d,free,K,B,n_active", KERNEL_SHAPES,
                         ids=["scripts_shape", "one_lane_one_trial", "sixteen_lanes", "last_of_sixteen", "two_compaction_passes"])
def test_kernels_against_the_restatement_on_random_states(pkg, opt, d, free, K, B, n_active):
    L, lib = pkg._lib, pkg.lib()
    rng = np.random.default_rng(11)
    nf = len(free)
    if d == 5:
        bounds = np.array([[-1.0, 2.0], [0.1, 0.7], [-9.0, 9.0], [50.0, 90.0], [-0.5, 0.5]])
        mu_h, sc_h = [0.3, 0.4, 1.0, 70.0, 0.1], [0.5, 0.1, 3.0, 5.0, 0.2]
    else:  # a generator of its own: the draws below are the same for every shape
        r2 = np.random.default_rng(1100 + d)
        lo = r2.uniform(-50.0, 50.0, d)
        bounds = np.stack([lo, lo + r2.uniform(0.2, 40.0, d)], axis=1)
        mu_h = list(bounds[:, 0] + r2.uniform(0.3, 0.7, d) * (bounds[:, 1] - bounds[:, 0]))
        sc_h = list(r2.uniform(0.1, 0.4, d) * (bounds[:, 1] - bounds[:, 0]))
    p = opt._params(bounds, free, opt._options(1e-6, K, 1e-5, None, 50, 1e-4))
    rp = ref.Params(bounds, free=free, n_trials=K, gtol=1e-5, max_iter=50)
    st = opt._State(B, d, DEV)
    u = rng.uniform(ref.DELTA, 1 - ref.DELTA, (B, d))
    # faces and one-sided stencils, on free coordinates
    u[:8, free[0]], u[8:16, free[1 % nf]], u[16:20, free[2 % nf]] = ref.DELTA, 1 - ref.DELTA, ref.DELTA + 1.5e-6
    u[20:24, free[3 % nf]] = 1 - ref.DELTA - 0.5e-6
    st.u.copy_(torch.from_numpy(u))
    st.f.copy_(torch.from_numpy(rng.normal(-5.0, 2.0, B)))
    st.g_prev[:, :nf] = torch.from_numpy(rng.normal(size=(B, nf)) * 10)
    st.s[:, :nf] = torch.from_numpy(rng.normal(size=(B, nf)) * 1e-2)
    hs = np.zeros((B, 16, 16))
    for b in range(B):
        m = rng.normal(size=(nf, nf))
        hs[b, :nf, :nf] = m @ m.T * 1e-3 + 1e-3 * np.eye(nf)
    st.hinv.copy_(torch.from_numpy(hs))
    flag_set = [L.CF_OPT_NEED_RESET, L.CF_OPT_HAS_PAIR | L.CF_OPT_HAS_STEP, L.CF_OPT_HAS_STEP,
                L.CF_OPT_HAS_PAIR | L.CF_OPT_HAS_STEP | L.CF_OPT_FRESH, L.CF_OPT_NEED_RESET | L.CF_OPT_HAS_STEP]
    st.flags.copy_(torch.tensor([flag_set[b % len(flag_set)] for b in range(B)], dtype=torch.int32))
    act = rng.permutation(B)[:n_active].astype(np.int32)
    dact = torch.from_numpy(act).to(DEV)
    n = act.size
    probs = []
    f_h, gp_h, s_h, fl_h = st.f.cpu().numpy(), st.g_prev.cpu().numpy(), st.s.cpu().numpy(), st.flags.cpu().numpy()  # one copy each
    for b in range(B):
        q = ref.Problem(rp, u[b], float(f_h[b]))
        q.g_prev, q.s = gp_h[b, :nf].copy(), s_h[b, :nf].copy()
        q.H, q.flags = hs[b, :nf, :nf].copy(), int(fl_h[b])
        probs.append(q)
    cs = st.c_struct()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rows = torch.empty((n * 2 * nf, d), dtype=torch.float64, device=DEV)
    L.check(lib.cf_opt_stencil(C.byref(p), C.byref(cs), dact.data_ptr(), n, rows.data_ptr(), stream))
    want_rows = np.concatenate([ref.stencil(rp, probs[b]) for b in act])
    np.testing.assert_array_equal(rows.cpu().numpy(), want_rows)
    np.testing.assert_array_equal(st.form[torch.from_numpy(act).long().to(DEV), :nf].cpu().numpy(), np.array([probs[b].form for b in act]))
    # stencil values: a smooth function of the rows, with one non-finite value in two problems
    mu = torch.tensor(mu_h, dtype=torch.float64, device=DEV)
    sc = torch.tensor(sc_h, dtype=torch.float64, device=DEV)
    fs = -0.5 * (((rows - mu) / sc) ** 2).sum(1)
    fs[3], fs[2 * nf * 7 + 1] = math.nan, -math.inf
    trials = torch.empty((n * K, d), dtype=torch.float64, device=DEV)
    L.check(lib.cf_opt_direction(C.byref(p), C.byref(cs), dact.data_ptr(), n, fs.data_ptr(), trials.data_ptr(), stream))
    fsh = fs.cpu().numpy()
    for a, b in enumerate(act):
        ref.direction(rp, probs[b], fsh[a * 2 * nf:(a + 1) * 2 * nf])
    ia = torch.from_numpy(act).long().to(DEV)
    g, hd, dd = st.g[ia, :nf].cpu().numpy(), st.hinv[ia, :nf, :nf].cpu().numpy(), st.d[ia, :nf].cpu().numpy()
    ok = np.array([probs[b].status == ref.RUNNING for b in act])
    assert ok.sum() > 0.6 * n and (~ok).sum() >= 2  # (30 of the 50 of the first shape)
    for a, b in enumerate(act):
        q = probs[b]
        assert int(st.status[b]) == q.status and int(st.flags[b]) == q.flags, (a, b)
        if not ok[a]:
            continue
        np.testing.assert_allclose(g[a], q.g, rtol=1e-13, atol=0)
        scale = np.max(np.abs(q.H))
        np.testing.assert_allclose(hd[a], q.H, rtol=0, atol=1e-13 * scale)
        np.testing.assert_allclose(dd[a], q.d, rtol=0, atol=1e-13 * np.max(np.abs(q.d)))
        assert float(st.gnorm[b]) == pytest.approx(q.gnorm, rel=1e-13)
    # trial rows from the device's direction: the same bits
    tr = trials.cpu().numpy()
    for a, b in enumerate(act):
        q = probs[b]
        q.g, q.d = g[a].copy(), dd[a].copy()
        want = []
        for k in range(K):
            v = u[b].copy()
            for i, c in enumerate(free):
                v[c] = ref.trial_u(u[b, c], q.d[i], k, rp.delta)
            want.append(ref.theta(rp, v))
        np.testing.assert_array_equal(tr[a * K:(a + 1) * K], np.array(want))
    # accept: trial values with a few non-finite ones; u, f, s, g_prev, flags, status, n_iter bit for bit
    ft = -0.5 * (((trials - mu) / sc) ** 2).sum(1)
    ft[5], ft[K * 9] = math.nan, math.inf
    L.check(lib.cf_opt_accept(C.byref(p), C.byref(cs), dact.data_ptr(), n, ft.data_ptr(), stream))
    fth = ft.cpu().numpy()
    for a, b in enumerate(act):
        ref.accept(rp, probs[b], fth[a * K:(a + 1) * K])
    uu, ff, ss, gp = st.u.cpu().numpy(), st.f.cpu().numpy(), st.s.cpu().numpy(), st.g_prev.cpu().numpy()
    for a, b in enumerate(act):
        q = probs[b]
        np.testing.assert_array_equal(uu[b], q.u)
        assert ff[b] == q.f and int(st.status[b]) == q.status and int(st.flags[b]) == q.flags and int(st.n_iter[b]) == q.n_iter
        if q.flags & ref.HAS_PAIR:
            np.testing.assert_array_equal(ss[b, :nf], q.s)
            np.testing.assert_array_equal(gp[b, :nf], q.g_prev)
    # compaction: the still-running problems of the active list, in order
    nxt = torch.empty(B, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.check(lib.cf_opt_compact(dact.data_ptr(), n, st.status.data_ptr(), nxt.data_ptr(), cnt.data_ptr(), stream))
    keep = [b for b in act if probs[b].status == ref.RUNNING]
    assert int(cnt) == len(keep) and nxt[: len(keep)].cpu().tolist() == keep


def test_starts_kernel_against_the_restatement(pkg, opt):
    L, lib = pkg._lib, pkg.lib()
    bounds = np.array([[-1.0, 1.0], [0.1, 0.7], [-9.0, 9.0]])
    p = opt._params(bounds, [0, 2], opt._options(1e-6, 4, 1e-5, None, 10, 1e-4))
    x0 = np.tile([0.5, 0.3, -20.0], (3000, 1))
    u, th = opt._starts(p, x0, opt.opt_key(7), L, lib)
    u, th = u.cpu().numpy(), th.cpu().numpy()
    key = opt.opt_key(7)
    for c in (0, 2):
        want = ref.DELTA + nested_uniform(key, c, np.arange(3000)) * (1.0 - 2.0 * ref.DELTA)
        np.testing.assert_array_equal(u[:, c], want)
    np.testing.assert_array_equal(u[:, 1], np.full(3000, (0.3 - 0.1) / 0.6))
    np.testing.assert_array_equal(th, bounds[:, 0] + u * (bounds[:, 1] - bounds[:, 0]))
    assert np.all((th > bounds[:, 0]) & (th < bounds[:, 1]))
    u2, _ = opt._starts(p, x0, None, L, lib)
    np.testing.assert_array_equal(u2.cpu().numpy()[:, 2], np.full(3000, ref.DELTA))  # clamped into the box


def nested_uniform(key, stream, counter):
    import nested_reference

    return nested_reference.uniform(key, stream, counter)


def test_starts_kernel_with_sixteen_free_coordinates(pkg, opt):
    """ndim = n_free = 16: every coordinate drawn from its own stream, bit for bit the restatement's generator."""
    L, lib = pkg._lib, pkg.lib()
    rng = np.random.default_rng(16)
    lo = rng.uniform(-100.0, 100.0, 16)
    bounds = np.stack([lo, lo + rng.uniform(1e-3, 50.0, 16)], axis=1)
    p = opt._params(bounds, list(range(16)), opt._options(1e-6, 8, 1e-5, None, 10, 1e-4))
    n = 1025
    key = opt.opt_key(16)
    u, th = opt._starts(p, np.zeros((n, 16)), key, L, lib)
    u, th = u.cpu().numpy(), th.cpu().numpy()
    for c in range(16):
        want = ref.DELTA + nested_uniform(key, c, np.arange(n)) * (1.0 - 2.0 * ref.DELTA)
        np.testing.assert_array_equal(u[:, c], want, err_msg=f"coordinate {c}")
    np.testing.assert_array_equal(th, bounds[:, 0] + u * (bounds[:, 1] - bounds[:, 0]))
    assert np.all((u >= ref.DELTA) & (u <= 1 - ref.DELTA))


@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 1023, 1024, 1025, 2048, 5000])
@pytest.mark.parametrize("running", ["random", "all", "none"])
def test_compact_kernel_against_numpy(pkg, opt, n_active, running):
    """cf_opt_compact alone: the still-running entries of the active list in order and their number, for lists shorter and
    longer than the kernel's 1024-entry chunk; `next` is written up to the count and no further."""
    L, lib = pkg._lib, pkg.lib()
    rng = np.random.default_rng(n_active)
    B = 6000
    status = {"random": rng.integers(0, 6, B), "all": np.zeros(B), "none": rng.integers(1, 6, B)}[running].astype(np.int32)
    act = rng.permutation(B)[:n_active].astype(np.int32)
    keep = act[status[act] == ref.RUNNING]
    sentinel = -12345
    nxt = torch.full((n_active + 64,), sentinel, dtype=torch.int32, device=DEV)
    cnt = torch.full((2,), sentinel, dtype=torch.int32, device=DEV)
    dact, dstatus = torch.from_numpy(act).to(DEV), torch.from_numpy(status).to(DEV)
    L.check(lib.cf_opt_compact(dact.data_ptr(), n_active, dstatus.data_ptr(), nxt.data_ptr(), cnt.data_ptr(),
                               torch.cuda.current_stream(DEV).cuda_stream))
    got, count = nxt.cpu().numpy(), cnt.cpu().numpy()
    assert count[0] == keep.size and count[1] == sentinel
    np.testing.assert_array_equal(got[:keep.size], keep)
    np.testing.assert_array_equal(got[keep.size:], np.full(n_active + 64 - keep.size, sentinel))


# ---- 2. analytic problems --------------------------------------------------------------------------------------------
def _gauss6():
    d = 6
    b = np.array([[-2.0, 2.0]] * d)
    a = _corr_precision(d, 1e4, 21) * (10.0 / 16.0)  # u-space Hessian eigenvalues 10 .. 1e5
    mu = np.array([0.3, -0.8, 1.1, 0.0, -1.5, 0.6])
    return b, a, mu


def test_correlated_gaussian_optimum(opt):
    b, a, mu = _gauss6()
    x0 = np.random.default_rng(1).uniform(-1.9, 1.9, (64, 6))
    res = opt.maximize(_quad(mu, a), b, x0, gtol=1e-8, max_iter=500)
    assert np.all(res.converged), res.status_counts()
    u = (res.x - b[:, 0]) / 4.0
    assert np.max(np.abs(u - (mu - b[:, 0]) / 4.0)) <= 1e-7


def test_correlated_gaussian_with_active_bounds(opt):
    b, a, _ = _gauss6()
    mu = np.array([0.3, -2.6, 1.1, 2.9, -1.5, 0.6])  # outside the box in two coordinates
    want = kkt_box_max(mu, a, b[:, 0], b[:, 1])
    x0 = np.random.default_rng(2).uniform(-1.9, 1.9, (32, 6))
    res = opt.maximize(_quad(mu, a), b, x0, gtol=1e-8, max_iter=500)
    assert np.all(res.converged), res.status_counts()
    assert np.max(np.abs((res.x - want) / 4.0)) <= ref.DELTA + 1e-7


def test_rosenbrock_all_starts_converge(opt):
    def rosen(th):
        return -((1.0 - th[:, 0]) ** 2 + 100.0 * (th[:, 1] - th[:, 0] * th[:, 0]) ** 2)

    b = np.array([[-2.0, 2.0], [-2.0, 2.0]])
    fit = opt.best_fit(rosen, b, n_starts=256, seed=3, gtol=1e-7, max_iter=1000)
    res = fit.problems
    assert np.all(res.converged), res.status_counts()
    assert np.max(np.abs((res.x - 1.0) / 4.0)) <= 1e-6


def _gauss4():
    sd = np.array([0.3, 0.5, 0.2, 0.4])
    r = np.array([[1.0, 0.5, -0.3, 0.2], [0.5, 1.0, 0.1, -0.2], [-0.3, 0.1, 1.0, 0.4], [0.2, -0.2, 0.4, 1.0]])  # eigenvalues >= 0.14
    cov = r * np.outer(sd, sd)
    mu = np.array([0.2, -0.3, 0.5, 0.0])
    return np.array([[-4.0, 4.0]] * 4), mu, cov


def test_gaussian_profiles_against_closed_forms(opt):
    b, mu, cov = _gauss4()
    f = _quad(mu, np.linalg.inv(cov))
    best = opt.best_fit(f, b, n_starts=16, seed=1, gtol=1e-9)
    j, grid = 1, np.linspace(mu[1] - 1.5, mu[1] + 1.5, 21)
    pr = opt.profile(f, b, j, grid, best=best, gtol=1e-9)
    want = -0.5 * (grid - mu[j]) ** 2 / cov[j, j]
    np.testing.assert_allclose(pr.values, want, rtol=0, atol=1e-8)
    assert np.all((pr.status == opt.CONVERGED) | (pr.status == opt.NOISE_FLOOR))
    np.testing.assert_allclose(pr.delta_chi2, -2.0 * want, rtol=0, atol=2e-8)
    lo, hi = pr.interval(1.0)
    wlo, whi = opt.crossings(grid, -2.0 * want, 1.0)
    assert lo == pytest.approx(wlo, abs=1e-7) and hi == pytest.approx(whi, abs=1e-7)
    assert pr.problems.status.size == 21 * 8
    # 2-D: the marginal 2 x 2 form on 11 x 11 points
    ij = (0, 2)
    g0, g2 = np.linspace(mu[0] - 0.6, mu[0] + 0.6, 11), np.linspace(mu[2] - 0.4, mu[2] + 0.4, 11)
    pr2 = opt.profile(f, b, ij, (g0, g2), best=best, n_starts=4, gtol=1e-9)
    prec2 = np.linalg.inv(cov[np.ix_(ij, ij)])
    t0, t2 = np.meshgrid(g0 - mu[0], g2 - mu[2], indexing="ij")
    want2 = -0.5 * (prec2[0, 0] * t0 * t0 + 2 * prec2[0, 1] * t0 * t2 + prec2[1, 1] * t2 * t2)
    assert pr2.values.shape == (11, 11)
    np.testing.assert_allclose(pr2.values, want2, rtol=0, atol=1e-8)


# ---- 3. real data ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def union3(pkg, opt):
    g = golden("sn_union3_1")
    box = pkg.likelihoods.SnUnion3.PRIOR_BOX
    lk = pkg.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    yield lk, box, g
    lk.engine.close()


@pytest.fixture(scope="module")
def desi(pkg, opt):
    g = golden("bao_desi")
    lk = pkg.likelihoods.DesiBao(g["bao_z"], g["bao_val"], g["bao_qty"], g["bao_inv_cov"], rd=float(g["rd"]), bounds=g["bounds"])
    yield lk, np.asarray(g["bounds"], dtype=np.float64), g
    lk.engine.close()


def _scipy_fit(logl, box, x0, free):
    """scipy L-BFGS-B on -log L over the free coordinates, central differences, tight tolerances (the host path)."""
    from scipy.optimize import minimize

    free = list(free)
    w = box[free, 1] - box[free, 0]

    def full(z):
        t = np.array(x0, dtype=np.float64)
        t[free] = z
        return t

    def fun(z):
        h = 1e-7 * w
        pts = [full(z)]
        for i in range(len(free)):
            for s in (1.0, -1.0):
                zz = z.copy()
                zz[i] += s * h[i]
                pts.append(full(zz))
        v = logl(np.array(pts))
        return -v[0], -(v[1::2] - v[2::2]) / (2 * h)

    r = minimize(fun, x0=np.asarray(x0, float)[free], jac=True, bounds=box[free], method="L-BFGS-B",
                 options=dict(ftol=1e-15, gtol=1e-10, maxiter=2000, maxcor=20))
    return full(r.x)


def _check_against_cpu(pkg, opt, lk_dev, oracle_lk, box, x0, free=None):
    from oracle import oracle_c as oc

    co = oc.COracle(oracle_lk)
    free = list(range(box.shape[0])) if free is None else free
    res = opt.maximize(lk_dev.engine.torch_log_prob(pkg.CF_OUT_LOGL), box, x0, free=free)
    assert np.all(res.converged), res.status_counts()
    for k in range(x0.shape[0]):
        t_cpu = _scipy_fit(co.logl, box, x0[k], free)
        f_cpu = float(co.logl(t_cpu[None, :])[0])
        assert np.all(np.abs(res.x[k] - t_cpu) <= 1e-5 * (box[:, 1] - box[:, 0])), (k, res.x[k], t_cpu)
        assert res.log_prob[k] >= f_cpu - 1e-8, (k, res.log_prob[k], f_cpu)
    return res


def test_union3_and_desi_against_scipy_on_the_cpu_oracle(pkg, opt, union3, desi):
    from test_oracle_golden import lk_bao_desi, lk_sn_union3_1

    lk, box, g = union3
    x0 = np.array([[0.0, 0.3, -3.0], [0.5, 0.6, 5.0], [-0.5, 0.15, -8.0], [0.1, 0.45, 0.5]])
    _check_against_cpu(pkg, opt, lk, lk_sn_union3_1(g), box, x0)
    lk, box, g = desi
    x0 = np.array([[0.67, 0.31, -0.75], [0.55, 0.2, -0.2], [0.78, 0.45, -0.95], [0.62, 0.35, -0.5]])
    _check_against_cpu(pkg, opt, lk, lk_bao_desi(g), box, x0)
    # three grid points of the w0 profile: w0 held, (h, Om) maximised
    x0 = np.array([[0.67, 0.31, -0.9], [0.6, 0.4, -0.6], [0.7, 0.25, -0.3]] * 1)
    _check_against_cpu(pkg, opt, lk, lk_bao_desi(g), box, x0, free=[0, 1])


def test_union3_published_chi2_and_significance(pkg, opt, union3):
    """sn/union3_1.py:161 gives chi2 (MAP) 22.15 with the velocity step and 2.57 sigma against :145, v = 0: 28.76.  The
    published values are the chi^2 of the best posterior sample, so a true maximum can only be lower, and only slightly.  A
    miss of these bounds alone points at the data of the fixture, not at the optimizer."""
    lk, box, g = union3
    f = lk.engine.torch_log_prob(pkg.CF_OUT_LOGL)
    fit = opt.best_fit(f, box, n_starts=32, seed=0)
    nested = opt.best_fit(f, box, n_starts=32, seed=0, fixed={2: 0.0})
    assert fit.best_converged and nested.best_converged
    assert 22.15 - 0.1 <= fit.chi2 <= 22.155, fit.chi2
    assert 28.76 - 0.1 <= nested.chi2 <= 28.765, nested.chi2
    assert opt.sigma_from_delta_chi2(nested.chi2 - fit.chi2, 1) == pytest.approx(2.57, abs=0.05)
    assert fit.chi2 < float(np.min(g["chi2"][np.isfinite(g["chi2"])]))  # 28.7611: no fixture row is better
    assert nested.x[2] == 0.0 or abs(nested.x[2]) < 1e-15


def test_desi_best_fit_below_the_published_chi2(pkg, opt, desi):
    """bao/desi.py:225 gives chi2 = 8.815 at the posterior median; the maximum lies at or below it and below every fixture row
    (8.8163).  A miss of this bound alone points at the data of the fixture, not at the optimizer."""
    lk, box, g = desi
    fit = opt.best_fit(lk.engine.torch_log_prob(pkg.CF_OUT_LOGL), box, n_starts=32, seed=0)
    assert fit.best_converged
    assert fit.chi2 <= 8.815, fit.chi2
    assert fit.chi2 < float(np.min(g["chi2"][np.isfinite(g["chi2"])]))


# ---- 4. determinism --------------------------------------------------------------------------------------------------
def test_a_problem_has_the_same_bits_in_any_batch(pkg, opt, desi):
    lk, box, _ = desi
    f = lk.engine.torch_log_prob(pkg.CF_OUT_LOGL)
    rng = np.random.default_rng(9)
    x0 = rng.uniform(box[:, 0], box[:, 1], (256, 3))
    alone = opt.maximize(f, box, x0)
    big = np.concatenate([x0, rng.uniform(box[:, 0], box[:, 1], (768, 3))])
    perm = rng.permutation(1024)
    mixed = opt.maximize(f, box, big[perm])
    back = np.empty(1024, dtype=np.int64)
    back[perm] = np.arange(1024)
    pos = back[:256]
    for name in ("x", "log_prob", "status", "n_iter", "grad_norm"):
        np.testing.assert_array_equal(getattr(mixed, name)[pos], getattr(alone, name), err_msg=name)
    for k in range(8):
        one = opt.maximize(f, box, x0[k:k + 1])
        for name in ("x", "log_prob", "status", "n_iter"):
            np.testing.assert_array_equal(getattr(one, name)[0], getattr(alone, name)[k], err_msg=f"{name} {k}")
    a = opt.best_fit(f, box, n_starts=64, seed=5)
    b = opt.best_fit(f, box, n_starts=64, seed=5)
    c = opt.best_fit(f, box, n_starts=64, seed=6)
    for name in ("x0", "x", "log_prob", "status", "n_iter"):
        np.testing.assert_array_equal(getattr(a.problems, name), getattr(b.problems, name))
    assert not np.any(np.all(a.problems.x0 == c.problems.x0, axis=1))


# ---- 5. edge cases ---------------------------------------------------------------------------------------------------
def test_nonfinite_starts_and_stencils_and_the_iteration_cap(opt):
    b, mu, cov = _gauss4()
    g = _quad(mu, np.linalg.inv(cov))

    def f(theta):
        v = g(theta)
        v = torch.where(theta[:, 3] > 3.0, torch.full_like(v, -math.inf), v)  # a region of log P = -inf
        return torch.where((theta[:, 0] > -3.3) & (theta[:, 0] < -3.2), torch.full_like(v, math.nan), v)  # a NaN strip

    rng = np.random.default_rng(4)
    x0 = rng.uniform(-2.0, 2.0, (16, 4))
    x0[3, 3] = 3.5  # starts where log P = -inf
    x0[7] = [-3.25, 0.0, 0.0, 0.0]  # starts in the NaN strip
    res = opt.maximize(f, b, x0)
    assert res.status[3] == opt.NONFINITE_START and res.status[7] == opt.NONFINITE_START
    np.testing.assert_array_equal(res.x[3], res.x0[3])
    assert res.log_prob[3] == -math.inf and res.n_iter[3] == 0
    others = [k for k in range(16) if k not in (3, 7)]
    solo = opt.maximize(f, b, x0[others])
    for name in ("x", "log_prob", "status", "n_iter"):
        np.testing.assert_array_equal(getattr(res, name)[others], getattr(solo, name), err_msg=name)
    # a start next to the NaN strip: its stencil is not finite
    edge = opt.maximize(f, b, np.array([[-3.2 + 1e-7 * 8.0 * 0.5, 0.0, 0.0, 0.0]]))
    assert edge.status[0] == opt.NONFINITE_STENCIL
    capped = opt.maximize(f, b, rng.uniform(-2.0, 2.0, (64, 4)), max_iter=3)
    assert np.all(capped.status != opt.RUNNING) and np.all(capped.n_iter <= 3)
    assert np.any(capped.status == opt.ITER_CAP)
    for r in (res, capped, edge):
        assert not np.any(np.isnan(r.x)) and not np.any(np.isnan(r.log_prob)) and not np.any(np.isnan(r.grad_norm))
