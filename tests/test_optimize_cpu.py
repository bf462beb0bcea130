"""CPU: the optimizer's restated iteration (tests/opt_reference.py) on analytic problems, the random-start keys, argument
validation, profile intervals, the significance convention and the refusal without a GPU -- all without a GPU."""
import ctypes
import math
from ctypes import c_double as C_double
from itertools import product

import numpy as np
import pytest

import opt_reference as ref


@pytest.fixture(scope="module")
def opt(pkg):
    return pkg.optimize


def _gauss(mu, a):
    """f(theta) = -1/2 (theta - mu)^T A (theta - mu) on rows."""
    mu, a = np.asarray(mu, float), np.asarray(a, float)

    def f(th):
        x = np.atleast_2d(th) - mu
        return -0.5 * np.einsum("wi,ij,wj->w", x, a, x)

    return f


def _corr_precision(d, cond, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return q @ np.diag(np.geomspace(1.0, cond, d)) @ q.T


def kkt_box_max(mu, a, lo, hi):
    """Maximiser of -1/2 (x - mu)^T A (x - mu) on [lo, hi] by exhaustive active-set enumeration."""
    d = len(mu)
    best, fbest = None, -math.inf
    for faces in product((None, 0, 1), repeat=d):
        x = np.empty(d)
        fixed = [i for i in range(d) if faces[i] is not None]
        freei = [i for i in range(d) if faces[i] is None]
        for i in fixed:
            x[i] = lo[i] if faces[i] == 0 else hi[i]
        if freei:
            aff, afx = a[np.ix_(freei, freei)], a[np.ix_(freei, fixed)]
            x[freei] = mu[freei] - np.linalg.solve(aff, afx @ (x[fixed] - mu[fixed]))
        if np.all(x >= lo - 1e-15) and np.all(x <= hi + 1e-15):
            f = -0.5 * (x - mu) @ a @ (x - mu)
            if f > fbest:
                best, fbest = x, f
    return best


# ---- the restated iteration ------------------------------------------------------------------------------------------
def test_restatement_reaches_a_correlated_gaussian_optimum():
    d = 4
    a = _corr_precision(d, 1e3, 1) * 50.0
    mu = np.array([0.3, -1.2, 2.0, 0.7])
    b = np.array([[-3.0, 3.0]] * d)
    p = ref.Params(b, gtol=1e-9, max_iter=400)
    for x0 in np.random.default_rng(2).uniform(-2.5, 2.5, (3, d)):
        st = ref.run(p, _gauss(mu, a), x0)
        assert st.status in (ref.CONVERGED, ref.NOISE_FLOOR), st.status
        np.testing.assert_allclose(ref.theta(p, st.u), mu, atol=1e-7 * 6)


def test_restatement_finds_the_kkt_point_with_active_bounds():
    d = 3
    a = _corr_precision(d, 1e2, 3) * 20.0
    mu = np.array([1.4, -0.3, -2.0])  # outside the box in two coordinates
    b = np.array([[-1.0, 1.0]] * d)
    want = kkt_box_max(mu, a, b[:, 0], b[:, 1])
    p = ref.Params(b, gtol=1e-9, max_iter=400)
    st = ref.run(p, _gauss(mu, a), np.zeros(d))
    assert st.status in (ref.CONVERGED, ref.NOISE_FLOOR)
    np.testing.assert_allclose(st.u, (want - b[:, 0]) / (b[:, 1] - b[:, 0]), atol=ref.DELTA + 1e-7)


def test_restatement_solves_rosenbrock():
    def rosen(th):
        th = np.atleast_2d(th)
        return -((1.0 - th[:, 0]) ** 2 + 100.0 * (th[:, 1] - th[:, 0] ** 2) ** 2)

    b = np.array([[-2.0, 2.0], [-2.0, 2.0]])
    p = ref.Params(b, gtol=1e-7, max_iter=1000)
    for x0 in np.random.default_rng(4).uniform(-1.9, 1.9, (6, 2)):
        st = ref.run(p, rosen, x0)
        assert st.status in (ref.CONVERGED, ref.NOISE_FLOOR), (x0, st.status, st.n_iter)
        np.testing.assert_allclose(st.u, [0.75, 0.75], atol=1e-6)


def test_restatement_holds_fixed_coordinates_and_one_sided_stencils():
    p = ref.Params(np.array([[0.0, 1.0]] * 3), free=[0, 2])
    st = ref.Problem(p, np.array([ref.DELTA, 0.4, 1.0 - ref.DELTA]), -1.0)
    rows = ref.stencil(p, st)
    assert st.form.tolist() == [1, -1]
    assert np.all(rows[:, 1] == 0.4)  # the fixed coordinate never moves
    assert np.all((rows > 0.0) & (rows < 1.0))


# ---- keys ------------------------------------------------------------------------------------------------------------
def test_opt_key_differs_from_every_ensemble_and_nested_key(pkg, opt):
    from importlib import import_module

    ens, ns = pkg.ensemble, import_module(pkg.__name__ + ".nested")
    for seed in range(4):
        for a in range(4):
            k = opt.opt_key(seed, a)
            assert k != opt.opt_key(seed, a + 1) and k != opt.opt_key(seed + 1, a)
            for b in range(4):
                assert k != ns.ns_key(seed, a, b)
                for half in range(3):
                    for stream in (0, 1, 2):
                        assert k != ens.stream_key(seed, a, half, stream)
                        assert k != ens.stream_key(seed, b, half, stream)


# ---- validation and the refusal ---------------------------------------------------------------------------------------
def _f(theta):
    return -(theta**2).sum(1)


def test_arguments_are_validated_before_the_device_check(opt):
    b = np.array([[-1.0, 1.0], [0.0, 2.0], [5.0, 9.0]])
    with pytest.raises(ValueError, match="strictly inside"):
        opt.profile(_f, b, 1, np.linspace(0.0, 1.0, 5))  # 0.0 sits on the face
    with pytest.raises(ValueError, match="strictly inside"):
        opt.profile(_f, b, 2, [6.0, 9.5])
    with pytest.raises(ValueError, match="strictly inside"):
        opt.profile(_f, b, (0, 2), (np.linspace(-0.5, 0.5, 3), np.array([4.0, 6.0])))
    with pytest.raises(ValueError, match="out of range"):
        opt.profile(_f, b, 3, [0.5])
    with pytest.raises(ValueError, match="out of range"):
        opt.best_fit(_f, b, fixed={-1: 0.0})
    with pytest.raises(ValueError, match="out of range"):
        opt.maximize(_f, b, np.zeros((2, 3)), free=[0, 7])
    with pytest.raises(ValueError, match="at most 16"):
        opt.maximize(_f, np.array([[0.0, 1.0]] * 17), np.full((1, 17), 0.5))
    with pytest.raises(ValueError, match=r"x0 must be \[B, 3\]"):
        opt.maximize(_f, b, np.zeros((2, 2)))
    with pytest.raises(ValueError, match="n_trials"):
        opt.maximize(_f, b, np.zeros((1, 3)), n_trials=9)
    with pytest.raises(ValueError, match="nothing to maximise"):
        opt.best_fit(_f, b, fixed={0: 0.0, 1: 1.0, 2: 7.0})


def test_refuses_without_a_gpu(pkg, opt):
    if pkg.lib().cf_device_count() > 0:
        pytest.skip("a GPU is visible")
    b = np.array([[-1.0, 1.0], [0.0, 2.0]])
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_NO_DEVICE"):
        opt.maximize(_f, b, np.zeros((1, 2)))
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_NO_DEVICE"):
        opt.best_fit(_f, b)
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_NO_DEVICE"):
        opt.profile(_f, b, 0, [0.0, 0.5])


def test_kernel_entry_points_validate_their_arguments(pkg):
    L, lib = pkg._lib, pkg.lib()
    p = L.cf_opt_params()
    p.ndim, p.n_free, p.h, p.delta, p.c1, p.n_trials, p.max_iter = 2, 1, 1e-6, 2.0**-40, 1e-4, 4, 10
    p.free_idx[0], p.width[0], p.width[1] = 1, 1.0, 1.0
    buf = (C_double * 8)()
    st = L.cf_opt_state()
    with pytest.raises(pkg.CosmofitError, match="null state"):
        L.check(lib.cf_opt_stencil(ctypes.byref(p), ctypes.byref(st), ctypes.cast(buf, ctypes.c_void_p), 1,
                                   ctypes.cast(buf, ctypes.c_void_p), None))
    p.n_trials = 9
    with pytest.raises(pkg.CosmofitError, match="n_trials"):
        L.check(lib.cf_opt_starts(ctypes.byref(p), 1, ctypes.cast(buf, ctypes.c_void_p), 0, 1, ctypes.cast(buf, ctypes.c_void_p),
                                  ctypes.cast(buf, ctypes.c_void_p), None))
    p.n_trials, p.free_idx[0] = 4, 2
    with pytest.raises(pkg.CosmofitError, match="free_idx"):
        L.check(lib.cf_opt_starts(ctypes.byref(p), 1, ctypes.cast(buf, ctypes.c_void_p), 0, 1, ctypes.cast(buf, ctypes.c_void_p),
                                  ctypes.cast(buf, ctypes.c_void_p), None))



# ---- intervals and significance ----------------------------------------------------------------------------------------
def test_interval_on_hand_made_profiles(opt):
    x = np.linspace(-2.0, 2.0, 9)  # step 0.5
    d = x**2  # crosses 1 exactly at the grid points -1, 1
    assert opt.crossings(x, d, 1.0) == (-1.0, 1.0)
    d2 = (x - 0.1) ** 2 * 4.0
    lo, hi = opt.crossings(x, d2, 1.0)
    # linear interpolation between (-0.5, 1.44) and (0, 0.04), and between (0.5, 0.64) and (1.0, 3.24)
    assert lo == pytest.approx(-0.5 + (1.0 - 1.44) * 0.5 / (0.04 - 1.44), rel=1e-15)
    assert hi == pytest.approx(0.5 + (1.0 - 0.64) * 0.5 / (3.24 - 0.64), rel=1e-15)
    # truncated by the prior on the left: the minimum sits at the first grid point
    dt = (x + 2.0) ** 2 / 2.0
    lo, hi = opt.crossings(x, dt, 1.0)
    assert lo is None and hi == pytest.approx(-1.0 + (1.0 - 0.5) * 0.5 / (1.125 - 0.5), rel=1e-15)
    assert opt.crossings(x, np.zeros_like(x), 1.0) == (None, None)
    res = opt.ProfileResult(index=(0,), grid=(x,), values=-0.5 * d2, x=None, status=None, delta_chi2=d2, log_prob_max=0.0,
                            best=None, problems=None)
    assert res.interval() == opt.crossings(x, d2, 1.0)
    with pytest.raises(ValueError):
        opt.ProfileResult(index=(0, 1), grid=(x, x), values=None, x=None, status=None, delta_chi2=None, log_prob_max=0.0,
                          best=None, problems=None).interval()


def test_sigma_from_delta_chi2(opt):
    from scipy import stats

    assert opt.sigma_from_delta_chi2(6.61, 1) == math.sqrt(6.61)
    assert opt.sigma_from_delta_chi2(28.76 - 22.15, 1) == pytest.approx(2.57, abs=0.005)  # sn/union3_1.py:161
    assert opt.sigma_from_delta_chi2(0.0, 2) == 0.0 and opt.sigma_from_delta_chi2(-1.0, 1) == 0.0
    s2 = opt.sigma_from_delta_chi2(6.0, 2)
    assert stats.norm.sf(s2) * 2 == pytest.approx(stats.chi2.sf(6.0, 2), rel=1e-10)
    assert s2 < math.sqrt(6.0)
