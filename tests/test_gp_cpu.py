"""CPU (-m "not gpu"): the judge of the Gaussian-process tests and everything of the feature that needs no GPU.

* The long-double restatement (tests/gp_reference.py) against scipy's float64 Cholesky path on the very draws the GPU tests
  use: within 1e-11, so the 1e-10 bar of the GPU tests has a factor >= 10 of room before a GPU is involved.
* The restatement against the defining identities.
* cf_gp_create's argument validation (it comes before the first HIP call).
* ``gp.HubbleGP``: normalisation, ``physical`` round trips, n = 1, the loud error without a GPU, and the mixture moments of
  ``marginal_predict`` on host tensors through a stand-in for the device launch."""
import ctypes as C

import numpy as np
import pytest

import gp_reference as R
import gp_shapes as GS

LD = R.LD
SCIPY_BAR = 1e-11


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GS.N_SET)
def test_restatement_matches_scipy_on_the_gpu_tests_draws(n):
    z, y, Cm = GS.data(n)[:3]
    mll, pred = GS.reference(n)
    worst_mll, worst_pred = 0.0, np.zeros(5)
    for i, t in enumerate(GS.base_thetas(n)):
        s = R.scipy_mll_parts(z, y, Cm, t)
        worst_mll = max(worst_mll, max(float(abs((LD(s[k]) - mll[i, k]) / mll[i, k])) for k in range(3)))
        sp = R.scipy_predict(z, y, Cm, t, GS.z_star_full(n), GS.TEST_NOISE)
        worst_pred = np.maximum(worst_pred, R.scaled_errors(sp, pred[i], t).astype(np.float64))
    print(f"n={n}: scipy vs restatement, log ML and parts rel {worst_mll:.2e}, predictions scaled {worst_pred.max():.2e}")
    assert worst_mll < SCIPY_BAR
    assert worst_pred.max() < SCIPY_BAR


@pytest.mark.parametrize("n", (2, 17, 38))
def test_restatement_quadratic_form_and_logdet_by_other_routes(n):
    z, y, Cm = GS.data(n)[:3]
    for t in GS.base_thetas(n)[:8]:
        K = R.kernel_matrix(z, Cm, t).astype(np.float64)
        r = y - t[0]
        _, quad, logdet = R.mll_parts(z, y, Cm, t)
        assert float(quad) == pytest.approx(float(r @ np.linalg.solve(K, r)), rel=1e-9)
        assert float(logdet) == pytest.approx(np.linalg.slogdet(K)[1], rel=1e-9, abs=1e-9)
        Lw = R.cholesky(K)
        assert float(np.max(np.abs(Lw @ Lw.T - K))) < 1e-17 * float(np.max(np.abs(K))) * n * 8


def test_restatement_mean_interpolates_the_data_as_the_noise_vanishes():
    z, y, Cm = GS.data(17)[:3]
    t = GS.base_thetas(17)[3].copy()
    t[2] = 0.02  # shorter than the spacing of the data: the RBF part is well conditioned on its own
    errs = []
    for s in (1e-2, 1e-4, 1e-6):
        t[3] = s
        errs.append(float(np.max(np.abs(R.predict(z, y, Cm, t, z)[:, 0] - y))))
    assert errs[0] > errs[1] > errs[2] and errs[2] < 1e-3


@pytest.mark.parametrize("n", (1, 17, 38))
def test_restatement_derivative_quantities_against_central_differences(n):
    """dmean = d mean / dz*; cov(f, f') = 1/2 d var / dz*; dvar = the mixed second derivative of the posterior covariance,
    checked through var(f(z + h) - f(z - h)) = 4 h^2 dvar + O(h^4) with the posterior covariance of the two points."""
    z, y, Cm = GS.data(n)[:3]
    t = GS.base_thetas(n)[5]
    zs = np.array([0.0, 0.37, float(z[0]), 1.1, 2.2], dtype=LD)
    h = LD(1e-4)
    p0, pp, pm = (R.predict(z, y, Cm, t, zs + d) for d in (LD(0), h, -h))
    sc = R.predict_scales(t, p0)
    assert float(np.max(np.abs((pp[:, 0] - pm[:, 0]) / (2 * h) - p0[:, 2])) / sc[2]) < 1e-7
    assert float(np.max(np.abs((pp[:, 1] - pm[:, 1]) / (4 * h) - p0[:, 4])) / sc[4]) < 1e-7
    # cov(f(a), f(b)) of the posterior, from the same pieces
    m, sf2, ell, s = (LD(v) for v in t)
    Lw = R.cholesky(R.kernel_matrix(z, Cm, t))
    zl = np.asarray(z, dtype=LD)
    k = lambda a: sf2 * np.exp(-((zl[:, None] - a[None, :]) ** 2) / (2 * ell * ell))
    va, vb = R.forward(Lw, k(zs + h)), R.forward(Lw, k(zs - h))
    cab = sf2 * np.exp(-((2 * h) ** 2) / (2 * ell * ell)) - np.sum(va * vb, axis=0)
    var_diff = pp[:, 1] + pm[:, 1] - 2 * cab  # both carry no test noise here
    assert float(np.max(np.abs(var_diff / (4 * h * h) - p0[:, 3])) / sc[3]) < 1e-5


def test_mixture_of_identical_components_is_the_component_and_spreads_add():
    z, y, Cm = GS.data(17)[:3]
    zs = GS.z_star(17, 9)
    p = np.array([R.predict(z, y, Cm, t, zs) for t in GS.base_thetas(17)[:6]])
    same = R.mixture(np.repeat(p[:1], 4, axis=0))
    assert float(np.max(np.abs(same - p[0]))) < 1e-17
    mix = R.mixture(p)
    assert np.all(mix[:, 1] >= np.mean(p[:, :, 1], axis=0) - 1e-18)  # the spread of the means only adds variance
    w = np.array([0, 0, 1.0, 0, 0, 0])
    assert float(np.max(np.abs(R.mixture(p, w) - p[2]))) < 1e-17


# ---- cf_gp_create ------------------------------------------------------------------------------------------------------
def _create(pkg, n, z=None, y=None, cov=None, bounds=None, null=None):
    L = pkg._lib
    m = max(n, 1)
    z = np.linspace(0.1, 1.9, m) if z is None else z
    y = np.zeros(m) if y is None else y
    cov = np.eye(m) if cov is None else cov
    bounds = GS.default_bounds(2.0) if bounds is None else bounds
    arrs = dict(z=np.ascontiguousarray(z, dtype=np.float64), y=np.ascontiguousarray(y, dtype=np.float64),
                cov=np.ascontiguousarray(cov, dtype=np.float64), bounds=np.ascontiguousarray(bounds, dtype=np.float64))
    d = L.cf_gp_desc()
    d.struct_size, d.device, d.n = C.sizeof(L.cf_gp_desc), 0, n
    for k, a in arrs.items():
        setattr(d, k, None if k == null else a.ctypes.data)
    h = C.c_void_p()
    rc = pkg.lib().cf_gp_create(C.byref(d), C.byref(h))
    if rc == 0:
        pkg.lib().cf_gp_destroy(h)
    return rc, pkg.lib().cf_last_error().decode()


def test_create_validates_before_it_touches_the_device(pkg):
    cases = [
        (dict(n=0), "n = 0 is outside 1..64"),
        (dict(n=65, z=np.linspace(0.1, 1.9, 65), y=np.zeros(65), cov=np.eye(65)), "n = 65 is outside 1..64"),
        (dict(n=3, null="cov"), "null data pointer"),
        (dict(n=3, null="z"), "null data pointer"),
        (dict(n=3, y=np.array([0.0, np.nan, 1.0])), "y has a non-finite entry"),
        (dict(n=3, z=np.array([0.0, np.inf, 1.0])), "z has a non-finite entry"),
        (dict(n=3, cov=np.array([[1.0, 0.1, 0.0], [0.1 + 1e-9, 1.0, 0.0], [0.0, 0.0, 1.0]])), "cov is not symmetric at (1, 0)"),
        (dict(n=3, bounds=np.array([[-2, 2], [0.05, 20], [2.0, 1.0], [0.05, 4]])), "bounds[2] must be finite with lo < hi"),
        (dict(n=3, bounds=np.array([[-2, 2], [-0.05, 20], [2.0, 6.0], [0.05, 4]])), "bounds[1] must have lo >= 0"),
    ]
    for kw, msg in cases:
        rc, err = _create(pkg, **kw)
        assert rc == -1, (kw, rc, err)
        assert msg in err, (msg, err)
    assert pkg.lib().cf_gp_create(None, None) == -1
    # a symmetric matrix to rounding is accepted as far as validation goes: what is left is the device
    cov = np.eye(3)
    cov[1, 0], cov[0, 1] = 0.1, 0.1 * (1 + 1e-14)
    rc, err = _create(pkg, 3, cov=cov)
    assert rc == (0 if pkg.lib().cf_device_count() > 0 else -2), err


def test_row_entry_points_validate_their_arguments(pkg):
    lib = pkg.lib()
    assert lib.cf_gp_mll(None, None, 1, None, None) == -1 and b"null" in lib.cf_last_error()
    assert lib.cf_gp_predict_device(None, None, 1, None, 1, 0.0, None, None) == -1
    i = pkg._lib.cf_gp_info()
    assert lib.cf_gp_get_info(None, C.byref(i)) == -1
    lib.cf_gp_destroy(None)


# ---- HubbleGP ----------------------------------------------------------------------------------------------------------
def test_hubble_gp_normalises_as_the_script_and_round_trips(pkg):
    z, H, cov = GS.raw_data(38)
    g = pkg.gp.HubbleGP(z, H, cov)
    assert g.n == 38 and g.h_mean == pytest.approx(np.mean(H), rel=1e-15) and g.h_std == pytest.approx(np.std(H), rel=1e-15)
    assert np.allclose(g.y, (H - np.mean(H)) / np.std(H), rtol=0, atol=1e-15)
    assert np.allclose(g.cov, cov / np.std(H) ** 2, rtol=1e-15, atol=0)
    assert np.array_equal(g.bounds, GS.default_bounds(z.max()))
    assert g.log_norm == pytest.approx(38 * np.log(np.std(H)), rel=1e-15)
    th = GS.base_thetas(38)[:5]
    ph = g.physical(th)
    assert np.allclose(ph[:, 0], th[:, 0] * g.h_std + g.h_mean) and np.allclose(ph[:, 1], th[:, 1] * g.h_std**2)
    assert np.array_equal(ph[:, 2:], th[:, 2:])
    assert np.allclose(g.normalised(ph), th, rtol=1e-13, atol=1e-13)
    assert g.physical(th[0]).shape == (4,)
    raw = pkg.gp.HubbleGP(z, H, cov, normalise=False, bounds=GS.default_bounds(2.0))
    assert raw.h_mean == 0.0 and raw.h_std == 1.0 and np.array_equal(raw.y, H) and raw.log_norm == 0.0
    with pytest.raises(ValueError, match="shapes disagree"):
        pkg.gp.HubbleGP(z, H[:-1], cov)
    with pytest.raises(ValueError, match="bounds must be"):
        pkg.gp.HubbleGP(z, H, cov, bounds=np.zeros((3, 2)))
    with pytest.raises(pkg.CosmofitError, match="not symmetric"):
        bad = cov.copy()
        bad[3, 1] *= 1.001
        pkg.gp.HubbleGP(z, H, bad)


def test_hubble_gp_single_point_normalises_by_one(pkg):
    g = pkg.gp.HubbleGP([0.5], [90.0], [[25.0]])
    assert g.n == 1 and g.h_mean == 90.0 and g.h_std == 1.0 and g.y[0] == 0.0 and g.cov[0, 0] == 25.0 and g.log_norm == 0.0
    assert np.array_equal(g.bounds[2], [0.5, 1.5])
    with pytest.raises(ValueError, match="max z > 0"):
        pkg.gp.HubbleGP([0.0], [70.0], [[25.0]])


def test_hubble_gp_without_a_gpu_raises_and_never_falls_back(pkg):
    if pkg.lib().cf_device_count() > 0:
        pytest.skip("a GPU is visible")
    import torch

    z, H, cov = GS.raw_data(17)
    g = pkg.gp.HubbleGP(z, H, cov)
    th = GS.base_thetas(17)[0]
    for call in (g.torch_log_prob, lambda: g.log_marginal_likelihood(th), lambda: g.predict(th, [0.0, 1.0]), g.fit, g.info,
                 lambda: g.marginal_predict(torch.zeros((3, 4), dtype=torch.float64), [0.0])):
        with pytest.raises(pkg.CosmofitError, match="CF_ERR_NO_DEVICE"):
            call()


def test_marginal_predict_mixture_moments_on_host_tensors(pkg, monkeypatch):
    """The chunking and the moments of ``marginal_predict`` with the restatement standing in for the device launch: every
    chunk size gives the restatement's mixture, weighted and unweighted, and H0 is the z* = 0 row."""
    import torch

    n = 17
    z, H, cov = GS.raw_data(n)
    g = pkg.gp.HubbleGP(z, H, cov)
    zs = GS.z_star(n, 9)
    S = 23
    th = GS.thetas(n, S)
    _, pred = GS.reference(n)
    table = pred[GS.row_index(S)][:, :9, :].astype(np.float64)  # [S, 9, 5] at TEST_NOISE
    calls = []

    def fake(self, x, zd, noise):
        assert noise == GS.TEST_NOISE
        rows = [int(np.nonzero((th == r.numpy()).all(axis=1))[0][0]) for r in x]
        cols = [int(np.nonzero(zs == v)[0][0]) for v in zd.numpy()]
        calls.append(len(rows))
        return torch.from_numpy(np.ascontiguousarray(table[rows][:, cols]))

    monkeypatch.setattr(pkg.gp.HubbleGP, "_predict_rows", fake)
    x = torch.from_numpy(th)
    w = np.random.default_rng(5).uniform(0.0, 1.0, S)
    w[4] = 0.0
    for weights in (None, w):
        want = R.mixture(table, weights)
        for max_bytes in (2**28, 9 * 40 * 5, 1):
            calls.clear()
            got = g.marginal_predict(x, zs, weights=None if weights is None else torch.from_numpy(weights), noise=GS.TEST_NOISE,
                                     max_bytes=max_bytes)
            assert sum(calls) == S and max(calls) == pkg.gp.marginal_chunk(S, 9, max_bytes)
            s = LD(g.h_std)
            assert np.allclose(got["mean"], np.asarray(want[:, 0] * s + LD(g.h_mean), dtype=np.float64), rtol=1e-13)
            assert np.allclose(got["std"], np.asarray(np.sqrt(want[:, 1]) * s, dtype=np.float64), rtol=1e-11)
            assert np.allclose(got["dmean"], np.asarray(want[:, 2] * s, dtype=np.float64), rtol=1e-11, atol=1e-12)
            assert np.allclose(got["dstd"], np.asarray(np.sqrt(want[:, 3]) * s, dtype=np.float64), rtol=1e-11)
            assert np.allclose(got["cov_fd"], np.asarray(want[:, 4] * s * s, dtype=np.float64), rtol=1e-9, atol=1e-11)
            assert np.allclose(got["q"], -1 + (1 + zs) * got["dmean"] / got["mean"], rtol=1e-14)
            assert zs[0] == 0.0 and got["H0"] == (got["mean"][0], got["std"][0])
    assert pkg.gp.marginal_chunk(23, 9, 1) == 1 and pkg.gp.marginal_chunk(23, 9, 9 * 40 * 5) == 5
    assert g.marginal_predict(x, zs[1:], noise=GS.TEST_NOISE)["H0"] is None
    with pytest.raises(ValueError, match="weights"):
        g.marginal_predict(x, zs, weights=torch.full((S,), -1.0, dtype=torch.float64), noise=GS.TEST_NOISE)
    with pytest.raises(ValueError, match="samples"):
        g.marginal_predict(x.float(), zs)


def test_log_prob_callable_keeps_the_gp_alive_and_sees_a_closed_one(pkg, monkeypatch):
    """What a sampler holds is the callable alone: it must keep the GP (whose ``__del__`` frees the device buffers) alive, and
    after ``close()`` it must raise before anything is launched.  A stand-in handle takes the place of the device's here."""
    import gc
    import weakref

    import torch

    destroyed = []
    monkeypatch.setattr(pkg.lib(), "cf_gp_destroy", lambda h: destroyed.append(h))
    z, H, cov = GS.raw_data(17)

    def make():
        g = pkg.gp.HubbleGP(z, H, cov)
        if g._h is None:  # no GPU here: a handle that is never dereferenced (the checks below all come before a launch)
            g._h, g._no_device = C.c_void_p(1), None
        return g.torch_log_prob(), weakref.ref(g)

    f, ref = make()
    gc.collect()
    assert ref() is not None and not destroyed, "the callable must hold the GP it evaluates"
    with pytest.raises(ValueError, match="on the GP's GPU"):
        f(torch.zeros((3, 4), dtype=torch.float64))  # a host tensor is refused, not evaluated
    ref().close()
    assert len(destroyed) == 1
    with pytest.raises(pkg.CosmofitError, match="has been closed"):
        f(torch.zeros((3, 4), dtype=torch.float64))
    with pytest.raises(pkg.CosmofitError, match="has been closed"):
        ref().torch_log_prob()
    del f
    gc.collect()
    assert ref() is None and len(destroyed) == 1  # collected with its last holder, and not destroyed twice
