"""GPU (-m gpu): the four entry points of csrc/cosmofit_bridge.hip called directly on torch buffers, as evidence.py calls them.
The judge is the long-double restatement tests/bridge_reference.py.

Bars.  z and theta: 1e-12 of the row's scale, where the scale is the a-priori size of the quantities the row's arithmetic
passes through (|R^-1| (|phi| + |mu|) + 1 for the substitution; |lo| + |hi| + width (1 + |mu| + |R| |z|) for the way back).
log J: 1e-12 of the sum of |terms|.  The round trip: 1e-12 of the box width.  Draws: 1e-14 absolute (|z| <= 8.6 and the device
log / cos are good to a few ulp).  The solve: log r within 1e-12 of the restatement run with the same tol = 1e-13 and the same
stopping rule, the four moments 1e-10 relative, f2 1e-12 of its bound 1 / s2.  A variance is a sum of squared deviations, each
deviation known to delta = 8 ulp of the mean (the exp, the division and the product behind every f), so where the f are equal
to within rounding a relative bar alone asks for digits no float64 sum holds (n1 = 2 with a diverging r: both f2 = 1 / s2 to
1e-54, variance 1e-38 in long double, 5e-32 in float64): the variances are held to 1e-10 var + 2 delta sqrt(var) + delta^2,
which is the relative bar wherever sqrt(var) / mean exceeds 4e-5.  What the fixed order of summation and the
row-per-thread kernels promise is asserted exactly: the same bits alone, at any position, repeated, and on a second stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import bridge_reference as BR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
SENTINEL = -7.25e300
PAD = 32
NDIMS = [1, 2, 3, 8, 16]
NS = [1, 2, 63, 64, 65, 257, 2049]
SOLVE_NS = [1, 2, 2047, 2048, 2049, 4097]


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type"
    return pkg._lib, pkg.lib()


def _dp(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _stream(stream):
    return torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream.cuda_stream


def _out(n, d):
    return (torch.full((n * d + PAD,), SENTINEL, dtype=torch.float64, device=DEV),
            torch.full((n + PAD,), SENTINEL, dtype=torch.float64, device=DEV))


def _take(a, b, n, d, what):
    torch.cuda.synchronize(DEV)  # also the side stream's work
    assert bool((a[n * d:] == SENTINEL).all()) and bool((b[n:] == SENTINEL).all()), f"{what} wrote past its rows"
    return a[:n * d].reshape(n, d).cpu().numpy(), b[:n].cpu().numpy()


def _forward(lib, theta, g, stream=None):
    L, so = lib
    n, d = theta.shape
    z, lj = _out(n, d)
    src = _dev(theta)  # held until the results have been read
    torch.cuda.synchronize(DEV)
    L.check(so.cf_bridge_forward(src.data_ptr(), n, d, _dp(g["lo"]), _dp(g["hi"]), _dp(g["mean"]), _dp(g["chol"]),
                                 z.data_ptr(), lj.data_ptr(), _stream(stream)))
    return _take(z, lj, n, d, "cf_bridge_forward")


def _points(lib, z, g, mirror=0, stream=None):
    L, so = lib
    n, d = z.shape
    th, lj = _out(n, d)
    src = _dev(z)  # held until the results have been read
    torch.cuda.synchronize(DEV)
    L.check(so.cf_bridge_points(src.data_ptr(), n, d, _dp(g["lo"]), _dp(g["hi"]), _dp(g["mean"]), _dp(g["chol"]), mirror,
                                th.data_ptr(), lj.data_ptr(), _stream(stream)))
    return _take(th, lj, n, d, "cf_bridge_points")


def geometry(d, seed=0):
    """A box of mixed widths and offsets, a proposal mean of a few units and a well-conditioned lower factor with garbage
    above the diagonal (never read)."""
    rng = np.random.default_rng([seed, d])
    unit = 10.0 ** rng.integers(-2, 3, d)  # offset and width of one size, so that 1e-12 of a width is many ulp of a face
    lo = rng.uniform(-3.0, 3.0, d) * unit
    hi = lo + rng.uniform(0.5, 2.0, d) * unit
    chol = np.tril(rng.uniform(-0.4, 0.4, (d, d)) / d, -1) + np.diag(rng.uniform(0.5, 2.0, d)) + np.triu(np.full((d, d), 1e300), 1)
    return dict(lo=lo, hi=hi, mean=rng.uniform(-2.0, 2.0, d), chol=np.ascontiguousarray(chol))


def thetas(g, n, seed=1):
    rng = np.random.default_rng([seed, n, g["lo"].size])
    u = rng.uniform(0.0, 1.0, (n, g["lo"].size))
    u[::5] = u[::5] ** 8          # rows that hug the lower faces
    u[1::7] = 1.0 - u[1::7] ** 8  # and the upper ones
    th = g["lo"] + (g["hi"] - g["lo"]) * np.clip(u, 1e-12, 1.0 - 1e-12)
    return th


def _z_scale(theta, g):
    """|R^-1| (|phi| + |mu|) + 1 per row, its largest component."""
    R = np.tril(g["chol"]).astype(LD)
    rinv = np.abs(BR.mr.lower_inverse(R))
    w = g["hi"].astype(LD) - g["lo"].astype(LD)
    phi = np.abs(np.log((theta.astype(LD) - g["lo"].astype(LD)) / w) - np.log((g["hi"].astype(LD) - theta.astype(LD)) / w))
    return ((phi + np.abs(g["mean"]).astype(LD)) @ rinv.T).max(axis=1) + 1


def _theta_scale(z, g):
    w = g["hi"] - g["lo"]
    return np.abs(g["lo"]) + np.abs(g["hi"]) + w * (1 + np.abs(g["mean"]) + np.abs(z) @ np.abs(np.tril(g["chol"])).T)


# ---- forward / points -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", NDIMS)
def test_forward_points_and_the_round_trip(lib, d, n):
    g = geometry(d)
    th = thetas(g, n)
    z, lj = _forward(lib, th, g)
    zr, ljr, mag = BR.forward(th, g["lo"], g["hi"], g["mean"], g["chol"])
    ez = float(np.max(np.abs(z.astype(LD) - zr).max(axis=1) / _z_scale(th, g)))
    el = float(np.max(np.abs(lj.astype(LD) - ljr) / mag))
    assert np.isfinite(z).all() and np.isfinite(lj).all()
    back, ljb = _points(lib, z, g, 0)
    br, ljbr, magb = BR.points(z, g["lo"], g["hi"], g["mean"], g["chol"], 0)
    et = float(np.max(np.abs(back.astype(LD) - br) / _theta_scale(z, g)))
    elb = float(np.max(np.abs(ljb.astype(LD) - ljbr) / magb))
    trip = float(np.max(np.abs(back - th) / (g["hi"] - g["lo"])))
    mir, ljm = _points(lib, z, g, 1)
    mr_, ljmr, magm = BR.points(z, g["lo"], g["hi"], g["mean"], g["chol"], 1)
    em = float(np.max(np.abs(mir.astype(LD) - mr_) / _theta_scale(z, g)))
    elm = float(np.max(np.abs(ljm.astype(LD) - ljmr) / magm))
    print(f"d = {d}, n = {n}: z {ez:.2e}, log J {el:.2e}, theta {et:.2e}, its log J {elb:.2e}, round trip {trip:.2e}, mirror {em:.2e} "
          f"/ {elm:.2e}  (bar 1e-12)")
    assert max(ez, el, et, elb, trip, em, elm) <= 1e-12
    if d > 1 or n > 1:
        assert not np.array_equal(mir, back)


@pytest.mark.parametrize("d", NDIMS)
def test_large_phi_gives_a_finite_jacobian_and_may_reach_a_face(lib, d):
    g = geometry(d, seed=2)
    R = np.tril(g["chol"]).astype(LD)
    rng = np.random.default_rng(d)
    phi = rng.uniform(-5, 5, (12, d))
    phi[0], phi[1], phi[2, 0], phi[3, -1], phi[4], phi[5] = 40.0, -40.0, 39.0, -37.5, 36.8, -36.8
    z = BR.solve_lower(R, phi.astype(LD) - g["mean"].astype(LD)).astype(np.float64)
    th, lj = _points(lib, z, g, 0)
    tr, ljr, mag = BR.points(z, g["lo"], g["hi"], g["mean"], g["chol"], 0)
    assert np.isfinite(lj).all() and np.isfinite(th).all()
    assert np.all(th >= g["lo"]) and np.all(th <= g["hi"])
    w = g["hi"] - g["lo"]
    assert np.all(g["hi"] - th[0] <= 1e-17 * w) and np.all(th[1] - g["lo"] <= 1e-17 * w), "|phi| = 40: theta is the face to 1e-17 widths"
    faces = int(np.sum(th == g["hi"]) + np.sum(th == g["lo"]))
    print(f"d = {d}: {faces} coordinates equal a face")
    assert faces >= 1
    assert float(np.max(np.abs(lj.astype(LD) - ljr) / mag)) <= 1e-12
    assert float(np.max(np.abs(th.astype(LD) - tr) / _theta_scale(z, g))) <= 1e-12
    thm, ljm = _points(lib, -z, g, 1)  # mean - R (-z) is mean + R z
    assert np.array_equal(thm, th) and np.array_equal(ljm, lj)


@pytest.mark.parametrize("d", NDIMS)
def test_rows_outside_give_nan_in_that_row_only_and_rows_do_not_see_each_other(lib, d):
    g = geometry(d, seed=3)
    n = 257
    th = thetas(g, n, seed=4)
    clean_z, clean_lj = _forward(lib, th, g)
    bad = th.copy()
    k = d - 1
    bad[3, 0], bad[64, k], bad[65, 0], bad[130, k], bad[200, 0], bad[256, k] = (g["lo"][0], g["hi"][k], g["lo"][0] - 1.0,
                                                                              np.inf, np.nan, np.nextafter(g["hi"][k], np.inf))
    rows = [3, 64, 65, 130, 200, 256]
    z, lj = _forward(lib, bad, g)
    keep = np.setdiff1d(np.arange(n), rows)
    assert np.isnan(z[rows]).all() and np.isnan(lj[rows]).all()
    assert np.array_equal(z[keep], clean_z[keep]) and np.array_equal(lj[keep], clean_lj[keep])
    zr, ljr, _ = BR.forward(bad, g["lo"], g["hi"], g["mean"], g["chol"])
    assert np.array_equal(np.isnan(zr), np.isnan(z)) and np.array_equal(np.isnan(ljr), np.isnan(lj))
    # every row alone has the bits it has at its position of the 257-row call
    back, ljb = _points(lib, clean_z, g, 0)
    mir, ljm = _points(lib, clean_z, g, 1)
    for i in (0, 1, 62, 63, 64, 65, 128, 255, 256):
        z1, l1 = _forward(lib, th[i:i + 1], g)
        assert np.array_equal(z1[0], clean_z[i]) and l1[0] == clean_lj[i]
        for mirror, (want_t, want_l) in enumerate(((back, ljb), (mir, ljm))):
            t1, j1 = _points(lib, clean_z[i:i + 1], g, mirror)
            assert np.array_equal(t1[0], want_t[i]) and j1[0] == want_l[i]
    moved = np.roll(th, 100, axis=0)
    zm, ljm2 = _forward(lib, moved, g)
    assert np.array_equal(np.roll(zm, -100, axis=0), clean_z) and np.array_equal(np.roll(ljm2, -100), clean_lj)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    zs, ljs = _forward(lib, th, g, stream=side)
    assert np.array_equal(zs, clean_z) and np.array_equal(ljs, clean_lj)


# ---- draw ----------------------------------------------------------------------------------------------------------------------------
def _draw(lib, key, first, n, d):
    L, so = lib
    z = torch.full((n * d + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_bridge_draw(key, first, n, d, z.data_ptr(), _stream(None)))
    assert bool((z[n * d:] == SENTINEL).all()), "cf_bridge_draw wrote past its rows"
    return z[:n * d].reshape(n, d).cpu().numpy()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", NDIMS)
def test_draws_match_the_host_generator(lib, pkg, d, n):
    key = pkg.evidence.bridge_key(11)
    for first in (0, 2**40 + 3):
        got = _draw(lib, key, first, n, d)
        ref = BR.draws(key, first, n, d)
        err = float(np.max(np.abs(got.astype(LD) - ref)))
        print(f"d = {d}, n = {n}, first = {first}: largest |device - host| = {err:.2e}  (bar 1e-14), max |z| = {np.abs(got).max():.2f}")
        assert err <= 1e-14 and np.abs(got).max() <= 8.6
    if n >= 63:
        cuts = [0, 1, n // 3, n - 1, n]
        pieces = np.concatenate([_draw(lib, key, first + a, b - a, d) for a, b in zip(cuts[:-1], cuts[1:]) if b > a])
        assert np.array_equal(pieces, got), "a row's bits depend on (key, first + row, ndim) only"
    if n == 2049:
        assert abs(got.mean()) <= 4 / np.sqrt(got.size) and abs(got.std() - 1) <= 4 / np.sqrt(2 * got.size)
        assert not np.array_equal(got, _draw(lib, pkg.evidence.bridge_key(12), first, n, d))


# ---- solve ---------------------------------------------------------------------------------------------------------------------------
def solve_inputs(n1, n2, seed=0):
    """l ~ -700 +- 30 with planted outliers of +-800 and -inf in l2 (where there is room for them)."""
    rng = np.random.default_rng([seed, n1, n2])
    l1, l2 = -700 + 30 * rng.standard_normal(n1), -700 + 30 * rng.standard_normal(n2)
    if n1 >= 8:
        l1[3] += 800.0
        l1[n1 - 2] -= 800.0
    if n2 >= 8:
        l2[2] += 800.0
        l2[n2 - 3] -= 800.0
        l2[7] = l2[n2 - 1] = -np.inf
    n_eff = max(1.0, n1 / 3.0)
    return l1, l2, float(BR.lower_median(l1)), n_eff / (n_eff + n2), n2 / (n_eff + n2)


def _solve(lib, l1, l2, lstar, s1, s2, tol=1e-13, max_iter=1000, stream=None):
    L, so = lib
    rec = torch.full((L.CF_BRIDGE_RESULT_DOUBLES + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    f2 = torch.full((len(l1) + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    d1, d2 = _dev(l1), _dev(l2)  # held until the results have been read
    torch.cuda.synchronize(DEV)
    L.check(so.cf_bridge_solve(d1.data_ptr(), len(l1), d2.data_ptr(), len(l2), lstar, s1, s2, tol, max_iter,
                               rec.data_ptr(), f2.data_ptr(), _stream(stream)))
    if stream is not None:
        stream.synchronize()
    assert bool((rec[L.CF_BRIDGE_RESULT_DOUBLES:] == SENTINEL).all()) and bool((f2[len(l1):] == SENTINEL).all())
    return dict(zip(L.BRIDGE_RESULT, rec[:L.CF_BRIDGE_RESULT_DOUBLES].cpu().tolist())), f2[:len(l1)].cpu().numpy()


@pytest.mark.parametrize("n2", SOLVE_NS)
@pytest.mark.parametrize("n1", SOLVE_NS)
def test_solve_matches_the_restatement(lib, n1, n2):
    l1, l2, lstar, s1, s2 = solve_inputs(n1, n2)
    got, f2 = _solve(lib, l1, l2, lstar, s1, s2)
    ref = BR.solve(l1, l2, lstar, s1, s2, tol=1e-13, max_iter=1000)
    d_r = abs(LD(got["log_r"]) - ref["log_r"])
    rel = {}
    for which in ("f1", "f2"):
        mean, var = ref["mean_" + which], ref["var_" + which]
        delta = 8 * np.finfo(np.float64).eps * abs(mean)
        rel["mean_" + which] = float(abs(LD(got["mean_" + which]) - mean) / mean) if mean != 0 else float(abs(got["mean_" + which]))
        allowed = 1e-10 * var + 2 * delta * np.sqrt(var) + delta * delta  # in units of which the bar below is 1e-10
        rel["var_" + which] = float(abs(LD(got["var_" + which]) - var) / allowed) * 1e-10 if allowed > 0 else float(abs(got["var_" + which]))
    d_f2 = float(np.max(np.abs(f2.astype(LD) - ref["f2"]))) * s2
    print(f"n1 = {n1}, n2 = {n2}: status {int(got['status'])} / {ref['status']}, iterations {int(got['n_iter'])} / {ref['n_iter']}, "
          f"|d log r| = {float(d_r):.2e} (bar 1e-12), moments {max(rel.values()):.2e} (bar 1e-10), f2 s2 {d_f2:.2e} (bar 1e-12)")
    # these unrelated l1 and l2 converge slowly (steps shrink by ~2 % per iteration), so the float64 rounding of r moves the
    # iteration at which a step first falls under tol by a few: the counts are held to 1 %, log r to the issue's 1e-12
    assert int(got["status"]) == ref["status"] and abs(int(got["n_iter"]) - ref["n_iter"]) <= max(1, ref["n_iter"] // 100)
    assert np.isfinite(f2).all() and all(np.isfinite(v) for v in got.values())
    assert d_r <= 1e-12 and max(rel.values()) <= 1e-10 and d_f2 <= 1e-12
    assert got["log_r"] == np.log(got["r"])
    again, f2_again = _solve(lib, l1, l2, lstar, s1, s2)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    other, f2_other = _solve(lib, l1, l2, lstar, s1, s2, stream=side)
    assert again == got and other == got and np.array_equal(f2_again, f2) and np.array_equal(f2_other, f2)


def test_solve_statuses(lib):
    L, _ = lib
    l1, l2, lstar, s1, s2 = solve_inputs(2049, 2048)
    capped, _ = _solve(lib, l1, l2, lstar, s1, s2, tol=0.0, max_iter=2)
    assert int(capped["status"]) == L.CF_BRIDGE_ITER_CAP and int(capped["n_iter"]) == 2
    ref = BR.solve(l1, l2, lstar, s1, s2, tol=0.0, max_iter=2)
    assert abs(LD(capped["log_r"]) - ref["log_r"]) <= 1e-12
    for where, value in ((0, np.nan), (2047, np.nan), (2047, np.inf)):
        bad = l2.copy()
        bad[where] = value
        rec, f2 = _solve(lib, l1, bad, lstar, s1, s2)
        assert int(rec["status"]) == L.CF_BRIDGE_NONFINITE and int(rec["n_iter"]) == 0 and np.isnan(rec["log_r"]) and np.isnan(f2).all()
    for value in (np.nan, np.inf, -np.inf):
        bad = l1.copy()
        bad[2048] = value
        assert int(_solve(lib, bad, l2, lstar, s1, s2)[0]["status"]) == L.CF_BRIDGE_NONFINITE
    nothing, _ = _solve(lib, l1, np.full(5, -np.inf), lstar, s1, s2)  # every draw outside the box: r = 0
    assert int(nothing["status"]) == L.CF_BRIDGE_NONFINITE and nothing["log_r"] == -np.inf
    # a well-overlapping pair converges in a handful of iterations
    rng = np.random.default_rng(9)
    a, b = -700 + rng.standard_normal(4097), -700.3 + 1.1 * rng.standard_normal(2049)
    ok, _ = _solve(lib, a, b, float(BR.lower_median(a)), 0.6, 0.4, tol=1e-10)
    assert int(ok["status"]) == L.CF_BRIDGE_CONVERGED and int(ok["n_iter"]) <= 20


def test_invalid_arguments_return_before_a_launch(lib):
    L, so = lib
    g = geometry(2)
    th = _dev(thetas(g, 4))
    z, lj = _out(4, 2)
    rec, f2 = _out(4, 2)
    torch.cuda.synchronize(DEV)
    inv = -1
    call = lambda n=4, d=2, lo=g["lo"], chol=g["chol"], a=th.data_ptr(): so.cf_bridge_forward(
        a, n, d, _dp(lo), _dp(g["hi"]), _dp(g["mean"]), _dp(chol), z.data_ptr(), lj.data_ptr(), None)
    assert call(d=0) == inv and call(d=17) == inv and call(n=0) == inv and call(a=None) == inv
    assert call(lo=g["hi"]) == inv and call(lo=np.array([np.nan, 0.0])) == inv and call(chol=np.zeros((2, 2))) == inv
    assert so.cf_bridge_points(th.data_ptr(), 4, 2, _dp(g["lo"]), _dp(g["hi"]), _dp(g["mean"]), _dp(g["chol"]), 2, z.data_ptr(),
                               lj.data_ptr(), None) == inv
    assert so.cf_bridge_draw(1, 0, 0, 2, z.data_ptr(), None) == inv and so.cf_bridge_draw(1, 0, 4, 17, z.data_ptr(), None) == inv
    assert so.cf_bridge_solve(th.data_ptr(), 4, th.data_ptr(), 4, 0.0, 0.5, 0.5, 1e-10, 0, rec.data_ptr(), f2.data_ptr(), None) == inv
    assert so.cf_bridge_solve(th.data_ptr(), 0, th.data_ptr(), 4, 0.0, 0.5, 0.5, 1e-10, 5, rec.data_ptr(), f2.data_ptr(), None) == inv
    assert so.cf_bridge_solve(th.data_ptr(), 4, th.data_ptr(), 4, np.nan, 0.5, 0.5, 1e-10, 5, rec.data_ptr(), f2.data_ptr(), None) == inv
    torch.cuda.synchronize(DEV)
    for buf in (z, lj, rec, f2):
        assert bool((buf == SENTINEL).all()), "a refused call wrote to its outputs"
