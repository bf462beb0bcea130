"""GPU (-m gpu): cf_ns_walk_start / cf_ns_propose / cf_ns_accept / cf_ns_transform (csrc/cosmofit_nested.hip) called directly
on torch buffers, as nested.py calls them, over the values their entry points accept: ndim 1 .. 16, two to a thousand
survivors (one for the walk start), 1 .. 1000 walkers around the 64-lane waves and 256-thread blocks, uniform, normal and
alternating priors, the sampler's DE scale with and without jitter, no move at all, a wide jitter.

Where no device libm call enters (sigma = 0, uniform dimensions, the walk start, the accept) the kernels have the bits of the
float64 restatement; with sigma > 0 the judge is long double and the bound comes from the reference's own terms
(tests/move_shapes.py: ns_propose_ld), which tests/test_move_shapes_cpu.py shows to hold for float64 and to be missed by a
dropped term or a shifted partner by eight orders.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import move_shapes as ms
import nested_reference as nr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
SENTINEL = -7.25e300
SEEDS = list(range(ms.NS_DEFAULT))


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg._lib, pkg.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the cases are shared and read-only


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _prior(L, prior):
    kind, a, b = prior
    p = L.cf_ns_prior()
    p.ndim = len(kind)
    for k in range(p.ndim):
        p.kind[k], p.a[k], p.b[k] = int(kind[k]), float(a[k]), float(b[k])
    return p


def _full(shape, dtype=torch.float64, value=SENTINEL):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _propose(lib, prior, su, key, gamma, sigma, wu, wtheta):
    """cf_ns_propose into buffers one row longer than m: (pu, ptheta, ok)."""
    L, so = lib
    m, d = wu.shape
    p = _prior(L, prior)
    pu, pth, ok = _full((m + 1, d)), _full((m + 1, d)), _full((m + 1,), torch.int32, -7)
    dsu, dwu, dwth = _dev(su), _dev(wu), _dev(wtheta)
    L.check(so.cf_ns_propose(C.byref(p), dsu.data_ptr(), su.shape[0], m, key, gamma, sigma, dwu.data_ptr(), dwth.data_ptr(),
                             pu.data_ptr(), pth.data_ptr(), ok.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert bool((pu[m] == SENTINEL).all()) and bool((pth[m] == SENTINEL).all()) and int(ok[m]) == -7, "cf_ns_propose wrote past m rows"
    return pu[:m].cpu().numpy(), pth[:m].cpu().numpy(), ok[:m].cpu().numpy()


def _check_ok_and_theta(prior, pu, pth, ok, wtheta):
    """ok is 0 exactly when a coordinate is <= 0 or >= 1; ptheta is wtheta's bits outside, T(pu) inside."""
    from scipy.special import ndtri

    kind, a, b = prior
    inside = ms.ns_inside(pu)
    np.testing.assert_array_equal(ok, inside.astype(np.int32))
    np.testing.assert_array_equal(_bits(pth[~inside]), _bits(wtheta[~inside]))
    uni = kind == 0
    u = pu[inside]
    np.testing.assert_array_equal(_bits(pth[inside][:, uni]), _bits(a[uni] + u[:, uni] * (b[uni] - a[uni])))
    un, got = u[:, ~uni], pth[inside][:, ~uni]
    assert np.all(np.isfinite(got))
    mid = (un >= 1e-9) & (un <= 1.0 - 1e-9)
    want = a[~uni] + b[~uni] * ndtri(un)
    np.testing.assert_allclose(got[mid], want[mid], rtol=1e-13, atol=1e-13)
    return int(inside.sum())


@pytest.mark.parametrize("seed", SEEDS)
def test_walk_start_is_numpy_indexing_by_the_restated_uniform(lib, seed):
    """cf_ns_walk_start: walker i starts at survivor floor(U_i n_surv); with one survivor every walker starts there."""
    L, so = lib
    c = ms.ns_case(seed)
    m, d, ns = c["m"], c["ndim"], c["n_surv"]
    wu, wth, wl = _full((m + 1, d)), _full((m + 1, d)), _full((m + 1,))
    dsu, dsth, dsl = _dev(c["su"]), _dev(c["stheta"]), _dev(c["slogl"])
    L.check(so.cf_ns_walk_start(dsu.data_ptr(), dsth.data_ptr(), dsl.data_ptr(), ns, d, m, c["key"], wu.data_ptr(), wth.data_ptr(),
                                wl.data_ptr(), _stream()))
    torch.cuda.synchronize()
    j = np.minimum((nr.uniform(c["key"], 0, np.arange(m)) * float(ns)).astype(np.int64), ns - 1)
    if ns == 1:
        assert np.all(j == 0)
    elif m >= 63:
        assert len(set(j.tolist())) > 1
    np.testing.assert_array_equal(_bits(wu[:m].cpu().numpy()), _bits(c["su"][j]))
    np.testing.assert_array_equal(_bits(wth[:m].cpu().numpy()), _bits(c["stheta"][j]))
    np.testing.assert_array_equal(_bits(wl[:m].cpu().numpy()), _bits(c["slogl"][j]))
    assert bool((wu[m] == SENTINEL).all()) and bool((wth[m] == SENTINEL).all()) and float(wl[m]) == SENTINEL


@pytest.mark.parametrize("seed", SEEDS)
def test_propose_against_the_restatement(lib, seed):
    """cf_ns_propose: sigma = 0 has the float64 restatement's bits (contraction is off in that kernel), (gamma, sigma) = (0, 0)
    returns the walker, sigma > 0 is within the bound of the long-double statement; ok and ptheta follow from pu."""
    c = ms.ns_case(seed)
    if c["n_surv"] < 2:
        c = ms.ns_case(seed, n_surv=2)
    pu, pth, ok = _propose(lib, c["prior"], c["su"], c["key"], c["gamma"], c["sigma"], c["wu"], c["wtheta"])
    if c["sigma"] == 0.0:
        np.testing.assert_array_equal(_bits(pu), _bits(ms.ns_propose_f64(c["key"], c["gamma"], 0.0, c["su"], c["wu"])))
        if c["gamma"] == 0.0:
            np.testing.assert_array_equal(_bits(pu), _bits(c["wu"]))
        frac = 0.0
    else:
        want, bound = ms.ns_propose_ld(c["key"], c["gamma"], c["sigma"], c["su"], c["wu"])
        frac = float(np.max(np.abs(pu.astype(LD) - want) / bound))
        assert frac <= 1.0, f"seed {seed}: {frac:.3f} of the bound"
    n_in = _check_ok_and_theta(c["prior"], pu, pth, ok, c["wtheta"])
    print(f"seed {seed}: ndim={c['ndim']} n_surv={c['n_surv']} m={c['m']} prior={c['prior_kind']} (gamma, sigma)={c['gs']}: "
          f"{n_in} of {c['m']} inside, largest error / bound {frac:.3f}")


@pytest.mark.parametrize("ndim,m", [(1, 257), (16, 1000)])
def test_two_survivors_are_always_two_different_partners(lib, ndim, m):
    c = ms.ns_case(100 + ndim, ndim=ndim, n_surv=2, m=m, gs=(0.25, 0.0), prior_kind="uniform")
    pu, _, _ = _propose(lib, c["prior"], c["su"], c["key"], 0.25, 0.0, c["wu"], c["wtheta"])
    d01 = 0.25 * (c["su"][0] - c["su"][1])
    d10 = 0.25 * (c["su"][1] - c["su"][0])
    fwd = np.all(_bits(pu) == _bits(c["wu"] + d01), axis=1)
    rev = np.all(_bits(pu) == _bits(c["wu"] + d10), axis=1)
    assert np.all(fwd ^ rev), "pu - wu is +gamma (su_0 - su_1) or its negative, never 0"
    assert fwd.any() and rev.any()


def test_the_faces_of_the_cube_are_outside(lib):
    """ok is 0 for a coordinate exactly 0.0 or 1.0, 1 for the smallest positive double and for the largest double below 1."""
    d = 4
    c = ms.ns_case(200, ndim=d, n_surv=3, m=70, gs=(0.0, 0.0), prior_kind="alternating")
    wu = c["wu"].copy()
    wu[3, 0], wu[10, 3], wu[64, 1], wu[65, 2] = 0.0, 1.0, 0.0, 1.0           # on a face: outside
    wu[5, 1], wu[6, 0], wu[66, 3], wu[67, 2] = 5e-324, 5e-324, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53  # inside
    pu, pth, ok = _propose(lib, c["prior"], c["su"], c["key"], 0.0, 0.0, wu, c["wtheta"])
    np.testing.assert_array_equal(_bits(pu), _bits(wu))
    want = np.ones(70, dtype=np.int32)
    want[[3, 10, 64, 65]] = 0
    np.testing.assert_array_equal(ok, want)
    _check_ok_and_theta(c["prior"], pu, pth, ok, c["wtheta"])
    # a PROPOSAL that lands exactly on a face: u = 0.5, gamma = 2, survivors at 0.5 and 0.25 give 0.5 +- 2 x 0.25 = 1.0 or 0.0
    m = 300
    su = np.array([[0.5, 0.5], [0.25, 0.5]])
    wu = np.full((m, 2), 0.5)
    wth = np.full((m, 2), 3.5)
    pu, pth, ok = _propose(lib, ms.ns_prior("uniform", 2), su, 77, 2.0, 0.0, wu, wth)
    assert set(pu[:, 0].tolist()) == {0.0, 1.0} and np.all(pu[:, 1] == 0.5)
    assert np.all(ok == 0)
    np.testing.assert_array_equal(_bits(pth), _bits(wth))


def test_inverse_normal_cdf_in_the_tails(lib):
    """Phi^-1 through cf_ns_transform at u from 1e-300 to 1e-9, 2^-53 and 1 - 1e-16 .. 1 - 1e-9, where a walk proposal can land
    although the prior draw cannot: finite, non-decreasing, of the right sign, within 1e-10 relative of mpmath at 30 digits
    (such a point carries under 1e-9 of the prior mass: 1e-10 there moves no evidence or moment at the precision the nested
    tests assert)."""
    L, so = lib
    u = ms.ns_tail_u()
    assert np.all(np.diff(u) > 0) and u[0] == 1e-300 and u[-1] == 1.0 - 2.0 ** -53
    p = _prior(L, (np.array([1], dtype=np.int32), np.array([0.0]), np.array([1.0])))
    du, out = _dev(u), _full((u.size + 1,))
    L.check(so.cf_ns_transform(C.byref(p), du.data_ptr(), u.size, out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert float(out[u.size]) == SENTINEL
    got = out[: u.size].cpu().numpy()
    want = ms.ns_tail_reference(u)
    rel = np.array([abs((float(g) - w) / w) for g, w in zip(got, want)], dtype=np.float64)
    k = int(rel.argmax())
    print(f"Phi^-1 in the tails: largest relative error {rel[k]:.3e} at u = {u[k]!r} (value {got[k]!r}); lower tail "
          f"{rel[u < 0.5].max():.3e}, upper tail {rel[u > 0.5].max():.3e}")
    assert np.all(np.isfinite(got))
    assert np.all(np.diff(got) >= 0.0), "non-decreasing in u"
    assert np.all(got[u < 0.5] < 0.0) and np.all(got[u > 0.5] > 0.0)
    assert rel.max() <= 1e-10


@pytest.mark.parametrize("seed", SEEDS)
def test_accept_counts_and_moves_exactly_the_accepted_rows(lib, seed):
    """cf_ns_accept: accept iff inside the cube and L* < log L < inf; l == L* is rejected; +inf, -inf and NaN count as non-finite;
    ok = 0 counts as out of the cube whatever l is; the three counters add over two calls; nothing is written past m rows."""
    L, so = lib
    c = ms.ns_case(seed)
    m, d = c["m"], c["ndim"]
    rng = np.random.default_rng(seed)
    lstar = 0.125
    wu, wth, wl = _full((m + 1, d)), _full((m + 1, d)), _full((m + 1,))
    wu[:m], wth[:m], wl[:m] = _dev(c["wu"]), _dev(c["wtheta"]), _dev(c["wlogl"])
    eu, eth, el = c["wu"].copy(), c["wtheta"].copy(), c["wlogl"].copy()
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    counts[3] = -7
    dlstar = _dev(np.array([lstar]))
    total = np.zeros(3, dtype=np.int64)
    for call in range(2):
        pu, pth = rng.uniform(0, 1, (m, d)), rng.standard_normal((m, d)) + 50.0 * (call + 1)
        pl = lstar + rng.standard_normal(m)
        ok = (rng.uniform(size=m) < 0.8).astype(np.int32)
        plant = [(lstar, 1), (math.inf, 1), (-math.inf, 1), (math.nan, 1), (lstar + 1.0, 0), (math.nan, 0), (math.inf, 0),
                 (np.nextafter(lstar, 1.0), 1), (np.nextafter(lstar, -1.0), 1)]
        rows = rng.permutation(m)[: len(plant)]
        for r, (l, o) in zip(rows, plant):
            pl[r], ok[r] = l, o
        out = ok == 0
        bad = ~out & ~np.isfinite(pl)
        with np.errstate(invalid="ignore"):
            acc = ~out & ~bad & (pl > lstar)
        for r, want in zip(rows, [False, False, False, False, False, False, False, True, False]):
            assert bool(acc[r]) == want
        eu[acc], eth[acc], el[acc] = pu[acc], pth[acc], pl[acc]
        total += [int(acc.sum()), int(out.sum()), int(bad.sum())]
        dpu, dpth, dok, dpl = _dev(pu), _dev(pth), _dev(ok), _dev(pl)
        L.check(so.cf_ns_accept(m, d, dlstar.data_ptr(), dpu.data_ptr(), dpth.data_ptr(), dok.data_ptr(), dpl.data_ptr(), wu.data_ptr(),
                                wth.data_ptr(), wl.data_ptr(), counts.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert counts.cpu().numpy().tolist() == total.tolist() + [-7]
        np.testing.assert_array_equal(_bits(wu[:m].cpu().numpy()), _bits(eu))  # rejected rows keep their bits
        np.testing.assert_array_equal(_bits(wth[:m].cpu().numpy()), _bits(eth))
        np.testing.assert_array_equal(_bits(wl[:m].cpu().numpy()), _bits(el))
        assert bool((wu[m] == SENTINEL).all()) and bool((wth[m] == SENTINEL).all()) and float(wl[m]) == SENTINEL
