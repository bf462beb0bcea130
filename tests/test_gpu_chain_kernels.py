"""GPU (-m gpu): chain_mean / chain_lagsum / chain_acf_mean (csrc/cosmofit_chain.hip) called directly on torch buffers, as
chain_stats.py calls them, at the shapes the C entry points accept: n_t = 1 .. 2500 around the 16-step chunks and the
8 x 16-step point below which time segments are empty, n_s around the 64-series blocks, lag ranges with tails, lags past
the end of the chain.

The judge is long double (tests/chain_shapes.py: the reference and the bounds derived from its own terms);
tests/test_quasar_shapes_cpu.py shows on the CPU that the bounds hold for the kernel's summation order with a factor 5 to
spare and that a single dropped product misses them by five orders.  What the kernels promise exactly is asserted exactly:
the same bits for any split of the lag range, any position of a series in the chain and any repetition, 0.0 for a lag at
or past n_t, and no write outside the output.
"""
import numpy as np
import pytest
import torch

import chain_shapes as cs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg._lib, pkg.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _mean(lib, dx):
    """chain_mean into a buffer one 64-series block longer than needed; the spare block keeps its sentinel."""
    L, so = lib
    n_t, n_s = dx.shape
    buf = torch.full((n_s + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_chain_mean(dx.data_ptr(), n_t, n_s, buf.data_ptr(), _stream()))
    assert bool((buf[n_s:] == SENTINEL).all()), "chain_mean wrote past its n_s means"
    return buf[:n_s]


def _lagsum(lib, dx, dmean, lag0, nlag):
    """chain_lagsum into a buffer one row and one 64-series block longer than [nlag, n_s]; the spare part keeps its sentinel."""
    L, so = lib
    n_t, n_s = dx.shape
    buf = torch.full((nlag * n_s + n_s + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_chain_lagsum(dx.data_ptr(), dmean.data_ptr(), n_t, n_s, lag0, nlag, buf.data_ptr(), _stream()))
    assert bool((buf[nlag * n_s:] == SENTINEL).all()), "chain_lagsum wrote past its [nlag, n_s] sums"
    return buf[: nlag * n_s].view(nlag, n_s)


CASES = [(n_t, cs.N_S[(2 * k + j) % len(cs.N_S)]) for k, n_t in enumerate(cs.N_T) for j in range(2)]


def test_the_sweep_reaches_every_size():
    assert {n for n, _ in CASES} == set(cs.N_T) and {s for _, s in CASES} == set(cs.N_S)
    nlags = {nl for _, nl in cs.lag_ranges(400)}
    assert {1, 15, 16, 17, 64, 100} <= nlags and {0, 1, 16, 37, 399} <= {l0 for l0, _ in cs.lag_ranges(400)}
    assert any(l0 + nl > 400 for l0, nl in cs.lag_ranges(400))


@pytest.mark.parametrize("n_t,n_s", CASES)
def test_mean_and_lag_sums_against_long_double(lib, n_t, n_s):
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type, not float64 judging float64"
    x = cs.series(n_t, n_s, seed=1000 * n_t + n_s)
    dx = torch.from_numpy(x).to(DEV)
    m_ref, d = cs.reference_mean(x)
    dmean = _mean(lib, dx)
    mean = dmean.cpu().numpy()
    err = np.abs(mean - m_ref.astype(np.float64))
    print(f"n_t={n_t} n_s={n_s}: mean, largest error / bound {float(np.max(err / cs.mean_bound(x))):.3f}")
    assert np.all(err <= cs.mean_bound(x))
    cache, worst = {}, (0.0, None)
    for lag0, nlag in cs.lag_ranges(n_t):
        got = _lagsum(lib, dx, dmean, lag0, nlag).cpu().numpy()
        for j in range(nlag):
            tau = lag0 + j
            if tau >= n_t:
                np.testing.assert_array_equal(got[j], np.zeros(n_s), err_msg=f"lag {tau} at or past n_t = {n_t} is 0.0")
                continue
            if tau not in cache:
                cache[tau] = (cs.reference_lagsum(x, d, tau).astype(np.float64), cs.lagsum_bound(x, d, tau))
            ref, bound = cache[tau]
            e = np.abs(got[j] - ref)
            frac = float(np.max(e / bound))
            if frac > worst[0]:
                worst = (frac, (lag0, nlag, tau))
            assert np.all(e <= bound), f"n_t={n_t} n_s={n_s} lag0={lag0} nlag={nlag} lag {tau}: {frac:.3f} of the bound"
    print(f"n_t={n_t} n_s={n_s}: lag sums, largest error / bound {worst[0]:.3f} at (lag0, nlag, lag) = {worst[1]}")


@pytest.mark.parametrize("n_t,n_s", [(130, 96), (400, 65), (17, 200), (2500, 64)])
def test_exact_properties_of_the_lag_sums(lib, n_t, n_s):
    x = cs.series(n_t, n_s, seed=77 + n_t)
    dx = torch.from_numpy(x).to(DEV)
    dmean = _mean(lib, dx)
    whole = _lagsum(lib, dx, dmean, 0, 80).cpu().numpy()
    # the lag range split between calls, at a 16-lag block and inside one, and started off a block
    for cut in (64, 70, 1, 15, 17):
        parts = np.concatenate([_lagsum(lib, dx, dmean, 0, cut).cpu().numpy(), _lagsum(lib, dx, dmean, cut, 80 - cut).cpu().numpy()])
        np.testing.assert_array_equal(parts, whole, err_msg=f"[0, 80) against [0, {cut}) + [{cut}, 80)")
    np.testing.assert_array_equal(_lagsum(lib, dx, dmean, 37, 5).cpu().numpy(), whole[37:42])
    # a second call: the same bits
    np.testing.assert_array_equal(_lagsum(lib, dx, dmean, 0, 80).cpu().numpy(), whole)
    np.testing.assert_array_equal(_mean(lib, dx).cpu().numpy(), dmean.cpu().numpy())
    # lags at or past n_t are 0.0; the others are not
    tail = _lagsum(lib, dx, dmean, n_t - 3, 40).cpu().numpy()
    np.testing.assert_array_equal(tail[3:], np.zeros((37, n_s)))
    assert np.all(tail[:3] != 0.0)
    np.testing.assert_array_equal(_lagsum(lib, dx, dmean, n_t + 1000, 17).cpu().numpy(), np.zeros((17, n_s)))
    # a series keeps its bits wherever it stands in the chain (other lane, other block, the ragged last block)
    perm = np.random.default_rng(n_t).permutation(n_s)
    dxp = torch.from_numpy(np.ascontiguousarray(x[:, perm])).to(DEV)
    dmp = _mean(lib, dxp)
    np.testing.assert_array_equal(dmp.cpu().numpy(), dmean.cpu().numpy()[perm])
    np.testing.assert_array_equal(_lagsum(lib, dxp, dmp, 0, 80).cpu().numpy(), whole[:, perm])


@pytest.mark.parametrize("n_w,ndim,nlag", [(1, 1, 1), (3, 4, 17), (64, 5, 64), (37, 16, 100), (300, 3, 257)])
def test_acf_mean_against_long_double(lib, n_w, ndim, nlag):
    """f[j][d] = (sum_w lagsum[j][w, d] / c0[w, d]) / n_w.  Bound: every quotient and every one of the n_w - 1 additions
    rounds once, each by at most u x (the sum of the |quotients|), and so does the final division: n_w u sum |quotients|
    covers them.  One walker with c0 = 0 makes its dimension NaN (0 / 0, as in emcee) and no other."""
    L, so = lib
    assert np.finfo(LD).eps < 1e-18
    n_t = max(nlag + 3, 40)
    x = cs.series(n_t, n_w * ndim, seed=n_w)
    dead = None
    if n_w > 1:
        dead = (n_w // 2) * ndim + (ndim - 1)  # a walker that never moved in the last dimension
        x[:, dead] = 64.0  # n_t x 64 and its quotient by n_t are exact: the deviations are 0.0, not rounding dust
    dx = torch.from_numpy(x).to(DEV)
    dmean = _mean(lib, dx)
    sums = _lagsum(lib, dx, dmean, 0, nlag).contiguous()
    c0 = sums[0].clone()
    f = torch.full((nlag * ndim + 64,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_chain_acf_mean(sums.data_ptr(), c0.data_ptr(), n_w, ndim, nlag, f.data_ptr(), _stream()))
    assert bool((f[nlag * ndim:] == SENTINEL).all())
    got = f[: nlag * ndim].view(nlag, ndim).cpu().numpy()
    s = sums.cpu().numpy().astype(LD).reshape(nlag, n_w, ndim)
    with np.errstate(invalid="ignore"):
        q = s / c0.cpu().numpy().astype(LD).reshape(1, n_w, ndim)
    want = (q.sum(axis=1) / LD(n_w)).astype(np.float64)
    bound = (n_w * cs.U * np.abs(q).sum(axis=1)).astype(np.float64)
    live = np.ones(ndim, dtype=bool)
    if dead is not None:
        assert float(c0[dead]) == 0.0
        live[ndim - 1] = False
        assert np.isnan(got[:, ndim - 1]).all()
    assert np.all(np.isfinite(got[:, live]))
    err = np.abs(got[:, live] - want[:, live])
    print(f"n_w={n_w} ndim={ndim} nlag={nlag}: largest error / bound {float(np.max(err / bound[:, live])):.3f}")
    assert np.all(err <= bound[:, live])
    np.testing.assert_array_equal(got[0, live], np.ones(int(live.sum())))  # lag 0: every quotient is 1
