"""GPU (-m gpu): cf_kde_sum_device (csrc/cosmofit_kde.hip) called directly on torch buffers, as tension.py calls it, over the
shapes of tests/kde_shapes.py.  The judge is the long-double restatement tests/kde_reference.py::kernel_sums.

Parity is the project's standing bar, 1e-10 relative, element by element, for out and sq (a sum of positive terms, each good to
|exponent| * 2^-52, should sit near 1e-14; the measured maximum is printed and recorded in profiles/NOTES_tension.md).  What
the fixed order of summation promises is asserted exactly: the same bits for a row alone, at any position of a call, in a call
large enough for the other launch form, repeated, and on a second stream.  Planted conditions are exact too, and every output
buffer is followed by sentinels that must survive."""
import numpy as np
import pytest
import torch

import kde_reference as kr
import kde_shapes as ks

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
SENTINEL = -7.25e300
PAD = 64
RTOL = 1e-10
WORST = {"out": 0.0, "sq": 0.0}


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg._lib, pkg.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sums(lib, y, w, q, self_offset=-1, want_sq=True, stream=None):
    """cf_kde_sum_device on device tensors into buffers PAD longer than [m]; (out [m], sq [m]) numpy, sentinels checked."""
    L, so = lib
    n, d = y.shape
    m = q.shape[0]
    out = torch.full((m + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    sq = torch.full((m + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream.cuda_stream
    L.check(so.cf_kde_sum_device(y.data_ptr(), None if w is None else w.data_ptr(), n, d, q.data_ptr(), m, self_offset,
                                 out.data_ptr(), sq.data_ptr() if want_sq else None, st))
    if stream is not None:
        stream.synchronize()
    assert bool((out[m:] == SENTINEL).all()) and bool((sq[m:] == SENTINEL).all()), "cf_kde_sum_device wrote past its [m] rows"
    if not want_sq:
        assert bool((sq == SENTINEL).all()), "cf_kde_sum_device wrote a d_sq it was not given"
    return out[:m].cpu().numpy(), sq[:m].cpu().numpy()


def _rel(got, ref):
    err = np.abs(got.astype(LD) - ref)
    assert np.all(err[ref == 0] == 0)
    live = ref > 0
    return float(np.max(err[live] / ref[live])) if live.any() else 0.0


def test_the_sweep_reaches_every_size():
    c = ks.CASES
    assert {x[0] for x in c} == set(ks.N) and {x[1] for x in c} == set(ks.NDIM)
    assert {(x[0], x[1]) for x in c} == {(n, d) for n in ks.N for d in ks.NDIM}
    assert {(x[2], x[3]) for x in c} == {(m, s) for m in ks.M for s in ks.SELF}
    assert {(x[2], x[4]) for x in c} == {(m, wt) for m in ks.M for wt in (False, True)}
    assert {(x[1], x[3]) for x in c} == {(d, s) for d in ks.NDIM for s in ks.SELF}
    assert {(x[1], x[4]) for x in c} == {(d, wt) for d in ks.NDIM for wt in (False, True)}
    assert ks.T < ks.S and ks.S % ks.T == 0


@pytest.mark.parametrize("n,ndim,m,self_offset,weighted", ks.CASES)
def test_sums_match_the_long_double_restatement(lib, n, ndim, m, self_offset, weighted):
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type"
    m, self_offset = ks.fit(n, m, self_offset)
    y, w, q = ks.inputs(n, ndim, m, self_offset, weighted, seed=1)
    got, got2 = _sums(lib, _dev(y), _dev(w), _dev(q), self_offset)
    ref, ref2 = kr.kernel_sums(y, w, q, self_offset)
    e1, e2 = _rel(got, ref), _rel(got2, ref2)
    WORST["out"], WORST["sq"] = max(WORST["out"], e1), max(WORST["sq"], e2)
    print(f"n={n} d={ndim} m={m} self={self_offset} weighted={weighted}: out {e1:.3g} sq {e2:.3g} (worst so far {WORST['out']:.3g} "
          f"{WORST['sq']:.3g})")
    assert e1 <= RTOL and e2 <= RTOL
    # without d_sq: the same out, and nothing written to the buffer
    alone, _ = _sums(lib, _dev(y), _dev(w), _dev(q), self_offset, want_sq=False)
    np.testing.assert_array_equal(alone.view(np.uint64), got.view(np.uint64))


def test_planted_conditions_are_exact(lib):
    rng = np.random.default_rng(5)
    n, d = 2 * ks.S + 3, 3
    y = rng.standard_normal((n, d))
    w = 10.0 ** rng.uniform(-3.0, 0.0, n)
    q = rng.standard_normal((300, d))
    base, base2 = _sums(lib, _dev(y), _dev(w), _dev(q))
    assert np.all(base > 0)
    # a query 10^3 units from every sample: exactly 0.0 (exp underflows; nothing rescales)
    far = q.copy()
    far[7] = 1.0e3
    got, got2 = _sums(lib, _dev(y), _dev(w), _dev(far))
    assert got[7] == 0.0 and got2[7] == 0.0 and not np.signbit(got[7])
    keep = np.arange(300) != 7
    np.testing.assert_array_equal(got[keep].view(np.uint64), base[keep].view(np.uint64))
    # one sample, and the query is that sample: nothing is left to sum
    one = _dev(y[:1])
    got, got2 = _sums(lib, one, None, one, 0)
    assert got[0] == 0.0 and got2[0] == 0.0
    got, _ = _sums(lib, one, None, one, -1)
    assert got[0] == 1.0
    # NaN and +-inf coordinates: NaN in that row (out and sq) and no other bit changes
    bad = q.copy()
    bad[0, 1], bad[150, 0], bad[299, 2] = np.nan, np.inf, -np.inf
    got, got2 = _sums(lib, _dev(y), _dev(w), _dev(bad))
    rows = np.array([0, 150, 299])
    assert np.isnan(got[rows]).all() and np.isnan(got2[rows]).all()
    keep = np.ones(300, dtype=bool)
    keep[rows] = False
    np.testing.assert_array_equal(got[keep].view(np.uint64), base[keep].view(np.uint64))
    np.testing.assert_array_equal(got2[keep].view(np.uint64), base2[keep].view(np.uint64))
    # a zero-weight sample changes no bit of any row, wherever it lies: on a query, elsewhere, or where it underflows
    w0 = w.copy()
    w0[[0, 1000, ks.S, n - 1]] = 0.0
    ref, ref2 = _sums(lib, _dev(y), _dev(w0), _dev(q))
    for place in (q[5], np.full(d, 0.3), np.full(d, 1.0e3)):
        y2 = y.copy()
        y2[[0, 1000, ks.S, n - 1]] = place
        got, got2 = _sums(lib, _dev(y2), _dev(w0), _dev(q))
        np.testing.assert_array_equal(got.view(np.uint64), ref.view(np.uint64))
        np.testing.assert_array_equal(got2.view(np.uint64), ref2.view(np.uint64))


@pytest.mark.parametrize("ndim,weighted", [(1, False), (3, True), (8, True)])
def test_a_rows_bits_depend_on_the_row_alone(lib, ndim, weighted):
    rng = np.random.default_rng(ndim)
    n, m, off = 2 * ks.S + 3, 257, 5
    y = rng.standard_normal((n, ndim))
    w = 10.0 ** rng.uniform(-3.0, 0.0, n) if weighted else None
    dy, dw = _dev(y), _dev(w)
    q = np.ascontiguousarray(y[off: off + m])
    # leave-one-out: query i is sample off + i
    ref, ref2 = _sums(lib, dy, dw, _dev(q), off)
    again, again2 = _sums(lib, dy, dw, _dev(q), off)
    np.testing.assert_array_equal(again.view(np.uint64), ref.view(np.uint64))
    np.testing.assert_array_equal(again2.view(np.uint64), ref2.view(np.uint64))
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    other, other2 = _sums(lib, dy, dw, _dev(q), off, stream=side)
    np.testing.assert_array_equal(other.view(np.uint64), ref.view(np.uint64))
    np.testing.assert_array_equal(other2.view(np.uint64), ref2.view(np.uint64))
    for r in (0, 1, 100, 255, 256):
        alone, alone2 = _sums(lib, dy, dw, _dev(q[r: r + 1]), off + r)
        assert alone.view(np.uint64)[0] == ref.view(np.uint64)[r] and alone2.view(np.uint64)[0] == ref2.view(np.uint64)[r], r
    # the rows 50 .. 149 as a call of their own: another position in the workgroup
    part, part2 = _sums(lib, dy, dw, _dev(q[50:150]), off + 50)
    np.testing.assert_array_equal(part.view(np.uint64), ref[50:150].view(np.uint64))
    np.testing.assert_array_equal(part2.view(np.uint64), ref2[50:150].view(np.uint64))
    # without the self skip: alone, in the 257-row call, and tiled into a call large enough for the other launch form
    free, free2 = _sums(lib, dy, dw, _dev(q))
    assert np.all(free > ref)
    L = lib[0]
    reps = (L.CF_KDE_SPLIT_BELOW_BLOCKS * L.CF_KDE_QUERY_BLOCK) // m + 1
    big, big2 = _sums(lib, dy, dw, _dev(np.tile(q, (reps, 1))))
    assert big.size >= L.CF_KDE_SPLIT_BELOW_BLOCKS * L.CF_KDE_QUERY_BLOCK
    np.testing.assert_array_equal(big.view(np.uint64).reshape(reps, m), np.broadcast_to(free.view(np.uint64), (reps, m)))
    np.testing.assert_array_equal(big2.view(np.uint64).reshape(reps, m), np.broadcast_to(free2.view(np.uint64), (reps, m)))
    alone, _ = _sums(lib, dy, dw, _dev(q[100:101]))
    assert alone.view(np.uint64)[0] == free.view(np.uint64)[100]


def test_invalid_arguments_launch_nothing(lib):
    L, so = lib
    n, d, m = 100, 3, 10
    y = torch.zeros((n, d), dtype=torch.float64, device=DEV)
    q = torch.zeros((m, d), dtype=torch.float64, device=DEV)
    out = torch.full((m + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    sq = torch.full((m + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream

    def call(y_p=y.data_ptr(), nn=n, nd=d, q_p=q.data_ptr(), mm=m, off=-1, out_p=out.data_ptr()):
        return so.cf_kde_sum_device(y_p, None, nn, nd, q_p, mm, off, out_p, sq.data_ptr(), st)

    bad = [dict(nd=0), dict(nd=9), dict(nd=-1), dict(nn=0), dict(nn=-5), dict(mm=0), dict(mm=-1), dict(y_p=None), dict(q_p=None),
           dict(out_p=None), dict(off=n - m + 1), dict(off=n), dict(off=-2)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"cf_kde_sum_device" in so.cf_last_error(), kw
    with pytest.raises(L.CosmofitError, match="CF_ERR_INVALID.*ndim"):
        L.check(call(nd=9))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((sq == SENTINEL).all()), "a refused cf_kde_sum_device wrote results"
    assert call() == 0 and call(off=n - m) == 0
    torch.cuda.synchronize()
    assert bool((out[:m] == float(n - 1)).all()) and bool((out[m:] == SENTINEL).all())  # all points equal: n - 1 terms of 1.0
