"""GPU (-m gpu): cf_marg_bin / cf_marg_hist (csrc/cosmofit_marginals.hip) called directly on torch buffers, as marginals.py
calls them, over the shapes of tests/marginals_shapes.py.  The judge is numpy (tests/marginals_reference.py): np.histogram
and np.histogram2d for indices and counts, long double for weighted sums.

Indices and counts are conditions, not tolerances: every element and every bin is compared, on inputs that hold every edge,
both neighbours of every edge, NaN and +-inf in every column.  Weighted sums meet the fixed-point bound derived in
tests/test_marginals_cpu.py.  What integer sums promise is asserted exactly: the same bits for any repetition, any
n_segments and any order of the rows; and every output buffer is followed by a sentinel that must survive."""
import ctypes as C

import numpy as np
import pytest
import torch

import marginals_reference as mr
import marginals_shapes as ms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
IDX_SENTINEL = 0xAB
H_SENTINEL = -0x5A5A5A5A5A5A5A5A
PAD = 256


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg._lib, pkg.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _bin(lib, dx, edges, offset=0):
    """cf_marg_bin into a byte buffer PAD longer than [n, ndim] (and `offset` bytes into it); the rest keeps its sentinel."""
    L, so = lib
    n, ndim = dx.shape
    bins = edges.shape[1] - 1
    de = torch.from_numpy(edges).to(DEV)
    buf = torch.full((offset + n * ndim + PAD,), IDX_SENTINEL, dtype=torch.uint8, device=DEV)
    L.check(so.cf_marg_bin(dx.data_ptr(), n, ndim, de.data_ptr(), bins, buf.data_ptr() + offset, _stream()))
    assert bool((buf[:offset] == IDX_SENTINEL).all()) and bool((buf[offset + n * ndim:] == IDX_SENTINEL).all()), \
        "cf_marg_bin wrote outside its [n, ndim] indices"
    return buf[offset: offset + n * ndim].view(n, ndim)


def _hist(lib, idx, bins, pairs, w=None, w_max=0.0, nseg=0):
    """cf_marg_hist into int64 buffers PAD longer than needed; (h1 [ndim, bins], h2 [npairs, bins, bins]) numpy int64."""
    L, so = lib
    n, ndim = idx.shape
    assert idx.is_contiguous() or idx.stride() == (ndim, 1)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n1, n2 = ndim * bins, len(pr) * bins * bins
    b1 = torch.full((n1 + PAD,), H_SENTINEL, dtype=torch.int64, device=DEV)
    b2 = torch.full((n2 + PAD,), H_SENTINEL, dtype=torch.int64, device=DEV)
    L.check(so.cf_marg_hist(idx.data_ptr(), None if w is None else w.data_ptr(), w_max, n, ndim, bins,
                            pr.ctypes.data_as(C.c_void_p), len(pr), b1.data_ptr(), b2.data_ptr() if len(pr) else None, nseg,
                            _stream()))
    assert bool((b1[n1:] == H_SENTINEL).all()) and bool((b2[n2:] == H_SENTINEL).all()), "cf_marg_hist wrote outside its histograms"
    return b1[:n1].view(ndim, bins).cpu().numpy(), b2[:n2].view(len(pr), bins, bins).cpu().numpy()


def _in_range(x, lo_hi):
    with np.errstate(invalid="ignore"):
        return (x >= lo_hi[:, 0]) & (x <= lo_hi[:, 1])


def test_the_sweep_reaches_every_size():
    assert {c[0] for c in ms.CASES} == set(ms.N) and {c[1] for c in ms.CASES} == set(ms.NDIM)
    assert {c[2] for c in ms.CASES} == set(ms.BINS)
    for k, sizes in enumerate((ms.N, ms.NDIM, ms.BINS)):
        assert all(sum(c[k] == s for c in ms.CASES) >= 2 for s in sizes)


@pytest.mark.parametrize("n,ndim,bins", ms.CASES)
def test_indices_and_counts_are_numpys(lib, n, ndim, bins):
    x, lo_hi = ms.inputs(n, ndim, bins, seed=n + ndim + bins)
    edges = mr.edges_of(lo_hi, bins)
    dx = torch.from_numpy(x).to(DEV)
    idx = _bin(lib, dx, edges)
    want = mr.bin_indices(x, edges)
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
    pairs = ms.all_pairs(ndim)
    h1, h2 = _hist(lib, idx, bins, pairs)
    np.testing.assert_array_equal(h1, mr.hist1(x, lo_hi, bins))
    np.testing.assert_array_equal(h2, mr.hist2(x, lo_hi, bins, pairs))
    # conservation, against numpy's own count of the rows in range
    ok = _in_range(x, lo_hi)
    np.testing.assert_array_equal(h1.sum(axis=1), ok.sum(axis=0))
    for p, (a, b) in enumerate(pairs):
        assert h2[p].sum() == int((ok[:, a] & ok[:, b]).sum())


@pytest.mark.parametrize("n,ndim,bins", [(257, 3, 20), (4097, 5, 100)])
def test_an_index_buffer_at_any_byte_offset(lib, n, ndim, bins):
    """The index pass stores four bytes at a time where the buffer allows it and single bytes where not: the same indices."""
    x, lo_hi = ms.inputs(n, ndim, bins, seed=3)
    edges = mr.edges_of(lo_hi, bins)
    dx = torch.from_numpy(x).to(DEV)
    want = mr.bin_indices(x, edges)
    for offset in (1, 2, 3, 4):
        idx = _bin(lib, dx, edges, offset=offset)
        np.testing.assert_array_equal(idx.cpu().numpy(), want)
        h1, _ = _hist(lib, idx, bins, [])
        np.testing.assert_array_equal(h1, mr.hist1(x, lo_hi, bins))


def test_pair_lists(lib):
    n, ndim, bins = 4097, 5, 20
    x, lo_hi = ms.inputs(n, ndim, bins, seed=11)
    edges = mr.edges_of(lo_hi, bins)
    idx = _bin(lib, torch.from_numpy(x).to(DEV), edges)
    full = ms.all_pairs(ndim)
    h1_all, h2_all = _hist(lib, idx, bins, full)
    # a subset, a repeated pair, (a, b) with (b, a), a column with itself
    pairs = [(3, 1), (4, 0), (3, 1), (1, 3), (2, 2)]
    h1, h2 = _hist(lib, idx, bins, pairs)
    np.testing.assert_array_equal(h1, h1_all)
    np.testing.assert_array_equal(h2, mr.hist2(x, lo_hi, bins, pairs))
    np.testing.assert_array_equal(h2[0], h2_all[full.index((3, 1))])
    np.testing.assert_array_equal(h2[0], h2[2])
    np.testing.assert_array_equal(h2[3], h2[0].T)
    np.testing.assert_array_equal(h2[4], np.diag(h1[2]))
    # the most pairs one call takes
    many = [full[i % len(full)] for i in range(256)]
    _, h2m = _hist(lib, idx, bins, many)
    for i, pr in enumerate(many):
        np.testing.assert_array_equal(h2m[i], h2_all[full.index(pr)])
    # one column, no pairs
    x1, lo_hi1 = ms.inputs(1000, 1, 100, seed=12)
    idx1 = _bin(lib, torch.from_numpy(x1).to(DEV), mr.edges_of(lo_hi1, 100))
    h1, h2 = _hist(lib, idx1, 100, [])
    assert h2.shape == (0, 100, 100)
    np.testing.assert_array_equal(h1, mr.hist1(x1, lo_hi1, 100))


@pytest.mark.parametrize("nseg", [0, 1])
def test_identical_rows_land_in_one_bin(lib, nseg):
    """70001 equal rows: one bin holds 70001 (more than 16 bits, and every atomic of the pass on one address)."""
    n, bins = 70001, 100
    x = np.tile(np.array([[0.25, -3.0, 7.5]]), (n, 1))
    lo_hi = np.array([[0.0, 1.0], [-4.0, 4.0], [7.5, 8.0]])
    edges = mr.edges_of(lo_hi, bins)
    idx = _bin(lib, torch.from_numpy(x).to(DEV), edges)
    h1, h2 = _hist(lib, idx, bins, ms.all_pairs(3), nseg=nseg)
    np.testing.assert_array_equal(h1, mr.hist1(x, lo_hi, bins))
    np.testing.assert_array_equal(h2, mr.hist2(x, lo_hi, bins, ms.all_pairs(3)))
    assert (h1 == n).sum() == 3 and h1.sum() == 3 * n and (h2 == n).sum() == 3 and h2.sum() == 3 * n
    w = torch.full((n,), 0.7, dtype=torch.float64, device=DEV)
    g1, g2 = _hist(lib, idx, bins, ms.all_pairs(3), w=w, w_max=0.7, nseg=nseg)
    s = mr.fixed_point_shift(n)
    assert (g1 == n * 2**s).sum() == 3 and (g1 != 0).sum() == 3 and (g2 == n * 2**s).sum() == 3 and (g2 != 0).sum() == 3


@pytest.mark.parametrize("n,ndim,bins,decades", [(1000, 3, 20, 0.0), (4097, 2, 128, 60.0), (70001, 5, 100, 0.0), (70001, 3, 128, 60.0)])
def test_weighted_sums_meet_the_fixed_point_bound(lib, n, ndim, bins, decades):
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type"
    x, lo_hi = ms.inputs(n, ndim, bins, seed=n + bins)
    w = ms.lognormal_weights(n, n + ndim, decades=decades)
    w[:: 7] = 0.0  # zero weights are legal and count nothing
    edges = mr.edges_of(lo_hi, bins)
    idx = _bin(lib, torch.from_numpy(x).to(DEV), edges)
    want_idx = mr.bin_indices(x, edges)
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    pairs = ms.all_pairs(ndim)
    w_max = float(w.max())
    q1, q2 = _hist(lib, idx, bins, pairs, w=torch.from_numpy(w).to(DEV), w_max=w_max)
    scale = np.ldexp(w_max, -mr.fixed_point_shift(n))
    r1, c1, r2, c2 = mr.weighted_hists(want_idx, w, bins, pairs)
    worst = 0.0
    for got, ref, cnt in ((q1, r1, c1), (q2, r2, c2)):
        assert (got >= 0).all()
        err = np.abs((got.astype(np.float64) * scale).astype(LD) - ref)
        bound = mr.fixed_point_bound(cnt, ref, w_max, n)
        assert np.all(got[cnt == 0] == 0)
        live = cnt > 0
        if live.any():
            worst = max(worst, float(np.max(err[live] / bound[live])))
        assert np.all(err <= bound)
    print(f"n={n} ndim={ndim} bins={bins} decades={decades}: largest error / bound {worst:.3g}")
    # and the integers themselves are the kernel's rule restated: rint(w / w_max * 2^s) summed per bin
    q = np.rint(w / w_max * 2.0 ** mr.fixed_point_shift(n)).astype(np.int64)
    acc = np.zeros((ndim, bins), dtype=np.int64)
    for c in range(ndim):
        ok = want_idx[:, c] != mr.NOT_COUNTED
        np.add.at(acc[c], want_idx[ok, c], q[ok])
    np.testing.assert_array_equal(q1, acc)


@pytest.mark.parametrize("weighted", [False, True])
def test_same_bits_for_any_repetition_geometry_and_row_order(lib, weighted):
    n, ndim, bins = 70001, 3, 100
    x, lo_hi = ms.inputs(n, ndim, bins, seed=21)
    w = ms.lognormal_weights(n, 22) if weighted else None
    edges = mr.edges_of(lo_hi, bins)
    pairs = ms.all_pairs(ndim)

    def run(xa, wa, nseg):
        idx = _bin(lib, torch.from_numpy(np.ascontiguousarray(xa)).to(DEV), edges)
        if wa is None:
            return idx.cpu().numpy(), _hist(lib, idx, bins, pairs, nseg=nseg)
        return idx.cpu().numpy(), _hist(lib, idx, bins, pairs, w=torch.from_numpy(np.ascontiguousarray(wa)).to(DEV),
                                        w_max=float(w.max()), nseg=nseg)

    idx0, (h1, h2) = run(x, w, 0)
    assert h1.sum() > 0 and h2.sum() > 0
    for rep in range(2):  # three runs in all
        idx_r, (a1, a2) = run(x, w, 0)
        np.testing.assert_array_equal(idx_r, idx0)
        np.testing.assert_array_equal(a1, h1)
        np.testing.assert_array_equal(a2, h2)
    for nseg in (1, 3, 64, 65536):
        _, (a1, a2) = run(x, w, nseg)
        np.testing.assert_array_equal(a1, h1, err_msg=f"n_segments = {nseg}")
        np.testing.assert_array_equal(a2, h2, err_msg=f"n_segments = {nseg}")
    perm = np.random.default_rng(23).permutation(n)
    idx_p, (a1, a2) = run(x[perm], None if w is None else w[perm], 0)
    np.testing.assert_array_equal(idx_p, idx0[perm])
    np.testing.assert_array_equal(a1, h1)
    np.testing.assert_array_equal(a2, h2)


def test_invalid_arguments_launch_nothing(lib):
    L, so = lib
    n, ndim, bins = 100, 3, 20
    x = torch.zeros((n, ndim), dtype=torch.float64, device=DEV)
    edges = torch.from_numpy(mr.edges_of(np.array([[-1.0, 1.0]] * ndim), bins)).to(DEV)
    idx = torch.full((n * ndim + PAD,), IDX_SENTINEL, dtype=torch.uint8, device=DEV)
    st = _stream()
    bad_bin = [(0, ndim, bins), (-1, ndim, bins), (2**31, ndim, bins), (n, 0, bins), (n, 17, bins), (n, ndim, 0), (n, ndim, 129)]
    for nn, nd, nb in bad_bin:
        assert so.cf_marg_bin(x.data_ptr(), nn, nd, edges.data_ptr(), nb, idx.data_ptr(), st) == -1, (nn, nd, nb)
    assert so.cf_marg_bin(None, n, ndim, edges.data_ptr(), bins, idx.data_ptr(), st) == -1
    assert so.cf_marg_bin(x.data_ptr(), n, ndim, None, bins, idx.data_ptr(), st) == -1
    assert so.cf_marg_bin(x.data_ptr(), n, ndim, edges.data_ptr(), bins, None, st) == -1
    with pytest.raises(L.CosmofitError, match="CF_ERR_INVALID"):
        L.check(so.cf_marg_bin(x.data_ptr(), n, ndim, edges.data_ptr(), 129, idx.data_ptr(), st))
    torch.cuda.synchronize()
    assert bool((idx == IDX_SENTINEL).all()), "a refused cf_marg_bin wrote indices"

    good = torch.zeros((n, ndim), dtype=torch.uint8, device=DEV)
    w = torch.ones(n, dtype=torch.float64, device=DEV)
    h1 = torch.full((ndim * bins + PAD,), H_SENTINEL, dtype=torch.int64, device=DEV)
    h2 = torch.full((3 * bins * bins + PAD,), H_SENTINEL, dtype=torch.int64, device=DEV)
    pr = np.array([(1, 0), (2, 0), (2, 1)], dtype=np.int32)
    pp = lambda a: a.ctypes.data_as(C.c_void_p)

    def hist(idx_p=good.data_ptr(), w_p=None, w_max=0.0, nn=n, nd=ndim, nb=bins, pairs=pr, npairs=3, h1_p=h1.data_ptr(),
             h2_p=h2.data_ptr(), nseg=0):
        return so.cf_marg_hist(idx_p, w_p, w_max, nn, nd, nb, None if pairs is None else pp(pairs), npairs, h1_p, h2_p, nseg, st)

    for nn, nd, nb in bad_bin:
        assert hist(nn=nn, nd=nd, nb=nb) == -1, (nn, nd, nb)
    assert hist(idx_p=None) == -1 and hist(h1_p=None) == -1 and hist(h2_p=None) == -1 and hist(pairs=None) == -1
    assert hist(npairs=-1) == -1 and hist(npairs=257) == -1
    assert hist(nseg=-1) == -1 and hist(nseg=65537) == -1
    for bad in (np.array([(1, 0), (3, 0), (2, 1)], dtype=np.int32), np.array([(1, 0), (2, -1), (2, 1)], dtype=np.int32)):
        assert hist(pairs=bad) == -1
    for w_max in (0.0, -1.0, float("nan"), float("inf")):
        assert hist(w_p=w.data_ptr(), w_max=w_max) == -1, w_max
    torch.cuda.synchronize()
    assert bool((h1 == H_SENTINEL).all()) and bool((h2 == H_SENTINEL).all()), "a refused cf_marg_hist wrote histograms"
    assert hist() == 0 and hist(w_p=w.data_ptr(), w_max=1.0) == 0 and hist(pairs=None, npairs=0, h2_p=None) == 0
    torch.cuda.synchronize()
    assert int(h1[0]) == n  # the last call: every index 0, unweighted
