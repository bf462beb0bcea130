"""GPU (-m gpu): cf_gp_mll_device / cf_gp_predict_device (csrc/cosmofit_gp.hip) called directly on torch buffers, as gp.py
calls them.  The judge is the long-double restatement (tests/gp_reference.py), computed once per data size
(``gp_shapes.reference``); tests/test_gp_cpu.py holds scipy's float64 path within 1e-11 of it on these very draws.

Bars (the project's 1e-10): log ML, r^T K^-1 r and log|K| relative; the five predictive columns relative to max |mean| over
the test points, s_f^2, max |dmean|, s_f^2 / l^2 and s_f^2 / l (the variances are differences of near-equal numbers: a bar
relative to the variance itself would test the conditioning, not the kernel).

What fixed-order sums promise is asserted exactly: a row has the same bits alone, at every W / S, at every position and
beside rows that are not evaluated; every output buffer is followed by a sentinel that must survive.  Every test prints the
largest error it saw (``-s`` shows them; profiles/NOTES_gp.md quotes them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gp_reference as R
import gp_shapes as GS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = R.LD
SENTINEL = -7.25e300
PAD = 64
BAR = 1e-10


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg._lib, pkg.lib()


def _make(lib, z, y, cov, bounds):
    L, so = lib
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (z, y, cov, bounds)]
    d = L.cf_gp_desc()
    d.struct_size, d.device, d.n = C.sizeof(L.cf_gp_desc), 0, len(arrs[0])
    d.z, d.y, d.cov, d.bounds = (a.ctypes.data for a in arrs)
    h = C.c_void_p()
    L.check(so.cf_gp_create(C.byref(d), C.byref(h)))
    return h


@pytest.fixture(scope="module")
def handles(lib):
    cache = {}

    def get(n):
        if n not in cache:
            z, y, cov, b = GS.data(n)[:4]
            cache[n] = _make(lib, z, y, cov, b)
        return cache[n]

    yield get
    for h in cache.values():
        lib[1].cf_gp_destroy(h)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _failed(lib, h):
    i = lib[0].cf_gp_info()
    lib[0].check(lib[1].cf_gp_get_info(h, C.byref(i)))
    return i.failed_factorizations


def _mll(lib, h, theta, parts=True):
    """cf_gp_mll_device into buffers PAD longer than [W] / [W, 2]: numpy (out [W], parts [W, 2]); the tails keep their sentinel."""
    L, so = lib
    W = theta.shape[0]
    dth = torch.from_numpy(np.ascontiguousarray(theta)).to(DEV)
    out = torch.full((W + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    prt = torch.full((2 * W + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_gp_mll_device(h, dth.data_ptr(), W, out.data_ptr(), prt.data_ptr() if parts else None, _stream()))
    o, p = out.cpu().numpy(), prt.cpu().numpy()
    assert (o[W:] == SENTINEL).all(), "cf_gp_mll_device wrote outside its [W] block"
    assert (p[2 * W if parts else 0:] == SENTINEL).all(), "cf_gp_mll_device wrote outside its [W, 2] block"
    return o[:W], p[: 2 * W].reshape(W, 2)


def _predict(lib, h, theta, zs, noise):
    L, so = lib
    S, nz = theta.shape[0], len(zs)
    dth = torch.from_numpy(np.ascontiguousarray(theta)).to(DEV)
    dz = torch.from_numpy(np.ascontiguousarray(zs, dtype=np.float64)).to(DEV)
    buf = torch.full((S * nz * 5 + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_gp_predict_device(h, dth.data_ptr(), S, dz.data_ptr(), nz, float(noise), buf.data_ptr(), _stream()))
    o = buf.cpu().numpy()
    assert (o[S * nz * 5:] == SENTINEL).all(), "cf_gp_predict_device wrote outside its [S, nz, 5] block"
    return o[: S * nz * 5].reshape(S, nz, 5)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("n", GS.N_SET)
def test_mll_and_parts_match_the_restatement_at_every_batch_size(lib, handles, n):
    h = handles(n)
    ref = GS.reference(n)[0]  # [N_BASE, 3]
    base_out, base_parts = _mll(lib, h, GS.thetas(n, GS.N_BASE))
    got = np.column_stack([base_out, base_parts]).astype(LD)
    rel = np.max(np.abs(got - ref) / np.abs(ref), axis=0).astype(np.float64)
    print(f"n={n}: max rel err log ML {rel[0]:.2e}, r^T K^-1 r {rel[1]:.2e}, log|K| {rel[2]:.2e}")
    assert np.isfinite(base_out).all()
    assert rel.max() < BAR
    for W in GS.ROWS_SET:
        idx = GS.row_index(W)
        out, parts = _mll(lib, h, GS.thetas(n, W))
        assert _same_bits(out, base_out[idx]) and _same_bits(parts, base_parts[idx]), f"W={W}: a row's bits moved"
        out_only, _ = _mll(lib, h, GS.thetas(n, W), parts=False)
        assert _same_bits(out_only, out)
    for i in (0, 17, 64):  # alone
        out, parts = _mll(lib, h, GS.base_thetas(n)[i:i + 1])
        assert _same_bits(out, base_out[i:i + 1]) and _same_bits(parts, base_parts[i:i + 1])
    assert _failed(lib, h) == 0


@pytest.mark.parametrize("n", GS.N_SET)
def test_predictions_match_the_restatement_at_every_shape(lib, handles, n):
    h = handles(n)
    ref = GS.reference(n)[1]  # [N_BASE, NZ_FULL, 5]
    th = GS.base_thetas(n)
    worst = np.zeros(5)
    by_nz = {}
    for nz in GS.NZ_SET:
        zs = GS.z_star(n, nz)
        base = _predict(lib, h, GS.thetas(n, GS.N_BASE), zs, GS.TEST_NOISE)
        assert np.isfinite(base).all()
        for i in range(GS.N_BASE):
            worst = np.maximum(worst, R.scaled_errors(base[i], ref[i, :nz], th[i]).astype(np.float64))
        by_nz[nz] = base
        for S in GS.ROWS_SET:
            got = _predict(lib, h, GS.thetas(n, S), zs, GS.TEST_NOISE)
            assert _same_bits(got, base[GS.row_index(S)]), f"S={S}, nz={nz}: a row's bits moved"
    # a test point's bits do not depend on the other test points either
    assert _same_bits(by_nz[1], by_nz[130][:, :1]) and _same_bits(by_nz[64], by_nz[65][:, :64])
    print(f"n={n}: max scaled err mean {worst[0]:.2e}, var {worst[1]:.2e}, dmean {worst[2]:.2e}, dvar {worst[3]:.2e}, "
          f"cov {worst[4]:.2e}; smallest var / s_f^2 {float(np.min(ref[:, :, 1] / th[:, None, 1])):.1e}")
    assert worst.max() < BAR


@pytest.mark.parametrize("n", (2, 38, 64))
def test_rows_that_are_not_evaluated_leave_their_neighbours_alone(lib, handles, n):
    h = handles(n)
    good, bad = GS.thetas(n, 40), GS.bad_rows(n)
    zs = GS.z_star(n, 7)
    clean_out, clean_parts = _mll(lib, h, good)
    clean_pred = _predict(lib, h, good, zs, 0.0)
    rows, is_bad = [], []
    for k in range(max(len(good), len(bad))):  # interleaved, a bad row first
        if k < len(bad):
            rows.append(bad[k]); is_bad.append(True)
        if k < len(good):
            rows.append(good[k]); is_bad.append(False)
    rows, is_bad = np.array(rows), np.array(is_bad)
    out, parts = _mll(lib, h, rows)
    assert (out[is_bad] == -np.inf).all() and np.isnan(parts[is_bad]).all()
    assert not np.isnan(out).any()
    assert _same_bits(out[~is_bad], clean_out) and _same_bits(parts[~is_bad], clean_parts)
    pred = _predict(lib, h, rows, zs, 0.0)
    assert np.isnan(pred[is_bad]).all()
    assert _same_bits(pred[~is_bad], clean_pred)
    # a non-finite test redshift is NaN at that point only
    zbad = zs.copy()
    zbad[[1, 4, 6]] = np.nan, np.inf, -np.inf
    pz = _predict(lib, h, good, zbad, 0.0)
    assert np.isnan(pz[:, [1, 4, 6]]).all() and _same_bits(pz[:, [0, 2, 3, 5]], clean_pred[:, [0, 2, 3, 5]])
    assert _failed(lib, h) == 0  # none of this is a failed factorisation


def test_negative_definite_noise_fails_every_factorisation_and_is_counted(lib):
    """C = -10 I with s_f^2 < 0.4 and s > 0.05: the first pivot s_f^2 - 10 s is negative for every row of the box.  Finite
    arithmetic: every row is -inf, and the device counter equals the row count."""
    n, W = 17, 65
    z = np.linspace(0.1, 1.9, n)
    b = np.array([[-2.0, 2.0], [0.05, 0.4], [2.0, 6.0], [0.05, 4.0]])
    h = _make(lib, z, np.sin(z), -10.0 * np.eye(n), b)
    try:
        th = b[:, 0] + np.random.default_rng(3).uniform(0.02, 0.98, (W, 4)) * (b[:, 1] - b[:, 0])
        assert _failed(lib, h) == 0
        out, parts = _mll(lib, h, th)
        assert (out == -np.inf).all() and np.isnan(parts).all()
        assert _failed(lib, h) == W
        assert np.isnan(_predict(lib, h, th, np.array([0.0, 0.5, 1.0]), 0.0)).all()
        assert _failed(lib, h) == W  # the counter is the log-ML entry's
    finally:
        lib[1].cf_gp_destroy(h)


def test_test_noise_enters_scaled_by_the_noise_scale(lib, handles):
    n = 38
    h = handles(n)
    th, zs = GS.thetas(n, 33), GS.z_star(n, 11)
    p0, p1 = _predict(lib, h, th, zs, 0.0), _predict(lib, h, th, zs, 0.25)
    assert _same_bits(p0[:, :, [0, 2, 3, 4]], p1[:, :, [0, 2, 3, 4]])
    want = th[:, None, 3] * 0.25
    assert np.max(np.abs((p1[:, :, 1] - p0[:, :, 1]) - want) / th[:, None, 1]) < 1e-15 * 4
    with pytest.raises(lib[0].CosmofitError, match="noise must be finite"):
        _predict(lib, h, th, zs, -1.0)
    with pytest.raises(lib[0].CosmofitError, match="nz must be"):
        lib[0].check(lib[1].cf_gp_predict_device(h, 1, 1, 1, 0, 0.0, 1, None))


def test_host_twins_give_the_device_entries_bits(lib, handles):
    L, so = lib
    n = 38
    h = handles(n)
    th, zs = GS.thetas(n, 257), GS.z_star(n, 63)
    out_d, parts_d = _mll(lib, h, th)
    pred_d = _predict(lib, h, th, zs, GS.TEST_NOISE)
    out, parts, pred = np.empty(257), np.empty((257, 2)), np.empty((257, 63, 5))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(so.cf_gp_mll(h, p(th), 257, p(out), p(parts)))
    L.check(so.cf_gp_predict(h, p(th), 257, p(zs), 63, GS.TEST_NOISE, p(pred)))
    assert _same_bits(out, out_d) and _same_bits(parts, parts_d) and _same_bits(pred, pred_d)
    L.check(so.cf_gp_mll(h, p(th), 0, None, None))  # zero rows: a no-op


def test_cf_gp_mll_beyond_one_piece_gives_the_device_entrys_bits(lib, handles):
    """cf_gp_mll stages its rows through the device in pieces of 16384: one row more crosses one boundary, so the second
    piece's row is read from behind the first's and its out / parts land behind them.  n = 1 keeps it cheap."""
    L, so = lib
    n, piece = 1, 16384
    h = handles(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    W = piece + 1
    th = GS.thetas(n, W)
    out, parts = np.full(W, SENTINEL), np.full((W, 2), SENTINEL)
    L.check(so.cf_gp_mll(h, p(th), W, p(out), p(parts)))
    out_d, parts_d = _mll(lib, h, th)
    assert np.isfinite(out).all() and np.isfinite(parts).all() and (out != SENTINEL).all() and (parts != SENTINEL).all()
    assert _same_bits(out, out_d) and _same_bits(parts, parts_d)
    assert _failed(lib, h) == 0


def test_cf_gp_predict_beyond_one_piece_gives_the_device_entrys_bits(lib, handles):
    """As above for cf_gp_predict at the largest nz of these tests: the smallest S beyond one piece of 16384 * 256 / (5 nz) rows."""
    L, so = lib
    n, piece, nz = 1, 16384, GS.NZ_FULL
    h = handles(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    S = max(1, piece * 256 // (nz * 5)) + 1
    th, zs = GS.thetas(n, S), GS.z_star(n, nz)
    pred = np.full((S, nz, 5), SENTINEL)
    L.check(so.cf_gp_predict(h, p(th), S, p(zs), nz, GS.TEST_NOISE, p(pred)))
    assert np.isfinite(pred).all() and (pred != SENTINEL).all()
    assert _same_bits(pred, _predict(lib, h, th, zs, GS.TEST_NOISE))
    assert _failed(lib, h) == 0


def test_row_counts_beyond_one_grid_are_launched_in_pieces(lib, handles):
    """Rows are launched as grids of at most 2^22 workgroups: a batch one row longer than that takes a second grid.  n = 1
    keeps it cheap; the rows on either side of the seam and the last one carry the bits they have alone."""
    L, so = lib
    n, W = 1, (1 << 22) + 1
    h = handles(n)
    base = GS.base_thetas(n)
    idx = np.arange(W) % GS.N_BASE
    dth = torch.from_numpy(base).to(DEV)[torch.from_numpy(idx).to(DEV)].contiguous()
    out = torch.full((W + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    prt = torch.full((2 * W + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_gp_mll_device(h, dth.data_ptr(), W, out.data_ptr(), prt.data_ptr(), _stream()))
    want_out, want_parts = _mll(lib, h, base)
    want_o = torch.from_numpy(want_out).to(DEV)[torch.from_numpy(idx).to(DEV)]
    want_p = torch.from_numpy(want_parts).to(DEV)[torch.from_numpy(idx).to(DEV)].reshape(-1)
    assert bool((out[:W].view(torch.int64) == want_o.view(torch.int64)).all())
    assert bool((prt[: 2 * W].view(torch.int64) == want_p.view(torch.int64)).all())
    assert bool((out[W:] == SENTINEL).all()) and bool((prt[2 * W:] == SENTINEL).all())
    zs = torch.tensor([0.0, 1.0], dtype=torch.float64, device=DEV)
    buf = torch.full((W * 10 + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_gp_predict_device(h, dth.data_ptr(), W, zs.data_ptr(), 2, 0.0, buf.data_ptr(), _stream()))
    want = torch.from_numpy(_predict(lib, h, base, np.array([0.0, 1.0]), 0.0)).to(DEV)[torch.from_numpy(idx).to(DEV)].reshape(-1)
    assert bool((buf[: W * 10].view(torch.int64) == want.view(torch.int64)).all()) and bool((buf[W * 10:] == SENTINEL).all())
