"""GPU (-m gpu): the two kernels of the scaled covariance (csrc/cosmofit_cscale.hip) through the handle-free
``cf_cscale_apply_device``, at the shapes they accept: n around the k step, the 16-wide tile, the 32-wide slab and the 64-wide
block, S around a row tile and a row block, 1 to 16 amplitudes per row, five kinds of second matrix -- against the long-double
restatement (tests/cscale_reference.py: factor C0 + s C1, substitute); the bits of (row, s_j) wherever it is computed; what lies
in the padding of the rows and beyond row S; the domain rules."""
import ctypes as C

import numpy as np
import pytest
import torch

import cscale_reference as CR
import cscale_shapes as CS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def V(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.covscale


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Apply:
    """One (n, kind): the decomposition on the device, 257 residual rows in a padded buffer, 16 amplitudes per row (the same 16,
    rotated by the row), the restatement for them and the device's results for all rows in one call -- computed once and shared."""

    def __init__(self, pkg, V, n, kind):
        self.n, self.kind = n, kind
        cov = CS.covariance(pkg, n)
        self.chol = np.linalg.cholesky(cov)
        c1 = CS.second_matrix(kind, cov)
        self.T, self.lam, self.info = V.decompose(self.chol, c1)
        self.dec = V.Decomposition(self.T, self.lam, device=0)
        self.rows = CS.residual_rows(self.chol, CS.S_MAX, seed=n)
        self.pitch = (n + 64) // 64 * 64  # at least one column of padding, as the residual rows of an engine have
        self.buf = torch.zeros((CS.S_MAX + 3, self.pitch), dtype=torch.float64, device=DEV)
        self.buf[:CS.S_MAX, :n] = _dev(self.rows)
        self.base = CS.amplitudes(self.info)
        self.s, idx = CS.per_row(self.base, CS.S_MAX)
        quad, logdet = CR.quad_logdet(self.chol, c1, self.rows, self.base)
        q_scale, l_scale = CR.scales(self.T, self.lam, self.rows, self.base)
        r = np.arange(CS.S_MAX)[:, None]
        self.q_ref, self.q_tol = quad[r, idx], CR.BAR * q_scale[r, idx]
        self.l_ref, self.l_tol = logdet[idx], CR.BAR * l_scale[idx]
        self.y_ref = np.asarray(self.rows, dtype=CR.LD) @ np.asarray(self.T, dtype=CR.LD).T
        self.y_tol = CR.BAR * (np.abs(self.rows) @ np.abs(self.T).T)
        self.sd = _dev(self.s)
        q, ld, y = self.dec.apply(self.buf, self.sd, S=CS.S_MAX, want_y=True)
        self.q, self.ld, self.y = q.cpu().numpy(), ld.cpu().numpy(), y.cpu().numpy()

    def call(self, buf, s, S=None, want_y=False):
        q, ld, y = self.dec.apply(buf, s, S=S, want_y=want_y)
        return q.cpu().numpy(), ld.cpu().numpy(), None if y is None else y.cpu().numpy()


_APPLY = {}


@pytest.fixture(scope="module", params=[(n, k) for n in CS.N_ALL for k in CS.KINDS], ids=lambda p: "%d-%s" % p)
def ap(request, pkg, V):
    if request.param not in _APPLY:
        _APPLY[request.param] = Apply(pkg, V, *request.param)
    return _APPLY[request.param]


def _worst(err, tol):
    err = np.asarray(err, dtype=np.float64)
    live = tol > 0
    assert not err[~live].any()  # a zero scale is a zero row or s = 0: exact
    return float(np.max(err[live] / tol[live])) * CR.BAR if live.any() else 0.0


def test_apply_agrees_with_the_restatement_over_shapes(ap):
    worst_q = worst_l = 0.0
    for S in CS.S_ALL:
        for n_s in CS.NS_ALL:
            q, ld, _ = ap.call(ap.buf, ap.sd[:S, :n_s].contiguous(), S=S)
            assert q.shape == ld.shape == (S, n_s)
            eq, el = np.abs(q - ap.q_ref[:S, :n_s]), np.abs(ld - ap.l_ref[:S, :n_s])
            assert (eq <= ap.q_tol[:S, :n_s]).all() and (el <= ap.l_tol[:S, :n_s]).all(), (ap.n, ap.kind, S, n_s)
            worst_q, worst_l = max(worst_q, _worst(eq, ap.q_tol[:S, :n_s])), max(worst_l, _worst(el, ap.l_tol[:S, :n_s]))
            # (row, s_j) does not depend on S, on n_s or on the other amplitudes of its row
            assert np.array_equal(_bits(q), _bits(ap.q[:S, :n_s])) and np.array_equal(_bits(ld), _bits(ap.ld[:S, :n_s])), (ap.n, S, n_s)
    ey = np.abs(ap.y - ap.y_ref)
    assert (ey <= ap.y_tol).all()
    print("n = %d, %s: quad %.2e, logdet %.2e, y %.2e of the scale of the terms summed"
          % (ap.n, ap.kind, worst_q, worst_l, _worst(ey, ap.y_tol)))
    assert not ap.rows[2].any() and not ap.q[2].any() and not ap.y[2].any()  # a zero row gives exact zeros


def test_bits_do_not_depend_on_position_y_stream_or_repetition(ap):
    want_q, want_l = _bits(ap.q), _bits(ap.ld)
    for p in CS.POSITIONS:
        q, ld, _ = ap.call(ap.buf[p:p + 1], ap.sd[p:p + 1])
        assert np.array_equal(_bits(q), want_q[p:p + 1]) and np.array_equal(_bits(ld), want_l[p:p + 1]), (ap.n, "row", p)
    perm = np.random.default_rng(ap.n).permutation(CS.S_MAX)
    pd = torch.from_numpy(perm).to(DEV)
    q, ld, y = ap.call(ap.buf[:CS.S_MAX][pd].contiguous(), ap.sd[pd].contiguous(), want_y=True)
    assert np.array_equal(_bits(q), want_q[perm]) and np.array_equal(_bits(ld), want_l[perm]), (ap.n, "permuted")
    assert np.array_equal(_bits(y), _bits(ap.y)[perm])
    q, ld, _ = ap.call(ap.buf, ap.sd, S=CS.S_MAX)  # repeated, and without y
    assert np.array_equal(_bits(q), want_q) and np.array_equal(_bits(ld), want_l), (ap.n, "repeated, y not stored")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        q, ld, y = ap.dec.apply(ap.buf, ap.sd, S=CS.S_MAX, want_y=True)
    side.synchronize()
    assert np.array_equal(_bits(q.cpu().numpy()), want_q) and np.array_equal(_bits(ld.cpu().numpy()), want_l), (ap.n, "second stream")
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(ap.y))
    torch.cuda.synchronize()


def test_padding_nan_rows_and_rows_beyond_s(pkg, ap):
    n, S, n_s = ap.n, 200, 5
    s = ap.sd[:, :n_s].contiguous()
    # NaN in the pad columns and in every row >= S (amplitudes included); the outputs padded too, their further rows untouched
    buf = ap.buf.clone()
    buf[:, n:] = float("nan")
    buf[S:, :] = float("nan")
    sbad = torch.cat([s, torch.full((3, n_s), float("nan"), dtype=torch.float64, device=DEV)])
    sbad[S:] = float("nan")
    q = torch.full((S + 2, n_s), -7.0, dtype=torch.float64, device=DEV)
    ld, y = q.clone(), torch.full((S + 2, n), -7.0, dtype=torch.float64, device=DEV)
    pkg._lib.check(pkg.lib().cf_cscale_apply_device(ap.dec._p, buf.data_ptr(), ap.pitch, S, sbad.data_ptr(), n_s, q.data_ptr(),
                                                    ld.data_ptr(), y.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream))
    q, ld, y = q.cpu().numpy(), ld.cpu().numpy(), y.cpu().numpy()
    assert np.array_equal(_bits(q[:S]), _bits(ap.q[:S, :n_s])) and np.array_equal(_bits(ld[:S]), _bits(ap.ld[:S, :n_s]))
    assert np.array_equal(_bits(y[:S]), _bits(ap.y[:S]))
    assert (q[S:] == -7.0).all() and (ld[S:] == -7.0).all() and (y[S:] == -7.0).all()
    # NaN and inf in one row stay in that row
    buf = ap.buf.clone()
    buf[17, 0] = float("nan")
    buf[90, n - 1] = float("inf")
    q, ld, y = ap.call(buf, s[:S].contiguous(), S=S, want_y=True)
    bad = np.zeros(S, dtype=bool)
    bad[[17, 90]] = True
    assert np.isnan(q[17]).all() and not np.isfinite(q[90]).any() and not np.isfinite(y[17]).any()
    assert np.array_equal(_bits(q[~bad]), _bits(ap.q[:S, :n_s][~bad])) and np.array_equal(_bits(y[~bad]), _bits(ap.y[:S][~bad]))
    assert np.array_equal(_bits(ld), _bits(ap.ld[:S, :n_s]))  # logdet does not read the rows


def test_domain_and_special_values_stay_in_their_place(pkg, ap):
    S = 65
    s = ap.s[:S].copy()
    lo, hi = ap.info["s_min"], ap.info["s_max"]
    planted = {(3, 0): np.nan, (16, 15): np.inf, (40, 7): -np.inf}
    if np.isfinite(lo):
        planted[(0, 1)] = lo * (1 + 1e-12)
        planted[(64, 9)] = 3 * lo
    if np.isfinite(hi):
        planted[(31, 4)] = hi * (1 + 1e-12)
    for (i, j), v in planted.items():
        s[i, j] = v
    q, ld, _ = ap.call(ap.buf, _dev(s), S=S)
    mask = np.zeros((S, CS.MAX_S), dtype=bool)
    for (i, j) in planted:
        mask[i, j] = True
    assert np.isnan(q[mask]).all() and np.isnan(ld[mask]).all(), (ap.n, ap.kind)
    assert np.array_equal(_bits(q[~mask]), _bits(ap.q[:S][~mask])) and np.array_equal(_bits(ld[~mask]), _bits(ap.ld[:S][~mask]))
    # s = 0: logdet exactly 0.0 and quad = sum_k y_k^2 in the kernel's order (the host twin runs the same order on the device's y)
    zero = ap.s == 0.0
    assert zero.sum() == CS.S_MAX and not ap.ld[zero].any() and not np.signbit(ap.ld[zero]).any()
    L = pkg._lib
    for i in (0, 1, 100, 256):
        hq, hl = np.empty(CS.MAX_S), np.empty(CS.MAX_S)
        yi, si = np.ascontiguousarray(ap.y[i]), np.ascontiguousarray(ap.s[i])
        L.check(pkg.lib().cf_selftest_cscale_host(yi.ctypes.data, ap.lam.ctypes.data, ap.n, si.ctypes.data, CS.MAX_S, hq.ctypes.data,
                                                  hl.ctypes.data))
        assert np.array_equal(_bits(hq), _bits(ap.q[i])), (ap.n, ap.kind, i)  # the same operations in the same order
        assert (np.abs(hl - ap.ld[i]) <= ap.l_tol[i]).all()                   # log1p is each side's own
        j0 = int(np.flatnonzero(zero[i])[0])
        assert abs(ap.q[i, j0] - float(np.sum(yi * yi))) <= 4 * ap.n * CR.EPS * ap.q[i, j0]


def test_apply_refuses_bad_arguments(pkg, ap):
    lib, p = pkg.lib(), ap.dec._p
    q = torch.empty((4, 2), dtype=torch.float64, device=DEV)
    s = ap.sd[:4, :2].contiguous()
    args = lambda **kw: [kw.get(k, d) for k, d in (("p", p), ("rows", ap.buf.data_ptr()), ("pitch", ap.pitch), ("S", 4),
                                                    ("s", s.data_ptr()), ("n_s", 2), ("q", q.data_ptr()), ("ld", None), ("y", None),
                                                    ("st", None))]
    assert lib.cf_cscale_apply_device(*args()) == 0
    assert lib.cf_cscale_apply_device(*args(pitch=ap.n - 1)) == -1 and b"pitch below n" in lib.cf_last_error()
    assert lib.cf_cscale_apply_device(*args(S=-1)) == -1 and lib.cf_cscale_apply_device(*args(S=2**31)) == -1
    assert lib.cf_cscale_apply_device(*args(n_s=0)) == -1 and lib.cf_cscale_apply_device(*args(n_s=17)) == -1
    assert lib.cf_cscale_apply_device(*args(q=None)) == -1 and b"no output" in lib.cf_last_error()
    assert lib.cf_cscale_apply_device(*args(rows=None)) == -1 and lib.cf_cscale_apply_device(*args(s=None)) == -1
    assert lib.cf_cscale_apply_device(*args(S=0, rows=None, s=None)) == 0
    n, dev = C.c_int64(), C.c_int32(-1)
    assert lib.cf_cscale_look(p, C.byref(n), C.byref(dev)) == 0 and n.value == ap.n and dev.value == 0
    torch.cuda.synchronize()
