"""GPU (-m gpu): the two kernels of the closed-form nuisance treatment (csrc/cosmofit_marg.hip) through the handle-free
``cf_marg_apply_device`` on planted rows, at the shapes they accept: n around the k step, the 16-wide tile, the 64-wide staged
tile and the 256-wide k slice, 1 to 16 components, S around a row tile and a workgroup's 64 rows -- against the long-double
restatement (tests/marg_reference.py, which never forms Wt); the bits of a row wherever it is computed; what lies in the padding
of the rows and beyond row S; non-finite rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import marg_reference as MR
import marg_shapes as MS
import mock_reference as KR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 5


@pytest.fixture(scope="module")
def N(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.nuisance


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(*xs):
    return tuple(None if x is None else x.cpu().numpy() for x in xs)


class Apply:
    """One (n, m): the projection on the device, 257 residual rows in a padded buffer, the normals of ``recover``, the
    restatement for the rows and the device's results for all rows in one call -- computed once and shared."""

    def __init__(self, pkg, N, n, m):
        self.n, self.m = n, m
        self.chol = np.linalg.cholesky(MS.covariance(pkg, n))
        self.A = MS.width(n, m)
        self.mu, self.sigma, self.box = MS.prior(MS.PRIORS[(n + m) % 3], n, m)
        self.proj = N.project(self.chol, self.A, self.mu, self.sigma, self.box)
        self.dec = N.Projection(self.proj, device=0)
        self.rows = MS.residual_rows(self.chol, MS.S_MAX, seed=n)
        self.pitch = (n + 64) // 64 * 64  # at least one column of padding, as the residual rows of an engine have
        self.buf = torch.zeros((MS.S_MAX + 3, self.pitch), dtype=torch.float64, device=DEV)
        self.buf[:MS.S_MAX, :n] = _dev(self.rows)
        self.key = N.recover_key(SEED)
        self.xid = pkg.mocks.normals(self.key, MS.S_MAX, m, k0=0, device=DEV)
        self.xi = self.xid.cpu().numpy()
        ref = MR.restate(self.chol, self.A, self.rows, self.mu, self.sigma, self.box)
        self.t_ref, self.q_ref, self.a_ref = ref["t"], ref["q"], ref["alpha_hat"]
        self.xi_ref = KR.normals(self.key, 0, MS.S_MAX, m)
        self.shift_ref = MR.solve_upper_t(ref["LF"], self.xi_ref.T).T  # U^-1 xi
        chi2_0 = np.asarray(ref["chi2_0"], dtype=np.float64)
        t_scale, v_scale, a_scale = MR.scales(self.proj, self.rows, chi2_0, xi=self.xi)
        self.t_tol, self.q_tol, self.a_tol = MR.BAR * t_scale, MR.BAR * v_scale, MR.BAR * a_scale
        self.t, self.q, self.a = _np(*self.dec.apply(self.buf, S=MS.S_MAX))
        self.draw = self.dec.apply(self.buf, S=MS.S_MAX, xi=self.xid, want=("alpha",))[2].cpu().numpy()

    def call(self, buf, S=None, xi=None, want=("t", "q", "alpha")):
        return _np(*self.dec.apply(buf, S=S, xi=xi, want=want))


_APPLY = {}


@pytest.fixture(scope="module", params=[(n, m) for n in MS.N_KERNEL for m in MS.M_KERNEL], ids=lambda p: "%d-%d" % p)
def ap(request, pkg, N):
    if request.param not in _APPLY:
        _APPLY[request.param] = Apply(pkg, N, *request.param)
    return _APPLY[request.param]


def _worst(err, tol):
    err = np.abs(np.asarray(err, dtype=np.float64))
    tol = np.broadcast_to(tol, err.shape)
    live = tol > 0
    assert not err[~live].any()  # a zero scale is a zero row with a zero prior mean: exact
    assert (err[live] <= tol[live]).all(), float(np.max(err[live] / tol[live])) * MR.BAR
    return float(np.max(err[live] / tol[live])) * MR.BAR if live.any() else 0.0


def test_apply_agrees_with_the_restatement_over_shapes(ap):
    worst = dict(t=_worst(ap.t - ap.t_ref, ap.t_tol), q=_worst(ap.q - ap.q_ref, ap.q_tol), alpha=_worst(ap.a - ap.a_ref, ap.a_tol),
                 draw=_worst(ap.draw - (ap.a_ref + ap.shift_ref), ap.a_tol),
                 shift=_worst((ap.draw - ap.a) - ap.shift_ref, ap.a_tol))  # alpha_draw - alpha_hat = U^-1 xi
    print("n = %d, m = %d: " % (ap.n, ap.m) + ", ".join("%s %.2e" % kv for kv in worst.items()) + " of the scale of the terms summed")
    for S in MS.S_KERNEL:
        t, q, a = ap.call(ap.buf, S=S)
        assert t.shape == a.shape == (S, ap.m) and q.shape == (S,)
        # a row does not depend on S
        assert np.array_equal(_bits(t), _bits(ap.t[:S])) and np.array_equal(_bits(q), _bits(ap.q[:S])), (ap.n, ap.m, S)
        assert np.array_equal(_bits(a), _bits(ap.a[:S])), (ap.n, ap.m, S)
        d = ap.call(ap.buf, S=S, xi=ap.xid[:S].contiguous(), want=("alpha",))[2]
        assert np.array_equal(_bits(d), _bits(ap.draw[:S])), (ap.n, ap.m, S, "draw")
    assert not ap.rows[2].any() and np.array_equal(_bits(ap.t[2]), _bits(ap.proj["ct"]))  # a zero row: t = ct exactly


def test_bits_do_not_depend_on_position_outputs_stream_or_repetition(ap):
    want_t, want_q, want_a, want_d = _bits(ap.t), _bits(ap.q), _bits(ap.a), _bits(ap.draw)
    for p in MS.POSITIONS:
        t, q, a = ap.call(ap.buf[p:p + 1])
        assert np.array_equal(_bits(t), want_t[p:p + 1]) and np.array_equal(_bits(q), want_q[p:p + 1]), (ap.n, ap.m, "row", p)
        assert np.array_equal(_bits(a), want_a[p:p + 1]), (ap.n, ap.m, "row", p)
        d = ap.call(ap.buf[p:p + 1], xi=ap.xid[p:p + 1].contiguous(), want=("alpha",))[2]
        assert np.array_equal(_bits(d), want_d[p:p + 1]), (ap.n, ap.m, "row", p, "draw")
    perm = np.random.default_rng(ap.n + ap.m).permutation(MS.S_MAX)
    pd = torch.from_numpy(perm).to(DEV)
    t, q, a = ap.call(ap.buf[:MS.S_MAX][pd].contiguous())
    assert np.array_equal(_bits(t), want_t[perm]) and np.array_equal(_bits(q), want_q[perm]) and np.array_equal(_bits(a), want_a[perm])
    # with and without the optional outputs
    assert np.array_equal(_bits(ap.call(ap.buf, S=MS.S_MAX, want=("t",))[0]), want_t)
    assert np.array_equal(_bits(ap.call(ap.buf, S=MS.S_MAX, want=("q",))[1]), want_q)
    assert np.array_equal(_bits(ap.call(ap.buf, S=MS.S_MAX, want=("alpha",))[2]), want_a)
    t, q, a = ap.call(ap.buf, S=MS.S_MAX)  # repeated
    assert np.array_equal(_bits(t), want_t) and np.array_equal(_bits(q), want_q) and np.array_equal(_bits(a), want_a)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        t, q, a = ap.dec.apply(ap.buf, S=MS.S_MAX, xi=ap.xid)
    side.synchronize()
    t, q, a = _np(t, q, a)
    assert np.array_equal(_bits(t), want_t) and np.array_equal(_bits(q), want_q) and np.array_equal(_bits(a), want_d), "second stream"
    torch.cuda.synchronize()


def test_padding_rows_beyond_s_and_non_finite_rows(pkg, ap):
    n, m, S = ap.n, ap.m, 200
    # NaN in the pad columns and in every row >= S (the normals included); the outputs padded too, their further rows untouched
    buf = ap.buf.clone()
    buf[:, n:] = float("nan")
    buf[S:, :] = float("nan")
    xi = torch.cat([ap.xid, torch.zeros((3, m), dtype=torch.float64, device=DEV)])
    xi[S:] = float("nan")
    t = torch.full((S + 2, m), -7.0, dtype=torch.float64, device=DEV)
    q, a = torch.full((S + 2,), -7.0, dtype=torch.float64, device=DEV), t.clone()
    pkg._lib.check(pkg.lib().cf_marg_apply_device(ap.dec._p, buf.data_ptr(), ap.pitch, S, xi.data_ptr(), t.data_ptr(), q.data_ptr(),
                                                  a.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream))
    t, q, a = _np(t, q, a)
    assert np.array_equal(_bits(t[:S]), _bits(ap.t[:S])) and np.array_equal(_bits(q[:S]), _bits(ap.q[:S]))
    assert np.array_equal(_bits(a[:S]), _bits(ap.draw[:S]))
    assert (t[S:] == -7.0).all() and (q[S:] == -7.0).all() and (a[S:] == -7.0).all()
    # NaN and inf inside a row: that row's outputs are NaN, no other row changes a bit
    buf = ap.buf.clone()
    buf[17, 0] = float("nan")
    buf[90, n - 1] = float("inf")
    buf[91, n // 2] = float("-inf")
    t, q, a = ap.call(buf, S=S)
    bad = np.zeros(S, dtype=bool)
    bad[[17, 90, 91]] = True
    assert np.isnan(t[bad]).all() and np.isnan(q[bad]).all() and np.isnan(a[bad]).all()
    assert np.array_equal(_bits(t[~bad]), _bits(ap.t[:S][~bad])) and np.array_equal(_bits(q[~bad]), _bits(ap.q[:S][~bad]))
    assert np.array_equal(_bits(a[~bad]), _bits(ap.a[:S][~bad]))


def test_apply_refuses_bad_arguments(pkg, N):
    ap = _APPLY.get((65, 3)) or Apply(pkg, N, 65, 3)
    lib, p = pkg.lib(), ap.dec._p
    q = torch.empty((4,), dtype=torch.float64, device=DEV)
    args = lambda **kw: [kw.get(k, d) for k, d in (("p", p), ("rows", ap.buf.data_ptr()), ("pitch", ap.pitch), ("S", 4), ("xi", None),
                                                    ("t", None), ("q", q.data_ptr()), ("a", None), ("st", None))]
    assert lib.cf_marg_apply_device(*args()) == 0
    assert lib.cf_marg_apply_device(*args(pitch=ap.n - 1)) == -1 and b"pitch below n" in lib.cf_last_error()
    assert lib.cf_marg_apply_device(*args(S=-1)) == -1 and lib.cf_marg_apply_device(*args(S=2**31)) == -1
    assert lib.cf_marg_apply_device(*args(q=None)) == -1 and b"no output" in lib.cf_last_error()
    assert lib.cf_marg_apply_device(*args(rows=None)) == -1 and lib.cf_marg_apply_device(*args(S=0, rows=None)) == 0
    n, m, dev, pmu, ln = C.c_int64(), C.c_int32(), C.c_int32(-1), C.c_double(), C.c_double()
    assert lib.cf_marg_info(p, C.byref(n), C.byref(m), C.byref(dev), C.byref(pmu), C.byref(ln)) == 0
    assert (n.value, m.value, dev.value, pmu.value, ln.value) == (ap.n, ap.m, 0, ap.proj["pmu"], ap.proj["log_norm"])
    torch.cuda.synchronize()
