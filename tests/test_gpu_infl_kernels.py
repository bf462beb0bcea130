"""GPU (-m gpu): the two kernels of the attribution (csrc/cosmofit_infl.hip) at the shapes they accept.  ``prec_gemm_kernel``
through the handle-free ``cf_prec_apply_device``: n around the k step, the 16-wide tile and the 64-wide block, S around a row tile
and a row block, against g from two long-double substitutions with the factor; what lies in the padding of the rows and beyond
row S; the bits of a row wherever it is computed.  ``infl_row_kernel`` and the launcher through ``cf_infl_device``: SN engines
around the pitch of the residual rows, one Pantheon+-sized engine, the DESI BAO engine, against the restatement applied to
``engine.parts``' own rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import infl_reference as IR
import infl_shapes as IS
import resid_shapes as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def I(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.influence


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- prec_gemm_kernel through cf_prec_apply_device -----------------------------------------------------------------------------
class Apply:
    """A covariance of n data, its precision matrix on the device, 257 residual rows in a padded buffer, the restatement's g for
    them and the device's g of all rows in one call -- computed once per n and shared."""

    def __init__(self, pkg, I, n):
        self.n = n
        self.chol = np.linalg.cholesky(IS.covariance(pkg, n))
        self.prec = I.Precision(self.chol + np.triu(np.full((n, n), np.nan), 1), device=0)
        self.K = IS.host_precision(pkg._lib, pkg.lib(), self.chol)[0]
        self.rows = IS.residual_rows(self.chol, IS.S_MAX, seed=n)
        self.pitch = (n + 64) // 64 * 64  # at least one column of padding, as the residual rows of an engine have
        self.buf = torch.zeros((IS.S_MAX + 3, self.pitch), dtype=torch.float64, device=DEV)
        self.buf[:IS.S_MAX, :n] = torch.from_numpy(self.rows).to(DEV)
        self.g_ref = IR.g_rows(self.chol, self.rows)
        self.tol = IR.BAR * IR.scale(self.K, self.rows)
        self.g = self.prec.apply(self.buf, S=IS.S_MAX).cpu().numpy()


_APPLY = {}


@pytest.fixture(scope="module", params=IS.N_APPLY)
def ap(request, pkg, I):
    if request.param not in _APPLY:
        _APPLY[request.param] = Apply(pkg, I, request.param)
    return _APPLY[request.param]


def test_apply_agrees_with_the_restatement_over_shapes(ap):
    worst = 0.0
    for S in IS.S_APPLY:
        got = ap.prec.apply(ap.buf, S=S).cpu().numpy()
        assert got.shape == (S, ap.n)
        err = np.abs(np.asarray(got - ap.g_ref[:S], dtype=np.float64))
        assert (err <= ap.tol[:S]).all(), (ap.n, S, float(np.max(err / np.where(ap.tol[:S] > 0, ap.tol[:S], 1))))
        live = ap.tol[:S] > 0
        if live.any():
            worst = max(worst, float(np.max(err[live] / ap.tol[:S][live])) * IR.BAR)
        assert np.array_equal(_bits(got), _bits(ap.g[:S])), (ap.n, S)  # a row does not depend on S
    print("n = %d: largest |g - g_ref| / sum_j |K_ij| |r_j| = %.2e" % (ap.n, worst))
    assert not ap.rows[2].any() and not ap.g[2].any()  # a zero row gives exact zeros


def test_padding_nan_rows_and_rows_beyond_s(ap):
    n, S = ap.n, 200
    clean = ap.g[:S]
    # NaN in the pad columns and in every row >= S; the output buffer padded too, its padding and further rows untouched
    buf = ap.buf.clone()
    buf[:, n:] = float("nan")
    buf[S:, :] = float("nan")
    out = torch.full((S + 2, ap.pitch), -7.0, dtype=torch.float64, device=DEV)
    ap.prec.apply(buf, S=S, out=out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(_bits(got[:S, :n]), _bits(clean))
    assert (got[:S, n:] == -7.0).all() and (got[S:] == -7.0).all()
    # NaN and inf in one row stay in that row
    buf = ap.buf.clone()
    buf[17, 0] = float("nan")
    buf[90, n - 1] = float("inf")
    got = ap.prec.apply(buf, S=S).cpu().numpy()
    bad = np.zeros(S, dtype=bool)
    bad[[17, 90]] = True
    assert not np.isfinite(got[17]).any() and not np.isfinite(got[90]).all()
    assert np.isfinite(got[~bad]).all() and np.array_equal(_bits(got[~bad]), _bits(clean[~bad]))


def test_apply_row_bits_do_not_depend_on_position_stream_or_repetition(ap):
    want = _bits(ap.g)
    for p in (0, 15, 16, 63, 64, 200, IS.S_MAX - 1):
        alone = ap.prec.apply(ap.buf[p:p + 1]).cpu().numpy()
        assert np.array_equal(_bits(alone), want[p:p + 1]), (ap.n, "row", p)
    perm = np.random.default_rng(ap.n).permutation(IS.S_MAX)
    moved = ap.prec.apply(ap.buf[:IS.S_MAX][torch.from_numpy(perm).to(DEV)].contiguous()).cpu().numpy()
    assert np.array_equal(_bits(moved), want[perm]), (ap.n, "permuted")
    assert np.array_equal(_bits(ap.prec.apply(ap.buf, S=IS.S_MAX).cpu().numpy()), want), (ap.n, "repeated")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = ap.prec.apply(ap.buf, S=IS.S_MAX)
    side.synchronize()
    assert np.array_equal(_bits(other.cpu().numpy()), want), (ap.n, "second stream")


def test_apply_refuses_bad_arguments(pkg, ap):
    lib, p = pkg.lib(), ap.prec._p
    g = torch.empty((4, ap.n), dtype=torch.float64, device=DEV)
    assert lib.cf_prec_apply_device(p, ap.buf.data_ptr(), ap.n - 1, 4, g.data_ptr(), ap.n, None) == -1
    assert lib.cf_prec_apply_device(p, ap.buf.data_ptr(), ap.pitch, 4, g.data_ptr(), ap.n - 1, None) == -1
    assert lib.cf_prec_apply_device(p, ap.buf.data_ptr(), ap.pitch, -1, g.data_ptr(), ap.n, None) == -1
    assert lib.cf_prec_apply_device(p, None, ap.pitch, 4, g.data_ptr(), ap.n, None) == -1
    assert lib.cf_prec_apply_device(p, None, ap.pitch, 0, None, ap.n, None) == 0
    kd = ap.prec.diag()
    np.testing.assert_array_equal(kd, np.diag(ap.K))


# ---- infl_row_kernel and the launcher through cf_infl_device -------------------------------------------------------------------
class Case:
    """An engine, its rows of theta, the residual rows ``engine.parts`` gives for them, the restatement of everything the
    entry point returns, and the device's results at the default chunking -- computed once per shape and shared."""

    def __init__(self, pkg, I, name):
        self.name = name
        if name == "bao":
            self.lk, g = RS.bao_likelihood(pkg)
            self.block, self.data, self.theta = "bao", g["bao_val"], RS.bao_thetas(pkg)
            A = np.asarray(g["bao_inv_cov"], dtype=np.float64)
            self.K = 0.5 * (A + A.T)
        else:
            n = int(name)
            self.lk, syn = RS.sn_likelihood(pkg, n)
            self.block, self.data = "sn", syn["obs"]
            self.theta = RS.sn_thetas(pkg, IS.S_PANTHEON if n == IS.N_PANTHEON else IS.S_MAX)
            self.chol = syn["chol"]
            self.K = np.linalg.inv(syn["cov"])  # the scale of the bar only
        self.engine = self.lk.engine
        self.S, self.n = self.theta.shape[0], self.K.shape[0]
        self.x = torch.from_numpy(self.theta).to(DEV)
        self.rows = RS.parts_rows(self.engine, self.theta, self.block, self.data)[0]
        self.kdiag = self.engine.precision(self.block).diag()
        self.ref = self.restate(self.rows)
        I.set_library_chunk(self.engine, 0)
        self.got = self.run(I, self.x)

    def restate(self, rows):
        g = IR.g_rows_inv(self.K, rows) if self.block == "bao" else IR.g_rows(self.chol, rows)
        return IS.restate(rows, g, self.kdiag)

    def run(self, I, x):
        res = I.rows(self.engine, x, self.block)
        out = {k: res[k].cpu().numpy() for k in I.WANT}
        out["sample"] = np.stack([res["sample"][c].cpu().numpy() for c in I.COLUMNS], axis=1)
        return out


_CASES = {}


@pytest.fixture(scope="module", params=[str(n) for n in IS.N_SN] + [str(IS.N_PANTHEON), "bao"])
def case(request, pkg, I):
    if request.param not in _CASES:
        _CASES[request.param] = Case(pkg, I, request.param)
    return _CASES[request.param]


def _assert_rows_within_bar(case, got, ref, rows, what):
    """The row arrays and the five sample columns against the restatement, on the scale of the terms summed."""
    tol = IR.BAR * IR.scale(case.K, rows)                       # of g_i
    isk = np.where(case.kdiag > 0, 1.0 / np.sqrt(np.where(case.kdiag > 0, case.kdiag, 1.0)), 0.0)
    scales = dict(g=tol, contrib=np.abs(rows) * tol, z=tol * isk[None, :], loo=tol * (isk**2)[None, :])
    worst = {}
    for key, t in scales.items():
        err = np.abs(np.asarray(got[key] - ref[key], dtype=np.float64))
        fin = np.isfinite(np.asarray(ref[key], dtype=np.float64))
        assert np.array_equal(np.isfinite(got[key]), fin), (what, key, "non-finite positions differ")
        assert (err[fin] <= t[fin]).all(), (what, key)
        live = fin & (t > 0)
        worst[key] = float(np.max(err[live] / t[live])) * IR.BAR if live.any() else 0.0
    s_got, s_ref = got["sample"], np.asarray(ref["sample"], dtype=np.float64)
    ok = np.isfinite(s_ref[:, 0])
    assert np.array_equal(np.isfinite(s_got[:, 0]), ok), (what, "NaN rows differ")
    chi_tol = (np.abs(rows) * tol).sum(axis=1)
    assert (np.abs(s_got[ok, 0] - s_ref[ok, 0]) <= chi_tol[ok]).all(), (what, "chi2")
    z_tol = tol * isk[None, :]
    d_tol = (2 * np.abs(np.asarray(ref["g"], dtype=np.float64)) + tol) * tol * (isk**2)[None, :]  # of g_i^2 / K_ii
    for s in np.nonzero(ok)[0]:
        for col, vals, vt in ((1, np.abs(ref["z"][s]), z_tol[s]), (3, ref["drop"][s], d_tol[s])):
            first, second = IR.top_two_gap(vals)
            idx = int(s_got[s, col + 1])
            assert idx in (first, second), (what, s, col)
            if float(vals[first] - vals[second]) > vt[first] + vt[second]:
                assert idx == first, (what, s, col, "index")
            assert abs(s_got[s, col] - float(vals[idx])) <= vt[idx] + 1e-300, (what, s, col, "value")
    print(what, {k: f"{v:.2e}" for k, v in worst.items()})


def test_rows_and_sample_table_agree_with_the_restatement(pkg, case):
    assert case.got["sample"].shape == (case.S, 5) and case.got["g"].shape == (case.S, case.n)
    _assert_rows_within_bar(case, case.got, case.ref, case.rows, f"{case.name}: cf_infl_device against the restatement")
    # the chi2 column against the likelihood's own chi^2: an independent route through the solve kernel
    chi2 = case.engine.chi_squared(case.theta)
    assert np.max(np.abs(case.got["sample"][:, 0] / chi2 - 1)) <= 1e-10
    # sum_i contrib_i is that chi^2 again
    assert np.max(np.abs(case.got["contrib"].sum(axis=1) / chi2 - 1)) <= 1e-10


def test_a_nan_theta_gives_nan_in_its_row_only(I, case):
    theta = case.theta.copy()
    theta[5, 2 if case.block == "sn" else 1] = np.nan
    got = case.run(I, torch.from_numpy(theta).to(DEV))
    keep = np.arange(case.S) != 5
    for key in (*I.WANT, "sample"):
        assert np.isfinite(got[key][keep]).all(), key
        assert np.array_equal(_bits(got[key][keep]), _bits(case.got[key][keep])), key
    assert np.isnan(got["g"][5]).all() and np.isnan(got["contrib"][5]).all() and np.isnan(got["sample"][5, [0, 1, 3]]).all()
    assert got["sample"][5, 2] == 0 and got["sample"][5, 4] == 0  # the first NaN wins


def test_a_row_has_the_same_bits_wherever_and_however_it_is_computed(pkg, I, case):
    eng, L = case.engine, pkg._lib
    keys = (*I.WANT, "sample")
    try:
        for chunk in IS.CHUNKS:
            I.set_library_chunk(eng, chunk)
            got = case.run(I, case.x)
            for key in keys:
                assert np.array_equal(_bits(got[key]), _bits(case.got[key])), (case.name, "chunk", chunk, key)
        I.set_library_chunk(eng, 32)
        for p in (0, 31, 32, case.S - 1):
            got = case.run(I, case.x[p:p + 1])
            for key in keys:
                assert np.array_equal(_bits(got[key]), _bits(case.got[key][p:p + 1])), (case.name, "row", p, key)
        again = case.run(I, case.x)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            other = case.run(I, case.x)
        for key in keys:
            assert np.array_equal(_bits(again[key]), _bits(case.got[key])), (case.name, "repeated", key)
            assert np.array_equal(_bits(other[key]), _bits(case.got[key])), (case.name, "second stream", key)
        # host pointers (cf_infl): the same kernels behind a copy
        out, arrs = IS.host_out(L, case.S, case.n)
        L.check(pkg.lib().cf_infl(eng._h, eng.precision(case.block)._p, case.theta.ctypes.data, case.S, None,
                                  L.RESID_BLOCKS[case.block], None, 0, C.byref(out), None, None))
        for key in keys:
            assert np.array_equal(_bits(arrs[key]), _bits(case.got[key])), (case.name, "host pointers", key)
    finally:
        I.set_library_chunk(eng, 0)


def test_host_pointers_beyond_one_piece_have_the_bits_of_the_device_path(pkg, I):
    """cf_infl stages its rows through the device in pieces of 4096: 4097 rows of the smallest SN engine cross one boundary, so
    the second piece's rows land behind the first's in g and in the sample table, and the accumulator is continued across it."""
    L, n, S, thr = pkg._lib, IS.N_SN[0], 4097, np.array(IS.THRESHOLDS)
    lk, _ = RS.sn_likelihood(pkg, n)
    eng = lk.engine
    try:
        theta = RS.sn_thetas(pkg, S)
        dacc = I.F.DatumAcc(n, thr.size, DEV)
        dev = I._launch(eng, torch.from_numpy(theta).to(DEV), None, "sn", ("g",), True, thr, dacc, None)
        out, arrs = IS.host_out(L, S, n, want=("g", "sample"))
        hacc, harrs = RS.host_acc(L, n, thr.size)
        L.check(pkg.lib().cf_infl(eng._h, eng.precision("sn")._p, theta.ctypes.data, S, None, L.RESID_BLOCKS["sn"], thr.ctypes.data,
                                  thr.size, C.byref(out), C.byref(hacc), None))
        assert np.isfinite(arrs["g"]).all() and np.isfinite(arrs["sample"]).all()
        for key in ("g", "sample"):
            assert np.array_equal(_bits(arrs[key]), _bits(dev[key].cpu().numpy())), key
        for key in ("w_sum", "mean", "m2", "exceed"):
            assert np.array_equal(_bits(harrs[key]), _bits(getattr(dacc, key).cpu().numpy())), key
        assert harrs["n_used"][0] == S and np.array_equal(harrs["n_used"], dacc.n_used.cpu().numpy())
        assert np.array_equal(harrs["n_skipped"], dacc.n_skipped.cpu().numpy())
    finally:
        eng.close()


def test_only_what_was_asked_for_is_returned_and_no_rows_is_a_no_op(I, case):
    res = I.rows(case.engine, case.x[:40], case.block, want=("z",))
    assert set(res) == {"z", "sample"}
    assert np.array_equal(_bits(res["z"].cpu().numpy()), _bits(case.got["z"][:40]))
    assert np.array_equal(_bits(res["sample"]["max_z"].cpu().numpy()), _bits(case.got["sample"][:40, 1]))
    none = I.rows(case.engine, case.x[:0], case.block)
    assert none["g"].shape == (0, case.n) and none["sample"]["chi2"].shape == (0,)


def test_a_datum_the_likelihood_ignores_gives_exact_zeros(pkg, I):
    g = RS.golden("bao_desi_fs_lya")
    inv = np.array(g["bao_inv_cov"], dtype=np.float64)
    dead = [3, inv.shape[0] - 1]
    inv[dead, :] = 0.0
    inv[:, dead] = 0.0
    lk = pkg.scripts.build("bao/desi_fs_lya.py", bao=(g["bao_z"], g["bao_val"], g["bao_qty"], inv))
    try:
        theta = RS.bao_thetas(pkg, 40)
        res = I.rows(lk.engine, torch.from_numpy(theta).to(DEV), "bao")
        for key in I.WANT:
            got = res[key].cpu().numpy()
            assert np.isfinite(got).all() and not got[:, dead].any(), key
        assert np.isinf(lk.engine.precision("bao").loo_sigma()[dead]).all()
        chi2 = lk.engine.chi_squared(theta)
        assert np.max(np.abs(res["sample"]["chi2"].cpu().numpy() / chi2 - 1)) <= 1e-10
        assert not np.isin(res["sample"]["max_z_index"].cpu().numpy(), dead).any()
    finally:
        lk.engine.close()
