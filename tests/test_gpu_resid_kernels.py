"""GPU (-m gpu): the two kernels of the fit report (csrc/cosmofit_resid.hip) at the shapes they accept -- SN engines around the
pitch of the residual rows, one Pantheon+-sized engine, the 13-datum DESI BAO engine; 1 .. 257 rows with the library's chunk
lowered so that chunk boundaries are crossed.  Kernel A against the long-double restatement applied to ``engine.parts``' own
rows, its bits against position / chunking / pointer kind; kernel B against the sequential restatement, its bits against every
cut of the chain."""
import ctypes as C

import numpy as np
import pytest
import torch

import resid_reference as R
import resid_shapes as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def F(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.fit_report


class Case:
    """An engine, its rows of theta, the residual rows ``engine.parts`` gives for them, and the device statistics of all rows
    at the default chunking -- computed once per shape and shared."""

    def __init__(self, pkg, F, name):
        self.name = name
        if name == "bao":
            self.lk, g = RS.bao_likelihood(pkg)
            self.block, self.data, self.theta = "bao", g["bao_val"], RS.bao_thetas(pkg)
        else:
            n = int(name)
            self.lk, syn = RS.sn_likelihood(pkg, n)
            self.block, self.data = "sn", syn["obs"]
            self.theta = RS.sn_thetas(pkg, 64 if n == RS.N_PANTHEON else RS.S_MAX)
        self.engine = self.lk.engine
        self.S = self.theta.shape[0]
        self.x = torch.from_numpy(self.theta).to(DEV)
        self.sigma = self.engine.resid_sigma(self.block)
        self.rows, self.y = RS.parts_rows(self.engine, self.theta, self.block, self.data)
        F.set_library_chunk(self.engine, 0)
        self.stats, self.blocks = (t.cpu().numpy() for t in F.sample_stats(self.engine, self.x, self.block))


_CASES = {}


@pytest.fixture(scope="module", params=[str(n) for n in RS.N_SN] + [str(RS.N_PANTHEON), "bao"])
def case(request, pkg, F):
    if request.param not in _CASES:
        _CASES[request.param] = Case(pkg, F, request.param)
    return _CASES[request.param]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_within_bar(got, want, what):
    errs = R.errors(got, want)
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for col, err in errs.items():
        assert err <= (RS.ABS if col in R.ABSOLUTE else RS.REL), (what, col, err)


# ---- kernel A ------------------------------------------------------------------------------------------------------------------
def test_sample_stats_agree_with_the_restatement(case):
    assert case.stats.shape == (case.S, len(R.COLUMNS))
    _assert_within_bar(case.stats, R.stats_matrix(case.rows, case.y, case.sigma), f"{case.name}: kernel A against the restatement")
    parts = case.engine.parts(case.theta)
    np.testing.assert_allclose(case.blocks[:, :3], parts["chi2_blocks"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(case.blocks[:, 6], parts["chi2_cc"], rtol=1e-10, atol=0)


def test_sigma_is_the_diagonal_of_the_covariance(pkg, case):
    if case.block == "bao":
        g = RS.golden("bao_desi_fs_lya")
        want = np.sqrt(np.diag(np.linalg.inv(g["bao_inv_cov"])))
    else:
        syn = pkg.synthetic.pantheon_like(n_sn=int(case.name), seed=5, rank=min(40, int(case.name)))
        want = np.sqrt(np.diag(syn["cov"]))
    np.testing.assert_allclose(case.sigma, want, rtol=1e-12, atol=0)


def test_a_nan_theta_gives_nan_in_its_row_only(F, case):
    theta = case.theta.copy()
    theta[5, 2 if case.block == "sn" else 1] = np.nan
    got = F.sample_stats(case.engine, torch.from_numpy(theta).to(DEV), case.block)[0].cpu().numpy()
    assert np.isnan(got[5, [0, 1, 2, 3, 5, 6, 7, 8]]).all()  # (ss_tot of the BAO block is of the data alone)
    keep = np.arange(case.S) != 5
    assert np.array_equal(_bits(got[keep]), _bits(case.stats[keep]))
    rows, y = RS.parts_rows(case.engine, theta, case.block, case.data)
    _assert_within_bar(got, R.stats_matrix(rows, y, case.sigma), f"{case.name}: a NaN row")


def test_a_row_has_the_same_bits_wherever_and_however_it_is_computed(pkg, F, case):
    eng, want = case.engine, _bits(case.stats)
    try:
        for chunk in RS.CHUNKS:
            F.set_library_chunk(eng, chunk)
            got = F.sample_stats(eng, case.x, case.block)[0].cpu().numpy()
            assert np.array_equal(_bits(got), want), (case.name, "chunk", chunk)
        F.set_library_chunk(eng, 32)
        for S in RS.ROWS:
            if S <= case.S:
                got = F.sample_stats(eng, case.x[:S], case.block)[0].cpu().numpy()
                assert np.array_equal(_bits(got), want[:S]), (case.name, "S", S)
        for p in (0, 31, 32, 95, 96, case.S - 1):
            if p < case.S:
                got = F.sample_stats(eng, case.x[p:p + 1], case.block)[0].cpu().numpy()
                assert np.array_equal(_bits(got), want[p:p + 1]), (case.name, "row", p)
        # host pointers (cf_resid): the same kernels behind a copy
        out, blocks = np.empty((case.S, len(R.COLUMNS))), np.empty((case.S, 10))
        L = pkg._lib
        L.check(pkg.lib().cf_resid(eng._h, case.theta.ctypes.data, case.S, None, L.RESID_BLOCKS[case.block], None, 0, out.ctypes.data,
                                   blocks.ctypes.data, None))
        assert np.array_equal(_bits(out), want), (case.name, "host pointers")
        np.testing.assert_allclose(blocks, case.blocks, rtol=1e-12, atol=0)
    finally:
        F.set_library_chunk(eng, 0)


def test_no_rows_is_a_no_op(F, case):
    stats, blocks = F.sample_stats(case.engine, case.x[:0], case.block)
    assert stats.shape == (0, len(R.COLUMNS)) and blocks.shape == (0, 10)
    d = F.datum_stats(case.engine, case.x[:0], block=case.block)
    assert np.isnan(d["mean"]).all() and (d["n_used"] == 0).all() and (d["n_skipped"] == 0).all()


# ---- kernel B ------------------------------------------------------------------------------------------------------------------
def _thresholds_between_pulls(rows, sigma):
    """Three thresholds, each half way between two neighbouring values of |r| / sigma: no pull is within rounding of one."""
    with np.errstate(invalid="ignore"):
        pulls = np.sort((np.abs(rows) / sigma[None, :]).ravel())
    pulls = pulls[np.isfinite(pulls)]
    out = []
    for q in (0.3, 0.6, 0.9):
        k = int(q * (pulls.size - 1))
        while k + 1 < pulls.size and not pulls[k + 1] - pulls[k] > 1e-9 * pulls[k + 1]:
            k += 1
        out.append(0.5 * (pulls[k] + pulls[min(k + 1, pulls.size - 1)]) if pulls.size > 1 else 0.5 * pulls[0])
    return tuple(out)


def _raw(acc):
    return {k: getattr(acc, k).cpu().numpy() for k in ("w_sum", "mean", "m2", "exceed", "n_used", "n_skipped")}


def _same_state(a, b):
    return all(np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]) for k in a)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_datum_accumulators(pkg, F, case, weighted):
    eng, S = case.engine, case.S
    theta = case.theta.copy()
    theta[7, 2 if case.block == "sn" else 1] = np.nan  # a row that must be skipped, and counted, for every datum
    rows = RS.parts_rows(eng, theta, case.block, case.data)[0]
    rng = np.random.default_rng(3)
    w = None
    if weighted:
        w = rng.uniform(0.0, 1.0, S)
        w[rng.choice(S, size=max(1, S // 10), replace=False)] = 0.0
    thr = _thresholds_between_pulls(rows, case.sigma)
    x = torch.from_numpy(theta).to(DEV)
    wd = None if w is None else torch.from_numpy(w).to(DEV)
    F.set_library_chunk(eng, 0)
    whole = F.Accumulator(eng, case.block, thr, device=DEV).update(x, wd)
    got, raw = whole.result(), _raw(whole)
    want_state = R.accumulate(R.new_state(rows.shape[1], 3), rows, case.sigma, thr, w)
    want = R.finish(want_state, case.sigma)
    assert np.array_equal(got["n_skipped"], want["n_skipped"]) and np.array_equal(got["n_used"], want["n_used"])
    assert (got["n_skipped"] >= 1).all()
    with np.errstate(invalid="ignore"):
        scale = np.abs(want["mean"]) + want["std"]
        e_mean = np.max(np.abs(got["mean"] - want["mean"]) / scale)
        e_std = np.max(np.abs(got["std"] - want["std"]) / scale)
    print(case.name, "kernel B against the restatement: mean %.2e std %.2e of |mean| + std" % (e_mean, e_std))
    assert e_mean <= 1e-10 and e_std <= 1e-10
    assert np.array_equal(np.isnan(got["mean"]), np.isnan(np.asarray(want["mean"], float)))
    # exceedance: the same additions of the same weights in the same order -- exact
    wt = np.ones(S) if w is None else w
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(rows) & (wt > 0)[:, None]
        for k, t in enumerate(thr):
            beyond = ok & (np.abs(rows) > t * case.sigma[None, :])
            seq = np.cumsum(np.where(beyond, wt[:, None], 0.0), axis=0)[-1]  # np.cumsum adds in row order
            assert np.array_equal(raw["exceed"][k], seq), (case.name, "threshold", k)
            assert np.array_equal(got["exceed"][k], seq / raw["w_sum"])
    if not weighted:
        assert np.array_equal(raw["w_sum"], got["n_used"].astype(np.float64))
    np.testing.assert_allclose(got["pull_mean"], got["mean"] / case.sigma, rtol=0, atol=0)
    # every cut of the chain gives the same bits: the library's chunk, two calls, the driver's chunk, host pointers
    try:
        for chunk in RS.CHUNKS[:2]:
            F.set_library_chunk(eng, chunk)
            assert _same_state(_raw(F.Accumulator(eng, case.block, thr, device=DEV).update(x, wd)), raw), (case.name, chunk)
        cut = min(100, S // 2)
        two = F.Accumulator(eng, case.block, thr, device=DEV).update(x[:cut], None if wd is None else wd[:cut])
        two.update(x[cut:], None if wd is None else wd[cut:])
        assert _same_state(_raw(two), raw), (case.name, "two calls")
        F.set_library_chunk(eng, 0)
        d = F.datum_stats(eng, x, weights=wd, block=case.block, thresholds=thr, chunk=50)
        for key in ("mean", "std", "exceed", "n_used", "n_skipped"):
            assert np.array_equal(d[key], got[key], equal_nan=True), (case.name, "driver chunk", key)
        L = pkg._lib
        acc, arrs = RS.host_acc(L, rows.shape[1], 3)
        t = np.asarray(thr, dtype=np.float64)
        L.check(pkg.lib().cf_resid(eng._h, theta.ctypes.data, S, None if w is None else w.ctypes.data, L.RESID_BLOCKS[case.block],
                                   t.ctypes.data, 3, None, None, C.byref(acc)))
        arrs["exceed"] = arrs["exceed"][:3]
        assert _same_state(arrs, raw), (case.name, "host pointers")
    finally:
        F.set_library_chunk(eng, 0)


def test_host_pointers_beyond_one_piece_have_the_bits_of_the_device_path(pkg, F):
    """cf_resid stages its rows through the device in pieces of 65536: 65537 rows of the smallest SN engine cross one boundary,
    so the second piece's row lands behind the first's in both tables, its weight is read from behind the first's, and the
    accumulator is continued across it."""
    L, n, S, thr = pkg._lib, RS.N_SN[0], 65537, np.array(RS.THRESHOLDS)
    lk, _ = RS.sn_likelihood(pkg, n)
    eng = lk.engine
    try:
        theta = RS.sn_thetas(pkg, S)
        w = np.random.default_rng(4).uniform(0.0, 1.0, S)
        w[::9] = 0.0
        dacc = F.Accumulator(eng, "sn", thr, device=DEV)
        d_sample, d_blocks = F._launch(eng, torch.from_numpy(theta).to(DEV), torch.from_numpy(w).to(DEV), "sn", dacc, True)
        sample, blocks = np.full((S, len(R.COLUMNS)), np.nan), np.full((S, 10), np.nan)
        hacc, arrs = RS.host_acc(L, n, thr.size)
        L.check(pkg.lib().cf_resid(eng._h, theta.ctypes.data, S, w.ctypes.data, L.RESID_BLOCKS["sn"], thr.ctypes.data, thr.size,
                                   sample.ctypes.data, blocks.ctypes.data, C.byref(hacc)))
        assert np.isfinite(blocks).all() and np.isfinite(sample[:, 0]).all()
        assert np.array_equal(_bits(sample), _bits(d_sample.cpu().numpy()))
        assert np.array_equal(_bits(blocks), _bits(d_blocks.cpu().numpy()))
        assert _same_state(arrs, _raw(dacc))
        assert arrs["n_used"][0] + arrs["n_skipped"][0] == S and arrs["n_skipped"][0] == np.count_nonzero(w == 0.0)
    finally:
        eng.close()


def test_report_is_one_pass_with_both_outputs(F, case):
    rep = F.report(case.engine, case.x, block=case.block, thresholds=(1.0, 2.0))
    assert np.array_equal(_bits(rep["stats"].cpu().numpy()), _bits(case.stats))
    d = F.datum_stats(case.engine, case.x, block=case.block, thresholds=(1.0, 2.0))
    for key in ("mean", "std", "exceed", "n_used", "n_skipped", "sigma"):
        assert np.array_equal(rep["datum"][key], d[key], equal_nan=True), key
    z = case.engine.sn_z if case.block == "sn" else case.engine.bao_z
    assert np.array_equal(rep["datum"]["z"], z) and rep["columns"] == R.COLUMNS
