"""GPU (-m gpu): the attribution as a user calls it -- the per-datum accumulators of ``influence.report`` against two-pass sums
and across every cut of a chain, the samplers' ``influence``, the split of the Union3 velocity-step Delta chi^2 over its 22
bins, the example, and what the entry point refuses on real handles.  The kernels themselves are judged in
tests/test_gpu_infl_kernels.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import infl_reference as IR
import infl_shapes as IS
import resid_reference as R
import resid_shapes as RS
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def I(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.influence


@pytest.fixture(scope="module")
def small(pkg, I):
    lk, syn = RS.sn_likelihood(pkg, 65)
    yield lk, syn
    lk.engine.close()


@pytest.fixture(scope="module")
def union3(pkg, I):
    g = golden("sn_union3_1")
    box = pkg.likelihoods.SnUnion3.PRIOR_BOX
    lk = pkg.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    yield lk, box, g
    lk.engine.close()


def _raw(acc):
    out = {}
    for name, a in (("z", acc.z), ("contrib", acc.contrib)):
        for k in ("w_sum", "mean", "m2", "exceed", "n_used", "n_skipped"):
            out[name + "." + k] = getattr(a, k).cpu().numpy()
    return out


def _same_state(a, b):
    return all(np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]) for k in a)


# ---- the accumulators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_report_accumulators(pkg, I, small, weighted):
    lk, syn = small
    eng, S = lk.engine, IS.S_MAX
    theta = RS.sn_thetas(pkg, S)
    theta[7, 2] = np.nan  # a row that must be skipped, and counted, for every datum
    rows = RS.parts_rows(eng, theta, "sn", syn["obs"])[0]
    kdiag = eng.precision("sn").diag()
    contrib, z, _, _ = IR.row_arrays(rows, IR.g_rows(syn["chol"], rows), kdiag)
    rng = np.random.default_rng(3)
    w = None
    if weighted:
        w = rng.uniform(0.0, 1.0, S)
        w[rng.choice(S, size=S // 10, replace=False)] = 0.0
    x = torch.from_numpy(theta).to(DEV)
    wd = None if w is None else torch.from_numpy(w).to(DEV)
    I.set_library_chunk(eng, 0)
    rep = I.report(eng, x, weights=wd, thresholds=IS.THRESHOLDS)
    d = rep["datum"]
    # against the restatement's two-pass sums, within the fit report's own accumulator bound: 1e-10 of |mean| + std
    for name, ref_rows in (("z", z), ("contrib", contrib)):
        mean, std = R.two_pass(ref_rows, w)
        scale = np.abs(mean) + std
        e_mean = float(np.max(np.abs(d[name + "_mean"] - mean) / scale))
        e_std = float(np.max(np.abs(d[name + "_std"] - std) / scale))
        print("influence.report, %s: mean %.2e std %.2e of |mean| + std" % (name, e_mean, e_std))
        assert e_mean <= 1e-10 and e_std <= 1e-10
    wt = np.ones(S) if w is None else w
    used = np.isfinite(np.asarray(z, dtype=np.float64)) & (wt > 0)[:, None]
    assert np.array_equal(d["n_used"], used.sum(axis=0)) and np.array_equal(d["n_skipped"], S - used.sum(axis=0))
    assert (d["n_skipped"] >= 1).all()
    # exceedance: thresholds in sigmas of the leave-one-out residual (no |z| of these rows lies within 1e-9 of a threshold)
    zd = np.asarray(z, dtype=np.float64)
    for k, t in enumerate(IS.THRESHOLDS):
        with np.errstate(invalid="ignore"):
            assert not (used & (np.abs(np.abs(zd) - t) < 1e-9)).any()
            want = (np.where(used & (np.abs(zd) > t), wt[:, None], 0.0)).sum(axis=0) / np.where(used, wt[:, None], 0.0).sum(axis=0)
        np.testing.assert_allclose(d["exceed"][k], want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(d["loo_sigma"], 1.0 / np.sqrt(kdiag), rtol=1e-15)
    np.testing.assert_allclose(d["sigma"], np.sqrt(np.diag(syn["cov"])), rtol=1e-12)
    assert (d["loo_sigma"] <= d["sigma"] * (1 + 1e-12)).all()  # conditioning on the others can only sharpen a datum
    assert np.array_equal(d["redshift"], eng.sn_z) and rep["columns"] == IR.COLUMNS
    # the per-sample table is that of influence.rows
    table = I.rows(eng, x, want=())["sample"]
    for j, name in enumerate(I.COLUMNS):
        assert np.array_equal(rep["sample"][:, j].cpu().numpy().view(np.uint64), table[name].cpu().numpy().view(np.uint64)), name
    # every cut of the chain gives the same bits: the library's chunk, two calls, host pointers
    whole = I.Accumulator(eng, "sn", IS.THRESHOLDS, device=DEV)
    whole.update(x, wd)
    raw = _raw(whole)
    try:
        for chunk in IS.CHUNKS:
            I.set_library_chunk(eng, chunk)
            acc = I.Accumulator(eng, "sn", IS.THRESHOLDS, device=DEV)
            acc.update(x, wd)
            assert _same_state(_raw(acc), raw), chunk
        two = I.Accumulator(eng, "sn", IS.THRESHOLDS, device=DEV)
        two.update(x[:100], None if wd is None else wd[:100])
        two.update(x[100:], None if wd is None else wd[100:])
        assert _same_state(_raw(two), raw), "two calls"
        for key, v in two.result().items():
            assert np.array_equal(v, d[key], equal_nan=True), key
        L = pkg._lib
        az, arr_z = RS.host_acc(L, 65, 3)
        ac, arr_c = RS.host_acc(L, 65, 0)
        t = np.asarray(IS.THRESHOLDS, dtype=np.float64)
        L.check(pkg.lib().cf_infl(eng._h, eng.precision("sn")._p, theta.ctypes.data, S, None if w is None else w.ctypes.data,
                                  L.CF_RB_SN, t.ctypes.data, 3, None, C.byref(az), C.byref(ac)))
        host = {"z." + k: v for k, v in arr_z.items()}
        host.update({"contrib." + k: v for k, v in arr_c.items()})
        host["contrib.exceed"] = host["contrib.exceed"][:0]
        assert _same_state(host, raw), "host pointers"
    finally:
        I.set_library_chunk(eng, 0)


def test_samplers_report_their_chains(pkg, I, small, union3):
    lk, _ = small
    E = pkg.ensemble
    start = torch.from_numpy(RS.sn_thetas(pkg, 16, seed=21)).to(DEV)
    ens = E.ShardedEnsemble(lk.engine.torch_log_prob(), start, seed=3, moves=(("stretch", 1.0),))
    ens.run_mcmc(5)
    got = ens.influence(discard=1, thresholds=(1.0, 2.5))
    chain = ens.get_chain(discard=1, flat=True)
    want = I.report(lk.engine, chain, thresholds=(1.0, 2.5))
    assert torch.equal(got["sample"], want["sample"]) and got["sample"].shape == (4 * 16, 5)
    for key, v in got["datum"].items():
        assert np.array_equal(v, want["datum"][key], equal_nan=True), key
    u3 = union3[0]
    p = pkg.nested.Prior()
    p.add_parameter("dM", dist=(-1, +1))
    p.add_parameter("om", dist=(0.1, 0.7))
    p.add_parameter("v", dist=(-9, 9))
    s = pkg.nested.DeviceNestedSampler(p, u3.engine.torch_log_prob(pkg.CF_OUT_LOGL), n_live=60, seed=5)
    s.run(f_live=0.2)
    pts, log_w, _ = s.posterior()
    x, w = torch.from_numpy(np.ascontiguousarray(pts)).to(DEV), torch.from_numpy(np.exp(log_w)).to(DEV)
    got = s.influence(thresholds=(2.0,))
    want = I.report(u3.engine, x, weights=w, thresholds=(2.0,))
    assert torch.equal(got["sample"], want["sample"])
    for key, v in got["datum"].items():
        assert np.array_equal(v, want["datum"][key], equal_nan=True), key
    assert got["datum"]["exceed"].shape == (1, 22) and np.allclose(got["datum"]["w_sum"], float(w.sum()), rtol=1e-12)


# ---- end to end on real data ---------------------------------------------------------------------------------------------------
def test_union3_velocity_step_delta_chi2_is_split_over_its_bins(pkg, I, union3):
    """sn/union3_1.py: chi2 22.148 with the velocity step free against 28.759 with v = 0 -- a Delta chi^2 of 6.61 that
    ``attribution`` splits exactly over the 22 bins."""
    lk, box, g = union3
    opt = pkg.optimize
    f = lk.engine.torch_log_prob(pkg.CF_OUT_LOGL)
    fit = opt.best_fit(f, box, n_starts=32, seed=0)
    nested = opt.best_fit(f, box, n_starts=32, seed=0, fixed={2: 0.0})
    assert fit.best_converged and nested.best_converged
    out = I.attribution(lk.engine, nested.x, fit.x)
    dchi2 = nested.chi2 - fit.chi2
    print("Delta chi^2 %.6f; attribution total %.6f, sum of delta %.6f" % (dchi2, out["total"], out["delta"].sum()))
    assert dchi2 == pytest.approx(6.61, abs=0.01)
    assert abs(out["total"] - dchi2) <= 1e-8 and abs(out["delta"].sum() - dchi2) <= 1e-8
    assert abs(out["cumulative"][-1] - dchi2) <= 1e-8
    assert np.array_equal(out["redshift"], np.sort(g["z_cmb"])) and out["delta"].shape == (22,)
    # paired rows: the same pair twice is the pair
    pair = I.attribution(lk.engine, np.stack([nested.x, nested.x]), np.stack([fit.x, fit.x]))
    assert np.array_equal(pair["delta"], out["delta"]) and not pair["delta_std"].any() and pair["total"] == out["total"]


def test_the_example_prints_its_table():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "union3_step_attribution.py")], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Delta chi^2" in r.stdout and "delta_i" in r.stdout and "largest leave-one-out z-scores" in r.stdout
    rows = [ln for ln in r.stdout.splitlines() if ln.strip() and ln.split()[0].isdigit()]
    assert len(rows) >= 22  # one line per bin


# ---- what the entry point refuses ----------------------------------------------------------------------------------------------
def test_refusals_on_real_handles(pkg, I, small):
    L, lib = pkg._lib, pkg.lib()
    lk, syn = small
    eng = lk.engine
    x = torch.from_numpy(RS.sn_thetas(pkg, 4)).to(DEV)
    sample = torch.empty((4, L.CF_INFL_NCOL), dtype=torch.float64, device=DEV)
    out = L.cf_infl_out()
    out.struct_size, out.sample = C.sizeof(L.cf_infl_out), sample.data_ptr()
    prec = eng.precision("sn")
    assert eng.precision("sn") is prec  # built once, kept on the engine

    def call(engine, p=prec._p, block=L.CF_RB_SN, S=4, theta=x.data_ptr(), n_thr=0):
        return lib.cf_infl_device(engine._h, p, theta, S, None, block, None, n_thr, C.byref(out), None, None, None)

    assert call(eng) == 0
    assert call(eng, block=L.CF_RB_BAO) == -1 and b"no BAO block" in lib.cf_last_error()
    assert call(eng, p=None) == -1 and b"null cf_prec" in lib.cf_last_error()
    assert call(eng, S=-1) == -1 and call(eng, theta=None) == -1 and call(eng, n_thr=5) == -1
    assert call(eng, S=0, theta=None) == 0
    other = I.Precision(np.linalg.cholesky(IS.covariance(pkg, 64)), device=0)
    assert call(eng, p=other._p) == -1 and b"cf_prec.n is not" in lib.cf_last_error()
    other.close()
    assert lib.cf_infl_set_chunk(eng._h, 65537) == -1 and lib.cf_infl_set_chunk(eng._h, 0) == 0
    with pytest.raises(ValueError, match="no BAO block"):
        I.rows(eng, x, "bao")
    two = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], devices=[0, 0])
    try:
        assert call(two.engine) == -1 and b"several devices" in lib.cf_last_error()
        with pytest.raises(ValueError, match="several devices"):
            I.rows(two.engine, x)
    finally:
        two.engine.close()
    import quasar_shapes as QS

    c = QS.build_case(0)
    qe = pkg.LikelihoodEngine(**QS.engine_kwargs(c, pkg.Param, pkg.engine.solve_mode_of(c["solve"])))
    try:
        th = torch.from_numpy(np.ascontiguousarray(c["theta"][:1])).to(DEV)
        assert lib.cf_infl_device(qe._h, prec._p, th.data_ptr(), 1, None, L.CF_RB_SN, None, 0, C.byref(out), None, None, None) == -1
        assert b"quasar" in lib.cf_last_error()
        with pytest.raises(ValueError, match="quasar engine"):
            I.rows(qe, th)
    finally:
        qe.close()
    # closing the engine releases its precision matrices
    lk2, _ = RS.sn_likelihood(pkg, 17)
    p2 = lk2.engine.precision("sn")
    lk2.engine.close()
    assert not p2._p.value
