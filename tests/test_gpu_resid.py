"""GPU (-m gpu): the fit report as a user calls it -- the statistics of the reference's own post-fit lines reproduced through the
mirrors of four scripts, the samplers' ``fit_report``, the summary's reductions, and the state the call leaves the handle's
workspace in.  The kernels themselves are judged in tests/test_gpu_resid_kernels.py."""
import numpy as np
import pytest
import torch

import resid_shapes as RS
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def F(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.fit_report


@pytest.fixture(scope="module")
def small(pkg, F):
    lk, syn = RS.sn_likelihood(pkg, 65)
    yield lk
    lk.engine.close()


@pytest.fixture(scope="module")
def union3(pkg, F):
    g = golden("sn_union3_1")
    box = pkg.likelihoods.SnUnion3.PRIOR_BOX
    lk = pkg.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], g["obs"], g["cov"], H0=float(g["H0"]), bounds=box)
    yield lk
    lk.engine.close()


# ---- 4. the reference's own numbers --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RS.FIXTURE_CASES)
def test_fixture_statistics_are_reproduced_on_the_device(pkg, F, case):
    g = golden("residuals")
    lk, block = RS.fixture_likelihood(pkg, case)
    try:
        x = torch.from_numpy(np.ascontiguousarray(g[case + "/thetas"])).to(DEV)
        assert x.shape[0] == 32
        stats = F.sample_stats(lk.engine, x, block)[0].cpu().numpy()
        worst = {}
        for fx, col in RS.FIXTURE_COLUMNS.items():
            got, want = stats[:, F.COLUMNS.index(col)], g[f"{case}/{fx}"]
            err = np.abs(got - want) if col in ("mean", "skew", "kurtosis") else np.abs(got / want - 1)
            worst[col] = float(err.max())
        print(case, "largest error against the fixture:", {k: f"{v:.2e}" for k, v in worst.items()})
        for col, err in worst.items():
            assert err <= 1e-10, (case, col, err)
        # the residual vectors the statistics are of: the fixture's first rows against the accessor path
        rows, y = RS.parts_rows(lk.engine, g[case + "/thetas"][:8], block, RS.fixture_data(case))
        np.testing.assert_allclose(rows, g[case + "/residuals"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(y, g[case + "/y"], rtol=1e-10, atol=0)
    finally:
        lk.engine.close()


# ---- 5. the samplers -----------------------------------------------------------------------------------------------------------
def _same_report(a, b):
    assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["chi2_blocks"], b["chi2_blocks"])
    for key, v in a["datum"].items():
        assert np.array_equal(v, b["datum"][key], equal_nan=True), key
    sa, sb = a["summary"], b["summary"]
    assert np.array_equal(sa["center"], sb["center"]) and sa["chi2"] == sb["chi2"] and sa["dof"] == sb["dof"]
    assert sa["at_center"] == sb["at_center"]
    for key, v in sa["posterior"].items():
        assert np.array_equal(v, sb["posterior"][key], equal_nan=True), key


def test_ensemble_fit_report_is_the_report_of_its_flat_chain(pkg, F, small):
    E = pkg.ensemble
    start = torch.from_numpy(RS.sn_thetas(pkg, 16, seed=21)).to(DEV)
    ens = E.ShardedEnsemble(small.engine.torch_log_prob(), start, seed=3, moves=(("stretch", 1.0),))
    ens.run_mcmc(7)
    got = ens.fit_report(discard=1, thin=2, thresholds=(1.0, 2.5), center="mean")
    chain = ens.get_chain(discard=1, thin=2, flat=True)
    assert got["stats"].shape == (chain.shape[0], len(F.COLUMNS)) and chain.shape[0] == 3 * 16
    _same_report(got, F.chain_report(small.engine, chain, thresholds=(1.0, 2.5), center="mean"))
    s = got["summary"]
    assert s["dof"] == 65 - 4 and s["n_data"] == 65
    assert np.allclose(s["center"], chain.mean(dim=0).cpu().numpy(), rtol=1e-14)
    assert s["chi2"] == pytest.approx(float(small.chi_squared(s["center"])), rel=1e-12)
    stats = got["stats"].cpu().numpy()
    for j, name in enumerate(F.COLUMNS[:-1]):
        assert np.array_equal(s["posterior"][name], np.percentile(stats[:, j], [15.9, 50, 84.1])), name
    # the same engine given explicitly
    _same_report(got, ens.fit_report(discard=1, thin=2, thresholds=(1.0, 2.5), center="mean", engine=small.engine))


def test_nested_fit_report_is_the_weighted_report_of_its_posterior(pkg, F, union3):
    nested = pkg.nested
    p = nested.Prior()
    p.add_parameter("dM", dist=(-1, +1))
    p.add_parameter("om", dist=(0.1, 0.7))
    p.add_parameter("v", dist=(-9, 9))
    s = nested.DeviceNestedSampler(p, union3.engine.torch_log_prob(pkg.CF_OUT_LOGL), n_live=60, seed=5)
    s.run(f_live=0.2)
    pts, log_w, _ = s.posterior()
    x, w = torch.from_numpy(np.ascontiguousarray(pts)).to(DEV), torch.from_numpy(np.exp(log_w)).to(DEV)
    got = s.fit_report(thresholds=(2.0,))
    _same_report(got, F.chain_report(union3.engine, x, weights=w, thresholds=(2.0,)))
    assert got["summary"]["dof"] == 22 - 3                                            # sn/union3_1.py:102
    d = got["datum"]
    assert d["exceed"].shape == (1, 22) and np.allclose(d["w_sum"], float(w.sum()), rtol=1e-12)
    assert np.array_equal(d["z"], golden("sn_union3_1")["z_cmb"])
    np.testing.assert_allclose(d["sigma"], np.sqrt(np.diag(golden("sn_union3_1")["cov"])), rtol=1e-12)


# ---- 6. the workspace ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [16, 150, 257])
def test_evaluations_around_a_report_return_the_same_bits(pkg, F, small, W):
    f = small.engine.torch_log_prob()
    theta = torch.from_numpy(RS.sn_thetas(pkg, W, seed=30 + W)).to(DEV)
    before = f(theta).clone()
    F.report(small.engine, torch.from_numpy(RS.sn_thetas(pkg, 100, seed=31)).to(DEV))
    after = f(theta).clone()
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    host = small.engine.log_probability(theta.cpu().numpy())
    np.testing.assert_allclose(host, after.cpu().numpy(), rtol=1e-12)


# ---- what the entry point refuses ----------------------------------------------------------------------------------------------
def test_refusals_on_real_handles(pkg, F, small):
    L, lib = pkg._lib, pkg.lib()
    x = torch.from_numpy(RS.sn_thetas(pkg, 4)).to(DEV)
    out = torch.empty((4, L.CF_RS_NCOL), dtype=torch.float64, device=DEV)

    def call(engine, block=L.CF_RB_SN, S=4, theta=x.data_ptr(), n_thr=0):
        return lib.cf_resid_device(engine._h, theta, S, None, block, None, n_thr, out.data_ptr(), None, None, None)

    assert call(small.engine) == 0
    assert call(small.engine, block=L.CF_RB_BAO) == -1 and b"no BAO block" in lib.cf_last_error()
    assert call(small.engine, S=-1) == -1 and call(small.engine, theta=None) == -1 and call(small.engine, n_thr=5) == -1
    assert call(small.engine, S=0, theta=None) == 0
    sigma = np.empty(65)
    assert lib.cf_resid_sigma(small.engine._h, L.CF_RB_BAO, sigma.ctypes.data) == -1
    assert lib.cf_resid_set_chunk(small.engine._h, 65537) == -1 and lib.cf_resid_set_chunk(small.engine._h, 0) == 0
    syn = pkg.synthetic.pantheon_like(n_sn=65, seed=5)
    two = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"], devices=[0, 0])
    try:
        assert call(two.engine) == -5 and b"several devices" in lib.cf_last_error()
        with pytest.raises(ValueError, match="several devices"):
            F.sample_stats(two.engine, x)
    finally:
        two.engine.close()
    import quasar_shapes as QS

    c = QS.build_case(0)
    qe = pkg.LikelihoodEngine(**QS.engine_kwargs(c, pkg.Param, pkg.engine.solve_mode_of(c["solve"])))
    try:
        th = torch.from_numpy(np.ascontiguousarray(c["theta"][:1])).to(DEV)
        for block in (L.CF_RB_SN, L.CF_RB_BAO):
            assert lib.cf_resid_device(qe._h, th.data_ptr(), 1, None, block, None, 0, out.data_ptr(), None, None, None) == -5
            assert b"quasar" in lib.cf_last_error()
        with pytest.raises(ValueError, match="quasar engine"):
            F.sample_stats(qe, th)
    finally:
        qe.close()
