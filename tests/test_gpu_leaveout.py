"""GPU (-m gpu): leave-group-out fits end to end, deterministic.  An SN engine and the engine rebuilt from the data without a
group: ``chi^2_full - q_B = chi^2_sub`` and, on a fixed set of theta rows weighted by exp(log P_full), the reweighted mean and
covariance equal those under exp(log P_sub) (an identity: no Monte-Carlo error).  The same chi^2 identity for the DESI BAO block
without one tracer.  On the real Union3.1 data the 22 singleton bins reproduce ``influence``'s deletion column."""
import numpy as np
import pytest
import torch

import infl_reference as IR
import leaveout_reference as LR
import resid_shapes as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble


@pytest.fixture(scope="module")
def LO(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.leaveout


def _sn_pair(pkg, n):
    """(full mirror, mirror without the group, group): the highest-redshift datum stays out of the group, so both engines
    integrate on the same grid (it ends at max(z) + 0.1; a different grid moves chi^2 by 1e-8)."""
    lk, syn = RS.sn_likelihood(pkg, n)
    top = int(np.argmax(syn["z_cmb"]))
    rest = np.setdiff1d(np.arange(n), [top])
    group = np.random.default_rng(n).permutation(rest)[:max(1, n // 4)].astype(np.int32)
    keep = np.setdiff1d(np.arange(n), group)
    sub = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"][keep], syn["z_hel"][keep], syn["obs"][keep],
                                             chol=np.linalg.cholesky(syn["cov"][np.ix_(keep, keep)]))
    return lk, sub, group


@pytest.mark.parametrize("n", [65, 257])
def test_sn_chi2_without_a_group_is_the_rebuilt_engines(pkg, LO, n):
    lk, sub, group = _sn_pair(pkg, n)
    try:
        theta = RS.sn_thetas(pkg, 33)
        q, dof = LO.group_chi2(lk.engine, torch.from_numpy(theta).to(DEV), [group, group[::-1].copy()], "sn")
        q = q.cpu().numpy()
        full, want = lk.engine.chi_squared(theta), sub.engine.chi_squared(theta)
        rel = np.abs((full - q[:, 0]) - want) / full
        print("n = %d, m = %d: chi2_full - q_B against the engine without B, largest difference %.2e of chi^2" % (n, group.size, rel.max()))
        assert rel.max() <= 1e-10 and dof.tolist() == [group.size] * 2 and (q > 0).all()
        assert np.max(np.abs(q[:, 1] / q[:, 0] - 1)) <= 1e-10                      # the order inside a group does not matter
        # pieces of g: the same bits whatever the piece size
        with LO.Groups(lk.engine, [group], "sn") as G:
            q1 = LO.group_chi2(lk.engine, theta, G, "sn")[0].cpu().numpy()
            q2 = LO.group_chi2(lk.engine, theta, G, "sn", piece=7)[0].cpu().numpy()
        assert np.array_equal(q1.view(np.uint64), q2.view(np.uint64)) and np.array_equal(q1[:, 0].view(np.uint64), q[:, 0].view(np.uint64))
    finally:
        lk.engine.close()
        sub.engine.close()


def test_reweighted_moments_equal_the_posterior_of_the_rebuilt_engine(pkg, LO):
    """4096 fixed theta rows with base weights exp(log P_full): ``leave_group_out``'s mean and covariance against the moments
    under exp(log P_sub) in long double, within 1e-9 of the column's std."""
    lk, sub, group = _sn_pair(pkg, 65)
    try:
        theta = RS.sn_thetas(pkg, 4096, seed=21)
        full, part = lk.engine.chi_squared(theta), sub.engine.chi_squared(theta)
        w_full = np.exp(-0.5 * (full - full.min()))
        out = LO.leave_group_out(lk.engine, torch.from_numpy(theta).to(DEV), [group], "sn", weights=torch.from_numpy(w_full).to(DEV),
                                 theta_ref=theta[int(np.argmin(full))])
        w = np.exp(-0.5 * (part - part.min()).astype(LD))
        w /= w.sum()
        mean = (w[:, None] * theta).sum(axis=0)
        d = theta - mean[None, :]
        cov = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0)
        std = np.sqrt(np.diag(cov)).astype(np.float64)
        e_mean = np.abs(np.asarray(out["mean"][0] - mean, dtype=np.float64)) / std
        e_cov = np.abs(np.asarray(out["cov"][0] - cov, dtype=np.float64)) / np.outer(std, std)
        print("reweighted against direct: mean %.2e, covariance %.2e of the std; ESS %.1f of %.1f, khat %.2f"
              % (e_mean.max(), e_cov.max(), out["ess"][0], out["ess"][0] / out["ess_fraction"][0], out["khat"][0]))
        assert e_mean.max() <= 1e-9 and e_cov.max() <= 1e-9
        ess_direct = float(1.0 / (w * w).sum())
        assert out["ess"][0] == pytest.approx(ess_direct, rel=1e-8)
        # the full-data columns and the summary columns
        wf = w_full / w_full.sum()
        assert np.allclose(out["mean_full"], (wf[:, None] * theta).sum(axis=0), rtol=0, atol=1e-9 * std.max())
        assert np.allclose(out["shift_sigma"][0], (out["mean"][0] - out["mean_full"]) / out["std_full"])
        assert out["q"].shape == (4096, 1) and out["dof"].tolist() == [group.size] and out["n_used"][0] == 4096
        assert out["q_mean"][0] == pytest.approx(float((wf * out["q"][:, 0].cpu().numpy()).sum()), rel=1e-10)
        from scipy.stats import chi2

        assert out["p_ref"][0] == pytest.approx(chi2.sf(out["q_ref"][0], group.size)) and 0 <= out["p_ref"][0] <= 1
        assert out["names"] == ["group0"] and out["log_mean_weight"][0] >= 0      # exp(q / 2) >= 1
        with pytest.raises(TypeError, match="unexpected keyword"):
            LO.chain_leave_group_out(lk.engine, torch.from_numpy(theta).to(DEV), groups=[group], thin=2)
    finally:
        lk.engine.close()
        sub.engine.close()


def test_bao_chi2_without_a_tracer_is_the_rebuilt_engines(pkg, LO):
    lk, g = RS.bao_likelihood(pkg)
    z = np.asarray(g["bao_z"], dtype=np.float64)
    zs = np.unique(z)
    tracer = zs[len(zs) // 2]                                         # a middle tracer: the top redshift keeps the grid
    group = np.nonzero(z == tracer)[0].astype(np.int32)
    keep = np.nonzero(z != tracer)[0]
    A = np.asarray(g["bao_inv_cov"], dtype=LD)
    K = LD(0.5) * (A + A.T)
    # the precision matrix of the data without the tracer is the Schur complement K_AA - K_AB K_BB^-1 K_BA, in long double
    Z = IR.solve_lower(LR.cholesky(K[np.ix_(group, group)]), K[np.ix_(group, keep)])
    inv_sub = np.asarray(K[np.ix_(keep, keep)] - Z.T @ Z, dtype=np.float64)
    sub = pkg.scripts.build("bao/desi_fs_lya.py", bao=(z[keep], np.asarray(g["bao_val"])[keep], np.asarray(g["bao_qty"])[keep], inv_sub))
    try:
        theta = RS.bao_thetas(pkg, 33)
        q, dof = LO.group_chi2(lk.engine, torch.from_numpy(theta).to(DEV), [group], "bao")
        full, want = lk.engine.chi_squared(theta), sub.engine.chi_squared(theta)
        rel = np.abs((full - q[:, 0].cpu().numpy()) - want) / full
        print("BAO, %d data, tracer at z = %g (%d data): chi2_full - q_B against the engine without it, largest difference %.2e of chi^2"
              % (z.size, tracer, group.size, rel.max()))
        assert rel.max() <= 1e-10 and dof.tolist() == [group.size]
    finally:
        lk.engine.close()
        sub.engine.close()


def test_union3_singleton_bins_reproduce_influences_deletion_column(pkg, LO):
    lk, block = RS.fixture_likelihood(pkg, "sn_union3_1")
    try:
        eng = lk.engine
        n = int(eng.n_sn)
        assert n == 22
        box = np.array([(-0.3, 0.3), (0.15, 0.5), (-2.0, 2.0)])            # (dM, Om, v) inside the script's prior box
        theta = torch.from_numpy(pkg.synthetic.walkers(box, 64, seed=3)).to(DEV)
        I = pkg.influence
        before = I.rows(eng, theta, block)
        groups, names = LO.groups_from_labels(np.arange(n))
        out = LO.leave_group_out(eng, theta, groups, block, names=names)
        after = I.rows(eng, theta, block)
        g, kd = before["g"].cpu().numpy(), eng.precision(block).diag()
        drop = (g * g) / kd[None, :]
        q = out["q"].cpu().numpy()
        fin = np.isfinite(drop)
        assert fin.any() and np.array_equal(np.isfinite(q), fin)
        rel = np.abs(q[fin] - drop[fin]) / drop[fin]
        print("Union3.1, 22 singleton bins over %d rows: q against g_i^2 / K_ii, largest difference %.2f eps" % (fin.all(axis=1).sum(), rel.max() / IR.EPS))
        assert rel.max() <= 4 * IR.EPS
        rows = fin.all(axis=1)
        assert np.array_equal(q[rows].argmax(axis=1), before["sample"]["max_drop_index"].cpu().numpy()[rows].astype(np.int64))
        for key in I.WANT:  # sum_b contrib_b and every other row array: unchanged by the pass
            assert np.array_equal(before[key].cpu().numpy().view(np.uint64), after[key].cpu().numpy().view(np.uint64)), key
        chi2 = before["sample"]["chi2"].cpu().numpy()
        assert np.max(np.abs(before["contrib"].cpu().numpy()[rows].sum(axis=1) / chi2[rows] - 1)) <= 1e-10
        assert out["names"] == [str(k) for k in range(n)] and out["dof"].tolist() == [1] * n
        assert out["mean"].shape == (n, eng.ndim) and out["khat"].shape == (n,) and out["reliable"].dtype == bool
    finally:
        lk.engine.close()


def test_samplers_leave_groups_out_of_their_chains(pkg, LO):
    lk, _ = RS.sn_likelihood(pkg, 65)
    u3, _ = RS.fixture_likelihood(pkg, "sn_union3_1")
    try:
        groups = [np.arange(0, 10), np.arange(5, 30)]
        start = torch.from_numpy(RS.sn_thetas(pkg, 16, seed=21)).to(DEV)
        ens = pkg.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), start, seed=3, moves=(("stretch", 1.0),))
        ens.run_mcmc(5)
        got = ens.leave_group_out(discard=1, groups=groups, names=["low", "mid"])
        want = LO.leave_group_out(lk.engine, ens.get_chain(discard=1, flat=True), groups, names=["low", "mid"])
        assert torch.equal(got["q"], want["q"]) and got["q"].shape == (4 * 16, 2) and got["names"] == ["low", "mid"]
        for key in ("mean", "cov", "ess", "khat", "shift_sigma", "width_ratio", "q_mean", "q_std", "dof"):
            assert np.array_equal(got[key], want[key], equal_nan=True), key
        with pytest.raises(TypeError, match="carry no weights"):
            ens.leave_group_out(groups=groups, weights=None)
        with pytest.raises(TypeError, match="unexpected keyword"):
            ens.leave_group_out(groups=groups, thresholds=(1.0,))
        p = pkg.nested.Prior()
        p.add_parameter("dM", dist=(-1, +1))
        p.add_parameter("om", dist=(0.1, 0.7))
        p.add_parameter("v", dist=(-9, 9))
        s = pkg.nested.DeviceNestedSampler(p, u3.engine.torch_log_prob(pkg.CF_OUT_LOGL), n_live=60, seed=5)
        s.run(f_live=0.2)
        pts, log_w, _ = s.posterior()
        x, w = torch.from_numpy(np.ascontiguousarray(pts)).to(DEV), torch.from_numpy(np.exp(log_w)).to(DEV)
        bins = [np.array([k]) for k in (0, 11, 21)]
        got = s.leave_group_out(groups=bins)
        want = LO.leave_group_out(u3.engine, x, bins, weights=w)
        assert torch.equal(got["q"], want["q"])
        for key in ("mean", "std", "ess", "ess_fraction", "khat", "n_used"):
            assert np.array_equal(got[key], want[key], equal_nan=True), key
        # dropping a bin moves the prior-volume points of a nested run by hundreds of units of log-weight: where the weights leave
        # the range of a double the sums are 0 / 0 and the group is flagged, never reported as reliable
        fin = np.isfinite(got["ess"])
        assert fin.any() and (got["ess"][fin] >= 1.0 / got["max_weight_share"][fin] - 1e-9).all() and (got["ess_fraction"][fin] > 0).all()
        assert not got["reliable"][~fin].any() and np.isinf(got["khat"][~fin]).all()
        with pytest.raises(TypeError, match="its own posterior weights"):
            s.leave_group_out(groups=bins, weights=w)
    finally:
        lk.engine.close()
        u3.engine.close()
