"""GPU (-m gpu): template scans as a user calls them (``scan.TemplateScan`` over ``cf_scan_eval_device``) on SN engines of 63,
65 and 257 SNe and the joint SN + BAO + CMB shape of the nuisance tests: rows and map against the long-double restatement
(tests/scan_reference.py) applied to ``engine.parts``' own residual rows; the same bits across the library's chunks and device /
host pointers; dchi2_k against ``LinearNuisance(mode="profile")`` with and without the candidate; ``singles`` against
``influence``'s z_i; a planted signal; the null distribution and the look-elsewhere p-value; the cosmology Jacobian in the base.
The kernels themselves are judged in tests/test_gpu_scan_kernels.py."""
import numpy as np
import pytest
import torch

import infl_reference as IR
import marg_reference as MR
import resid_shapes as RS
import scan_reference as SR
import scan_shapes as SS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = SR.LD
F64 = lambda x: np.asarray(x, dtype=np.float64)
N_GROUPS = 12


@pytest.fixture(scope="module")
def SC(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.scan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sn_engine(pkg, n, obs_shift=None):
    syn = pkg.synthetic.pantheon_like(n_sn=n, seed=5, rank=min(40, n))
    obs = syn["obs"] if obs_shift is None else syn["obs"] + obs_shift
    lk = pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], obs, chol=syn["chol"])
    return lk.engine, syn, RS.sn_thetas(pkg, SS.S_MAX)


def _joint_engine(pkg):
    """n_sn 65, 13 BAO data, Planck + ACT compression, thawing dark energy (the joint shape of tests/test_gpu_marg.py)."""
    from conftest import golden

    LK = pkg.likelihoods
    g = golden("bao_desi_cmb_des5y")
    syn = pkg.synthetic.pantheon_like(n_sn=65, seed=7, rank=40)
    inv = np.linalg.inv(g["bao_cov"][:13, :13])
    inv = 0.5 * (inv + inv.T)
    full = LK.DesiCmbDes5y(syn["z_cmb"], syn["z_hel"], syn["obs"], None, g["bao_z"][:13], g["bao_val"][:13], g["bao_qty"][:13], inv,
                           chol=syn["chol"], comp=dict(pkg.cmb_data.PLANCK_ACT), fde="thawing")
    box = np.array([(-19.5, -19.2), (64.0, 72.0), (0.0215, 0.0232), (0.112, 0.126), (-1.0, 1.0), (-0.99, -0.6)])
    return full.engine, syn, pkg.synthetic.walkers(box, 65, seed=12)


def _family(SC, syn):
    """Steps at eight redshifts, the windows of one and two out of six bins, twelve interleaved groups and all the data as one
    group (the offset again: dead).  No two of them are complements of each other: with the offset in the base those would tie."""
    Cd, z = SC.Candidates, syn["z_cmb"]
    q = np.quantile(z, np.linspace(0.1, 0.9, 8))
    return Cd.stack(Cd.steps(z, q), Cd.windows(z, np.quantile(z, np.linspace(0.0, 1.0, 7)) * [1, 1, 1, 1, 1, 1, 1.001], max_bins=2),
                    Cd.labels(np.arange(z.size) % N_GROUPS), Cd.labels(np.zeros(z.size, dtype=np.int64)))


class Case:
    """One engine, its rows of theta, the residual rows of ``engine.parts`` for them, a family of candidates scanned on top of
    the offset, and the restatement -- built once and shared."""

    def __init__(self, pkg, SC, name):
        self.name = name
        self.eng, self.syn, theta = _joint_engine(pkg) if name == "joint" else _sn_engine(pkg, int(name))
        self.theta = np.ascontiguousarray(theta)
        self.td = _dev(self.theta)
        n = self.eng.n_sn
        self.base = np.ones((n, 1))
        self.cand, self.table = _family(SC, self.syn)
        self.sk = np.full(self.cand.shape[1], np.inf)
        self.sk[2::5] = 0.3
        self.ts = SC.TemplateScan(self.eng, (self.cand, self.table), base=self.base, cand_sigma=self.sk)
        self.rows = self.eng.parts(self.theta)["delta"]
        self.chi2 = self.eng.chi_squared(self.theta)
        self.ref = SR.restate(self.syn["chol"], self.cand, self.rows, base=self.base, cand_sigma=self.sk)
        self.tol = SR.BAR * SR.scale(self.ts.info["V"], self.rows)

    def close(self):
        self.ts.close()
        self.eng.close()


_CASES = {}


def _case(pkg, SC, name):
    if name not in _CASES:
        _CASES[name] = Case(pkg, SC, name)
    return _CASES[name]


@pytest.fixture(scope="module", params=[str(n) for n in SS.N_ENGINE] + ["joint"])
def case(request, pkg, SC):
    return _case(pkg, SC, request.param)


@pytest.fixture(scope="module")
def small(pkg, SC):
    return _case(pkg, SC, "65")


def test_rows_and_map_against_the_restatement(pkg, SC, case):
    ts, ref = case.ts, case.ref
    assert np.array_equal(ts.info["live"], ref["live"]) and not hasattr(ts, "engine")
    assert not ts.info["live"][-1] and ts.info["live"][:-1].all()             # all the data as one group: spanned by the offset
    m = ts.map(case.td).cpu().numpy()
    r = {k: v.cpu().numpy() for k, v in ts.torch_rows(case.td).items()}
    e_map = float(np.max(np.abs(F64(m - ref["s"])) / case.tol[:, None]))
    top, k, s_top, gap = SR.best(ref["s"], ref["live"], 0)
    best_tol = 2.0 * case.tol * np.abs(F64(s_top))
    excused = (gap > 0) & (gap <= 2.0 * best_tol)
    agree = r["best_k"] == k
    e_best = float(np.max(np.abs(F64(r["best"] - top)) / best_tol))
    print("%s engine: map %.2e of the terms summed, best %.2e of 2 |s| x that, %d rows excused" % (case.name, e_map * SR.BAR, e_best * SR.BAR, int(excused.sum())))
    assert np.isfinite(m).all() and e_map <= 1.0 and e_best <= 1.0
    assert excused.mean() <= SS.EXCUSED_MAX and (agree | excused).all()
    assert (np.abs(F64(r["s_best"] - s_top))[agree] <= case.tol[agree]).all()
    assert (np.abs(r["chi2"] - case.chi2) <= SR.BAR * np.abs(case.chi2)).all()  # the engine's own chi^2, by the accessor path
    stat = np.where(ts.info["live"][None, :], m * m, -1.0)
    assert np.array_equal(_bits(r["best"]), _bits(stat.max(axis=1))) and np.array_equal(r["best_k"], stat.argmax(axis=1))
    # alpha_hat and its error
    a, err = ts.alpha_hat(m)
    lv = ref["live"]
    assert (np.abs(F64(a[:, lv] - ref["alpha_hat"][:, lv])) <= case.tol[:, None] * F64(ref["alpha_err"][lv])[None, :] * (1 + 1e-9)).all()
    assert np.allclose(err[lv], F64(ref["alpha_err"][lv]), rtol=1e-9, atol=0)


def test_same_bits_across_chunks_and_pointers(pkg, SC, case):
    ts, eng = case.ts, case.eng
    want = {k: v.cpu().numpy() for k, v in ts.torch_rows(case.td).items()}
    want_map = ts.map(case.td).cpu().numpy()
    try:
        for chunk in SS.CHUNKS:
            SC.set_library_chunk(eng, chunk)
            got = {k: v.cpu().numpy() for k, v in ts.torch_rows(case.td).items()}
            assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in ("best", "s_best", "chi2")), (case.name, chunk)
            assert np.array_equal(got["best_k"], want["best_k"]) and np.array_equal(_bits(ts.map(case.td).cpu().numpy()), _bits(want_map))
    finally:
        SC.set_library_chunk(eng, 0)
    host = ts.rows(case.theta)                                                # host pointers
    assert all(np.array_equal(_bits(host[k]), _bits(want[k])) for k in ("best", "s_best", "chi2")) and np.array_equal(host["best_k"], want["best_k"])
    assert np.array_equal(_bits(ts.map(case.theta)), _bits(want_map))
    one = ts.rows(case.theta[7])                                              # one row, alone
    assert np.array_equal(_bits(one["best"]), _bits(want["best"][7:8])) and one["best_k"][0] == want["best_k"][7]
    # the report: the accumulators of one pass against long-double sums of the device's own map
    w = np.random.default_rng(3).uniform(0.0, 2.0, len(case.theta))
    rep = ts.report(case.td, weights=_dev(w))
    wl, ml = np.asarray(w, dtype=LD), np.asarray(want_map, dtype=LD)
    sw = wl.sum()
    mean = (wl[:, None] * ml).sum(axis=0) / sw
    assert (np.abs(F64(rep["s_mean"] - mean)) <= 1e-10 * F64((wl[:, None] * np.abs(ml)).sum(axis=0) / sw)).all()
    assert (np.abs(F64(rep["dchi2_mean"] - (wl[:, None] * ml * ml).sum(axis=0) / sw)) <= 1e-10 * rep["dchi2_mean"]).all()
    assert abs(rep["w_sum"] - float(sw)) <= 1e-10 * float(sw) and rep["n_bad"] == 0
    wins = np.bincount(want["best_k"], weights=w, minlength=ts.K) / float(sw)
    assert np.allclose(rep["win_fraction"], wins, rtol=1e-12, atol=1e-15) and abs(rep["win_fraction"].sum() - 1.0) <= 1e-12
    assert np.array_equal(_bits(rep["best"].cpu().numpy()), _bits(want["best"])) and rep["best_quantiles"].shape == (5,)
    assert np.array_equal(_bits(ts.report(case.td, weights=_dev(w))["s_mean"]), _bits(rep["s_mean"]))  # the same cut: the same bits


def test_dchi2_against_the_profiled_nuisance_likelihood(pkg, SC, case):
    """s_k^2 is chi2_prof(base) - chi2_prof(base + a_k) of ``LinearNuisance(mode="profile")``.  On the scale of the terms the
    joint projection sums (``marg_reference.scales``: chi^2 + sum_j (sum_i |r_i| |Wt_ij|)^2, whose last column IS v_k) each of
    the two profiled values is within the bar, and s^2 within 2 |s| times the bar on its own terms, which that scale contains:
    four bars in all."""
    Nu, ts = pkg.nuisance, case.ts
    m = ts.map(case.theta)
    theta = case.theta[:33]
    with Nu.LinearNuisance(case.eng, case.base, mode="profile") as base:
        chi2_base = base.chi_squared(theta)
    live = np.nonzero(ts.info["live"])[0]
    for k in live[np.linspace(0, live.size - 1, 5).astype(int)]:
        sig = [np.inf, case.sk[k]]
        with Nu.LinearNuisance(case.eng, np.column_stack([case.base, case.cand[:, k]]), sigma=sig, mode="profile") as both:
            chi2_both = both.chi_squared(theta)
            _, v_scale, _ = MR.scales(both.info, case.rows[:33], case.chi2[:33])
        err = float(np.max(np.abs(m[:33, k] ** 2 - (chi2_base - chi2_both)) / v_scale))
        print("%s engine, candidate %d (%s): %.2e of the terms summed" % (case.name, k, ts.table[k]["kind"], err))
        assert err <= 4.0 * MR.BAR


def test_singles_without_a_base_are_the_influence_z_scores(pkg, SC, small):
    """Both sides sum n products per score in float64 (at most n EPS of the terms summed each, Higham's bound for a recursive
    sum); the entries of the precision matrix are long-double results rounded once, those of V the results of two float64
    triangular substitutions, whose forward error is at most n EPS of the terms THEY sum: |L^-T| |L^-1| in place of |K|.  Hence
    4 n EPS of sum_j |r_j| (|L^-T| |L^-1|)_ji / sqrt(K_ii)."""
    eng, n = small.eng, small.eng.n_sn
    with SC.TemplateScan(eng, SC.Candidates.singles(n)) as ts:
        theta = small.td[:33]
        m = ts.map(theta).cpu().numpy()
        z = pkg.influence.rows(eng, theta, want=("z",))["z"].cpu().numpy()
        Kl, bound = IR.precision(np.tril(small.syn["chol"]))
        terms = (np.abs(small.rows[:33]) @ F64(bound)) / np.sqrt(F64(np.diag(Kl)))[None, :]
        err = float(np.max(np.abs(m - z) / terms))
        print("singles against influence z: %.2e of the terms summed (bound %.2e)" % (err, 4 * n * SR.EPS))
        assert err <= 4 * n * SR.EPS
        assert np.allclose(ts.info["F"], F64(np.diag(Kl)), rtol=1e-10, atol=0) and ts.info["live"].all()


def test_a_planted_signal_is_named_and_measured(pkg, SC, small):
    eng0, syn = small.eng, small.syn
    theta_ref = np.array(pkg.synthetic.THETA_TRUE, dtype=np.float64)
    groups = SC.Candidates.labels(np.arange(eng0.n_sn) % N_GROUPS)
    with SC.TemplateScan(eng0, groups, base=small.base, base_jacobian=theta_ref) as ts0:
        k_star = 7
        err = float(ts0.alpha_hat(np.zeros(ts0.K))[1][k_star])
        alpha = 6.0 * err
        s0 = ts0.map(theta_ref)[0]
    eng, _, _ = _sn_engine(pkg, 65, obs_shift=alpha * groups[0][:, k_star])
    with SC.TemplateScan(eng, groups, base=small.base, base_jacobian=theta_ref) as ts:
        r = ts.rows(theta_ref)
        s = ts.map(theta_ref)[0]
        a_hat, a_err = ts.alpha_hat(s)
        print("planted %.4f at candidate %d: best_k %d, alpha_hat %.4f +- %.4f (%.2f sigma local)" % (alpha, k_star, r["best_k"][0], a_hat[k_star], a_err[k_star], np.sqrt(r["best"][0])))
        assert r["best_k"][0] == k_star and ts.table[k_star] == dict(kind="label", label=k_star)
        assert abs(a_hat[k_star] - alpha) <= 3.0 * a_err[k_star]
        # the scan is linear in the data: the planted amplitude adds exactly 6 to the score of its own candidate
        assert abs((s[k_star] - s0[k_star]) - 6.0) <= 1e-9
        sig = ts.significance(theta_ref, n_draws=2000, seed=1)
        assert sig["best_k"] == k_star and sig["candidate"]["label"] == k_star and sig["local_sigma"] == pytest.approx(np.sqrt(r["best"][0]))
        assert sig["p_global"] <= 5 / 2001 and sig["n_trials"] > 1.0 and sig["sigma_global"] < sig["local_sigma"]
    eng.close()


def test_null_draws(pkg, SC, small):
    from scipy import stats

    eng, n = small.eng, small.eng.n_sn
    a = small.cand[:, 3]
    with SC.TemplateScan(eng, a[:, None], base=small.base) as one:
        null = one.null(4096, seed=2).cpu().numpy()
        assert null.shape == (4096,) and np.isfinite(null).all() and (null >= 0).all()
        p = stats.kstest(null, stats.chi2(1).cdf).pvalue
        print("K = 1: KS p-value of 4096 null draws against chi^2(1): %.3f" % p)
        assert p > 0.01
        # the same seed: the same bits, in one call or two; another seed: other draws
        two = np.concatenate([one.null(1000, seed=2).cpu().numpy(), one.null(3096, seed=2, row0=1000).cpu().numpy()])
        assert np.array_equal(_bits(two), _bits(null)) and np.array_equal(_bits(one.null(4096, seed=2).cpu().numpy()), _bits(null))
        assert not np.array_equal(one.null(64, seed=3).cpu().numpy(), null[:64])
        assert one.null(0).shape == (0,)
    with SC.TemplateScan(eng, np.column_stack([a, a]), base=small.base) as twice:       # two identical candidates: one trial
        null2 = twice.null(4096, seed=2).cpu().numpy()
        assert np.allclose(null2, null, rtol=1e-9, atol=1e-12)
        for obs in (1.0, 4.0, 6.0):
            g = SC.global_p(obs, null2, level=0.9973)
            lo, hi = g["p_interval"]
            assert lo <= g["p_local"] <= hi, (obs, g)
    with SC.TemplateScan(eng, a[:, None], base=small.base, sign=1) as up:              # one-sided: half the draws score zero
        nu = up.null(4096, seed=2).cpu().numpy()
        assert abs(float((nu == 0).mean()) - 0.5) <= 5 * 0.5 / np.sqrt(4096) and np.array_equal(nu[nu > 0], null[nu > 0])


def test_the_cosmology_jacobian_in_the_base(pkg, SC, small):
    eng = small.eng
    theta_ref = np.array(pkg.synthetic.THETA_TRUE, dtype=np.float64)
    with SC.TemplateScan(eng, small.cand[:, :4], base_jacobian=theta_ref) as first:
        J, kept = first.jacobian, first.jacobian_kept
        assert J.shape == (eng.n_sn, eng.ndim) and 1 <= len(kept) <= eng.ndim and first.base.shape[1] == len(kept)
        # the offset column is -1 (or +1) times ones; H0's is a multiple of it in an SN-only engine: one of the two is kept
        assert np.allclose(np.abs(J[:, 0]), 1.0, atol=1e-6) and 0 in kept and 1 not in kept
    cand = np.column_stack([J[:, kept[-1]], small.cand[:, 0], J[:, 1], J @ np.arange(1.0, eng.ndim + 1)])
    with SC.TemplateScan(eng, cand, base_jacobian=theta_ref) as ts:
        assert list(ts.info["live"]) == [False, True, False, False]
        r = ts.rows(small.theta[:9])
        assert (r["best_k"] == 1).all() and not ts.map(small.theta[:9])[:, [0, 2, 3]].any()
    with pytest.raises(ValueError, match="<= 16"):
        SC.TemplateScan(eng, small.cand[:, :4], base=np.random.default_rng(0).standard_normal((eng.n_sn, 14)), base_jacobian=theta_ref)
    with pytest.raises(ValueError, match="theta_ref"):
        SC.TemplateScan(eng, small.cand[:, :4], base_jacobian=theta_ref[:2])


def test_rejected_rows_and_refusals(pkg, SC, small):
    ts, eng, lib = small.ts, small.eng, pkg.lib()
    bad = small.theta[:4].copy()
    bad[2, 2] = np.nan
    r = ts.rows(bad)
    clean = ts.rows(small.theta[:4])
    keep = [0, 1, 3]
    assert np.isnan(r["best"][2]) and r["best_k"][2] == -1 and np.array_equal(_bits(r["best"][keep]), _bits(clean["best"][keep]))
    th, o = small.td, torch.empty(4, dtype=torch.float64, device=DEV)

    def call(h=eng._h, p=ts._scan._p, theta=th.data_ptr(), S=4, sign=0, best=o.data_ptr(), chi2=None, map_=None, mp=0):
        return lib.cf_scan_eval_device(h, p, theta, S, sign, None, chi2, best, None, None, map_, mp, None, None)

    assert call() == 0 and call(best=None, chi2=o.data_ptr()) == 0
    assert call(p=None) == -1 and b"null cf_scan" in lib.cf_last_error()
    assert call(S=-1) == -1 and call(theta=None) == -1 and call(sign=3) == -1
    assert call(best=None) == -1 and b"no output" in lib.cf_last_error()
    assert call(map_=o.data_ptr(), mp=ts.K - 1) == -1 and b"map pitch below K" in lib.cf_last_error()
    assert call(S=0, theta=None) == 0
    other = SC.Scan(np.ones((64, 2)), device=0)
    assert call(p=other._p) == -1 and b"cf_scan.n is not" in lib.cf_last_error()
    other.close()
    assert lib.cf_scan_set_chunk(eng._h, 65537) == -1 and lib.cf_scan_set_chunk(eng._h, 0) == 0
    torch.cuda.synchronize()
