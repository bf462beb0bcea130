"""GPU (-m gpu): the scaled covariance as a user calls it (``covscale.ScaledCovariance`` over ``cf_cscale_eval_device``) -- the
s = 0 column against the engine itself, three amplitudes against an engine rebuilt from ``cholesky(C0 + s C1)`` plus numpy's
``slogdet`` difference, the same bits across the library's chunks, device and host pointers and ``scan``, one Pantheon+-sized
engine against the long-double restatement, the closed-form best fit of ``C1 = C0``, and a short ensemble run.  The kernels
themselves are judged in tests/test_gpu_cscale_kernels.py."""
import warnings

import numpy as np
import pytest
import torch

import cscale_reference as CR
import cscale_shapes as CS
import resid_shapes as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = (("CHI2", 0), ("LOGL", 1), ("LOGP", 2))


@pytest.fixture(scope="module")
def V(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.covscale


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _joint(pkg):
    """n_sn 65, 13 BAO data, Planck + ACT compression (the joint shape of tests/test_gpu_mock.py)."""
    from conftest import golden

    g = golden("bao_desi_cmb_des5y")
    syn = pkg.synthetic.pantheon_like(n_sn=65, seed=7, rank=40)
    inv = np.linalg.inv(g["bao_cov"][:13, :13])
    data = dict(bao_z=g["bao_z"][:13], bao_val=g["bao_val"][:13], bao_qty=g["bao_qty"][:13], bao_inv=0.5 * (inv + inv.T))

    def build(chol):
        return pkg.likelihoods.DesiCmbDes5y(syn["z_cmb"], syn["z_hel"], syn["obs"], None, data["bao_z"], data["bao_val"], data["bao_qty"],
                                            data["bao_inv"], chol=chol, comp=dict(pkg.cmb_data.PLANCK_ACT), fde="thawing")

    box = np.array([(-19.5, -19.2), (64.0, 72.0), (0.0215, 0.0232), (0.112, 0.126), (-1.0, 1.0), (-0.99, -0.6)])
    return build, syn, pkg.synthetic.walkers(box, 65, seed=12)


class Case:
    """One engine, a second matrix, the ScaledCovariance over them and the rows of theta -- built once per shape and shared."""

    def __init__(self, pkg, V, name):
        self.name = name
        if name == "joint":
            self.build, self.syn, self.theta = _joint(pkg)
            kind = "rank4"
        else:
            n = int(name)
            self.syn = pkg.synthetic.pantheon_like(n_sn=n, seed=5, rank=min(40, n))
            self.build = lambda chol: pkg.sn_pantheon.PantheonLikelihood(self.syn["z_cmb"], self.syn["z_hel"], self.syn["obs"], chol=chol)
            self.theta = RS.sn_thetas(pkg, CS.S_MAX)
            kind = CS.KINDS[CS.N_ENGINE.index(n) % len(CS.KINDS)] if n != 257 else "indefinite"
        self.lk = self.build(self.syn["chol"])
        self.eng = self.lk.engine
        self.c1 = CS.second_matrix(kind, self.syn["cov"])
        self.c1_dense = np.asarray(CR.c1_matrix(self.c1, self.syn["cov"].shape[0]), dtype=np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the wide bounds are cut to the domain on purpose
            self.sc = V.ScaledCovariance(self.eng, self.c1, (-1e6, 1e6))
        lo, hi = self.sc.s_bounds
        self.grid = np.array([0.0, 0.6 * max(lo, -0.5), min(1.0, 0.5 * hi), min(0.05, 0.1 * hi)])
        self.td = _dev(self.theta)

    def close(self):
        self.sc.close()
        self.eng.close()


_CASES = {}


def _case(pkg, V, name):
    if name not in _CASES:
        _CASES[name] = Case(pkg, V, name)
    return _CASES[name]


@pytest.fixture(scope="module", params=[str(n) for n in CS.N_ENGINE] + ["joint"])
def case(request, pkg, V):
    return _case(pkg, V, request.param)


@pytest.fixture(scope="module")
def small(pkg, V):
    """The 65-SN engine (C1 = C0) of the cases above, for the tests one engine is enough for."""
    return _case(pkg, V, "65")


def test_zero_amplitude_is_the_engine(pkg, V, case):
    eng, sc = case.eng, case.sc
    chi2 = eng.chi_squared(case.theta)
    want = {0: chi2, 1: eng.log_likelihood(case.theta), 2: eng.log_probability(case.theta)}
    for name, kind in KINDS:
        got = sc.scan(case.td, [0.0], kind=kind)[:, 0].cpu().numpy()
        err = float(np.max(np.abs(got - want[kind]) / chi2))
        print("%s engine, s = 0, %s: %.2e of chi^2" % (case.name, name, err))
        assert np.isfinite(got).all() and err <= CR.BAR
    p = sc.parts(np.column_stack([case.theta[:9], np.zeros(9)]))
    assert not p["logdet"].any() and (np.abs(p["quad"] - eng.parts(case.theta[:9])["chi2_blocks"][:, 0]) <= CR.BAR * chi2[:9]).all()


def test_three_amplitudes_against_a_rebuilt_engine(pkg, V, case):
    eng, sc = case.eng, case.sc
    C0 = case.syn["chol"] @ case.syn["chol"].T
    ours = {kind: sc.scan(case.td, case.grid, kind=kind).cpu().numpy() for _, kind in KINDS}
    ld0 = np.linalg.slogdet(C0)[1]
    for j in (1, 2, 3):
        s = float(case.grid[j])
        Cs = C0 + s * case.c1_dense
        other = case.build(np.linalg.cholesky(Cs))
        try:
            chi2 = other.engine.chi_squared(case.theta)
            dld = np.linalg.slogdet(Cs)[1] - ld0
            want = {0: chi2, 1: other.engine.log_likelihood(case.theta) - 0.5 * dld, 2: other.engine.log_probability(case.theta) - 0.5 * dld}
        finally:
            other.engine.close()
        for name, kind in KINDS:
            err = float(np.max(np.abs(ours[kind][:, j] - want[kind]) / chi2))
            print("%s engine, s = %.4g, %s against the rebuilt engine: %.2e of chi^2" % (case.name, s, name, err))
            assert err <= 1e-10
    # the other blocks and the prior are the engine's own: what is not SN is unchanged by s
    parts = eng.parts(case.theta)
    rest = eng.chi_squared(case.theta) - parts["chi2_blocks"][:, 0]
    quad = sc.parts(np.column_stack([case.theta, np.full(len(case.theta), case.grid[2])]))["quad"]
    assert (np.abs(ours[0][:, 2] - quad - rest) <= 1e-10 * ours[0][:, 2]).all()
    prior = eng.log_probability(case.theta) - eng.log_likelihood(case.theta)
    assert (np.abs((ours[2][:, 2] - ours[1][:, 2]) - prior) <= 1e-10 * np.abs(ours[2][:, 2])).all()


def test_same_bits_across_chunks_pointers_and_scan(pkg, V, case):
    sc, eng = case.sc, case.eng
    S = len(case.theta)
    grid = np.concatenate([case.grid, np.linspace(case.grid[1], case.grid[2], 15)])  # 19 amplitudes: scan splits them 16 + 3
    for _, kind in KINDS:
        want = sc.scan(case.td, grid, kind=kind).cpu().numpy()
        assert want.shape == (S, 19) and np.isfinite(want).all()
        try:
            for chunk in CS.CHUNKS:
                V.set_library_chunk(eng, chunk)
                assert np.array_equal(_bits(sc.scan(case.td, grid, kind=kind).cpu().numpy()), _bits(want)), (case.name, chunk)
        finally:
            V.set_library_chunk(eng, 0)
        # per-amplitude calls: (row, s_j) does not depend on the other amplitudes of the call
        for j in (0, 3, 15, 16, 18):
            one = sc.scan(case.td, grid[j:j + 1], kind=kind).cpu().numpy()
            assert np.array_equal(_bits(one[:, 0]), _bits(want[:, j])), (case.name, j)
        # host pointers (scan on host numbers goes through the device path; the methods below through cf_cscale_eval)
        ext = np.column_stack([case.theta, np.full(S, grid[2])])
        host = {0: sc.chi_squared, 1: sc.log_likelihood, 2: sc.log_probability}[kind](ext)
        assert np.array_equal(_bits(host), _bits(want[:, 2])), (case.name, "host pointers")
    f = sc.torch_log_prob()
    got = f(_dev(ext)).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(host)) and np.array_equal(_bits(sc.log_probs_vectorized(ext)), _bits(host))
    assert sc.log_probability(ext[0]) == host[0] and isinstance(sc.log_probability(ext[0]), float)
    # outside the bounds of p: -inf; a non-finite theta entry: NaN in that row only
    out = ext[:4].copy()
    out[1, -1], out[2, -1] = sc.p_bounds[1] + 1e-3 * abs(sc.p_bounds[1]), sc.s_range[0] * 1.001  # row 1 leaves the bounds, row 2 the domain
    res = sc.log_probability(out)
    assert res[1] == -np.inf and res[2] == -np.inf and np.array_equal(_bits(res[[0, 3]]), _bits(host[[0, 3]]))
    assert np.isfinite(case.sc.s_range[0]) and sc.log_likelihood(out)[2] == -np.inf  # beyond the domain the likelihood itself is -inf
    assert np.isnan(sc.chi_squared(out)[2])
    bad = ext[:4].copy()
    bad[1, 0] = np.nan
    for fn in (sc.chi_squared, sc.log_likelihood, sc.log_probability):
        r = fn(bad)
        assert np.isnan(r[1]) and np.isfinite(r[[0, 2, 3]]).all()


def test_refusals_on_real_handles(pkg, V, small):
    case = small
    lib, eng, sc = pkg.lib(), case.eng, case.sc
    out = torch.empty((4, 2), dtype=torch.float64, device=DEV)
    s = torch.zeros((4, 2), dtype=torch.float64, device=DEV)

    def call(h=eng._h, p=sc._dec._p, theta=case.td.data_ptr(), amp=s.data_ptr(), n_s=2, S=4, kind=2, o=out.data_ptr()):
        return lib.cf_cscale_eval_device(h, p, theta, amp, n_s, S, kind, o, None, None)

    assert call() == 0
    assert call(p=None) == -1 and b"null cf_cscale" in lib.cf_last_error()
    assert call(S=-1) == -1 and call(theta=None) == -1 and call(amp=None) == -1 and call(n_s=17) == -1 and call(kind=5) == -1
    assert call(o=None) == -1 and b"no output" in lib.cf_last_error()
    assert call(S=0, theta=None, amp=None) == 0
    other = V.Decomposition(np.eye(64), np.ones(64), device=0)
    assert call(p=other._p) == -1 and b"cf_cscale.n is not" in lib.cf_last_error()
    other.close()
    assert lib.cf_cscale_set_chunk(eng._h, 65537) == -1 and lib.cf_cscale_set_chunk(eng._h, 0) == 0
    torch.cuda.synchronize()


def test_pantheon_sized_engine_within_the_bar(pkg, V):
    """n = 1701, 33 rows, the extra scatter of the low-z sample (C1 = the 0/1 diagonal of z <= 0.2, s = 0.12^2) against the
    long-double restatement.  One call of the restatement takes half a minute at this size, so its result is the recorded one
    (tests/cscale_reference.py says how to record it again); the SN chi^2 the engine gave when it was recorded guards that the
    residual rows are still the recorded ones."""
    from conftest import golden

    n, S = CS.N_PANTHEON, CS.S_PANTHEON
    ref = golden(CR.PANTHEON_FIXTURE)
    lk, syn, c1, theta = CR.pantheon_case(pkg, n, S)
    try:
        assert np.array_equal(theta, ref["theta"]) and float(ref["p"]) == CR.PANTHEON_P
        chi2_sn0 = lk.engine.parts(theta)["chi2_blocks"][:, 0]
        assert np.allclose(chi2_sn0, ref["chi2_sn0"], rtol=1e-12, atol=0), "the rows changed: record the fixture again"
        quad = np.asarray(ref["quad_hi"], dtype=CR.LD) + ref["quad_lo"]
        logdet = (np.asarray(ref["logdet_hi"], dtype=CR.LD) + ref["logdet_lo"])[0]
        with V.ScaledCovariance(lk.engine, c1, (0.0, 0.09), power=2) as sc:
            got = sc.parts(np.column_stack([theta, np.full(S, CR.PANTHEON_P)]))
            s = CR.PANTHEON_P ** 2
            assert np.allclose(got["s"], s, rtol=4e-16, atol=0)
            q_scale, l_scale = CR.scales(sc.transform, sc.eigenvalues, lk.engine.parts(theta)["delta"], [s])
            eq = float(np.max(np.abs(np.asarray(got["quad"] - quad, dtype=np.float64)) / q_scale[:, 0]))
            el = float(np.max(np.abs(np.asarray(got["logdet"] - logdet, dtype=np.float64))) / l_scale[0])
            print("n = %d, %d rows: quad %.2e, logdet %.2e of the scale of the terms summed" % (n, S, eq, el))
            assert eq <= CR.BAR and el <= CR.BAR
            assert np.count_nonzero(sc.eigenvalues) == int(c1.sum()) and sc.s_range[1] == np.inf
    finally:
        lk.engine.close()


def test_best_fit_finds_the_closed_form_amplitude(pkg, V, small):
    """C1 = C0 with the engine columns fixed: log L(s) = const - (chi2_0 / (1 + s) + n log1p(s)) / 2 peaks at s* = chi2_0 / n - 1.

    Tolerance, from the optimiser's own stopping rule (optimize.py): it stops when the box-scaled gradient it measures is below
    gtol + gtol_rel |f| (1e-5 + 16 eps |f| / h), and its central differences carry eps |f| / h of rounding noise, so the true
    |dL/du| at the end is at most gtol + 17 eps |f| / h.  With L''(s*) = n / (2 (1 + s*)^2) and u = (s - lo) / width that is
    |s - s*| <= (gtol + 17 eps |f| / h) / (width L''(s*)); a factor 2 covers the quadratic approximation."""
    case, eng = small, small.eng
    n = 65
    theta0 = np.array(pkg.synthetic.THETA_TRUE, dtype=np.float64)[:eng.ndim]
    chi2_0 = float(eng.chi_squared(theta0))
    s_star = chi2_0 / n - 1.0
    lo, hi = -0.8, 3.0
    assert lo < s_star < hi
    with V.ScaledCovariance(eng, case.syn["cov"], (lo, hi)) as sc:
        f = sc.torch_log_prob(pkg.CF_OUT_LOGL)
        box = np.vstack([np.column_stack([theta0 - 1.0, theta0 + 1.0]), [sc.p_bounds]])
        fit = pkg.optimize.best_fit(f, box, n_starts=8, seed=0, fixed={i: float(theta0[i]) for i in range(eng.ndim)})
        assert fit.best_converged
        width = sc.p_bounds[1] - sc.p_bounds[0]
        tol = 2 * (1e-5 + 17 * CR.EPS * abs(fit.log_prob) / 1e-6) / (width * n / (2 * (1 + s_star) ** 2))
        print("best fit s = %.10f, closed form %.10f, difference %.2e (tolerance %.2e)" % (fit.x[-1], s_star, fit.x[-1] - s_star, tol))
        assert abs(fit.x[-1] - s_star) <= tol
        want = eng.log_likelihood(theta0) + 0.5 * chi2_0 - 0.5 * (chi2_0 / (1 + s_star) + n * np.log1p(s_star))
        assert abs(fit.log_prob - want) <= 1e-10 * chi2_0


def test_ensemble_on_the_scaled_likelihood(pkg, V, small):
    eng = small.eng
    d = np.zeros(65)
    d[:30] = 1.0
    with V.ScaledCovariance(eng, d, (0.0, 0.04), power=2) as sc2:
        W = 64
        start_box = np.vstack([np.array([(-19.6, -19.1), (60.0, 80.0), (0.15, 0.5), (-2.0, 2.0)]), [sc2.p_bounds]])
        box = np.vstack([small.lk.bounds, [sc2.p_bounds]])  # the engine's own prior box and the bounds of p
        start = _dev(pkg.synthetic.walkers(start_box, W, seed=3))
        ens = pkg.ensemble.ShardedEnsemble(sc2.torch_log_prob(), start, seed=11, moves=(("stretch", 1.0),))
        ens.run_mcmc(50)
        pos, logp = ens.full_state()
        pos, logp = pos.cpu().numpy(), logp.cpu().numpy()
        chain = ens.get_chain(flat=True).cpu().numpy()
        assert np.isfinite(chain).all() and np.isfinite(ens.get_log_prob(flat=True).cpu().numpy()).all()
        assert ((chain > box[:, 0]) & (chain < box[:, 1])).all()
        again = sc2.log_probability(pos)  # host pointers
        assert np.array_equal(_bits(again), _bits(logp))
        assert np.array_equal(_bits(ens.get_log_prob()[-1].cpu().numpy()), _bits(logp))
