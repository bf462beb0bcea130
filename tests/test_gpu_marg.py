"""GPU (-m gpu): linear SN nuisance parameters in closed form as a user calls them (``nuisance.LinearNuisance`` over
``cf_marg_eval_device``) on engines of 1, 2, 63, 64, 65 and 257 SNe and one joint SN + BAO + CMB shape: every out_kind and both
modes against the long-double restatement (tests/marg_reference.py) applied to ``engine.parts``' own residual rows; the same bits
across the library's chunks and device / host pointers; and, against a SECOND engine that reads the offset from theta, chi2_prof
as that engine's chi^2 at M_ref + alpha_hat, the conditional density of drawn alpha, and the integral over M by quadrature.  The
kernels themselves are judged in tests/test_gpu_marg_kernels.py."""
import numpy as np
import pytest
import torch

import marg_reference as MR
import marg_shapes as MS
import resid_shapes as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = (("CHI2", 0), ("LOGL", 1), ("LOGP", 2))
M_REF = -19.35
LD = MR.LD
F64 = lambda x: np.asarray(x, dtype=np.float64)


@pytest.fixture(scope="module")
def N(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.nuisance


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sn_pair(pkg, n):
    """(full likelihood: theta = (M, H0, Om, v); reduced engine: theta' = (H0, Om, v) with the offset fixed at M_REF)."""
    SP, Param = pkg.sn_pantheon, pkg.Param
    syn = pkg.synthetic.pantheon_like(n_sn=n, seed=5, rank=min(40, n))
    full = SP.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    red = pkg.LikelihoodEngine(ndim=3, z_max=full.z_max, n_grid=SP.N_GRID,
                               params=dict(offset=Param(fixed=M_REF), H0=Param(0), Om=Param(1), v=Param(2)),
                               sn=dict(z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"], z_turn=SP.Z_TURN),
                               bounds=SP.bounds[1:], gauss=[(0,) + tuple(SP.H0_PRIOR[1:])])
    return full.engine, red, syn, RS.sn_thetas(pkg, MS.S_MAX)


def _joint_pair(pkg):
    """n_sn 65, 13 BAO data, Planck + ACT compression, thawing dark energy (the joint shape of tests/test_gpu_cscale.py)."""
    from conftest import golden

    LK, Param = pkg.likelihoods, pkg.Param
    g = golden("bao_desi_cmb_des5y")
    syn = pkg.synthetic.pantheon_like(n_sn=65, seed=7, rank=40)
    inv = np.linalg.inv(g["bao_cov"][:13, :13])
    inv = 0.5 * (inv + inv.T)
    comp = dict(pkg.cmb_data.PLANCK_ACT)
    full = LK.DesiCmbDes5y(syn["z_cmb"], syn["z_hel"], syn["obs"], None, g["bao_z"][:13], g["bao_val"][:13], g["bao_qty"][:13], inv,
                           chol=syn["chol"], comp=comp, fde="thawing")
    red = pkg.LikelihoodEngine(
        ndim=5, z_max=full.z_max, n_grid=LK.N_GRID, ez_model=pkg._lib.CF_EZ_PHYSICAL, fde=LK.FDE_BY_NAME["thawing"],
        params=dict(offset=Param(fixed=M_REF), H0=Param(0), obh2=Param(1), och2=Param(2), v=Param(3), w0=Param(4)),
        sn=dict(z_cmb=syn["z_cmb"], z_hel=syn["z_hel"], obs=syn["obs"], chol=syn["chol"], z_turn=0.10563),
        bao=dict(z=g["bao_z"][:13], val=g["bao_val"][:13], qty=g["bao_qty"][:13], inv_cov=inv, rd_fit=comp["rd_fit"], dh_exact=False),
        cmb=dict(mode=comp["cmb_mode"], prior=comp["cmb_prior"], inv_cov=comp["cmb_inv_cov"], zstar_fit=comp["zstar_fit"]),
        physical=LK._physical(comp))
    box = np.array([(-19.5, -19.2), (64.0, 72.0), (0.0215, 0.0232), (0.112, 0.126), (-1.0, 1.0), (-0.99, -0.6)])
    return full.engine, red, syn, pkg.synthetic.walkers(box, 65, seed=12)


class Case:
    """One shape: the engine that samples the offset, the one that holds it at M_REF, the rows of theta, the offset marginalised
    with a flat prior (``one``) and a set of named templates under a mixed prior in both modes -- built once and shared."""

    def __init__(self, pkg, N, name):
        self.name = name
        self.full, self.eng, self.syn, theta = _joint_pair(pkg) if name == "joint" else _sn_pair(pkg, int(name))
        self.theta_full = np.ascontiguousarray(theta)
        self.theta = np.ascontiguousarray(theta[:, 1:])
        self.td = _dev(self.theta)
        n = self.eng.n_sn
        self.one = N.LinearNuisance(self.eng, N.Templates.offset(n), slots=("offset",))
        kind = MS.KINDS[(MS.N_ENGINE.index(n) if name != "joint" else 3) % len(MS.KINDS)]
        self.A = MS.templates(kind, n)
        self.prior = MS.prior("mixed", n, self.A.shape[1])
        self.lns = {mode: N.LinearNuisance(self.eng, self.A, *self.prior, mode=mode) for mode in ("profile", "marginal")}
        self.rows = self.eng.parts(self.theta)["delta"]
        self.e = {0: self.eng.chi_squared(self.theta), 1: self.eng.log_likelihood(self.theta), 2: self.eng.log_probability(self.theta)}

    def close(self):
        for ln in (self.one, *self.lns.values()):
            ln.close()
        self.eng.close()
        self.full.close()


_CASES = {}


def _case(pkg, N, name):
    if name not in _CASES:
        _CASES[name] = Case(pkg, N, name)
    return _CASES[name]


@pytest.fixture(scope="module", params=[str(n) for n in MS.N_ENGINE] + ["joint"])
def case(request, pkg, N):
    return _case(pkg, N, request.param)


@pytest.fixture(scope="module")
def small(pkg, N):
    return _case(pkg, N, "65")


def _reference_values(ref, e, kind, mode):
    """The restatement's value of (kind, mode) from the engine's own value e of that kind, long double."""
    e = np.asarray(e, dtype=LD)
    if kind == 0:
        return (e - ref["chi2_0"]) + ref["chi2_prof"]
    return e + ref["dlogl"] if mode == "marginal" else e - LD(0.5) * (ref["chi2_prof"] - ref["chi2_0"])


def test_values_against_the_restatement(pkg, N, case):
    for label, A, prior, lns in (("named templates", case.A, case.prior, case.lns),
                                 ("offset", N.Templates.offset(case.eng.n_sn), (None, None, None), dict(marginal=case.one))):
        ref = MR.restate(case.syn["chol"], A, case.rows, *prior)
        proj = next(iter(lns.values())).info
        _, v_scale, a_scale = MR.scales(proj, case.rows, case.e[0])
        for mode, ln in lns.items():
            for kname, kind in KINDS:
                got = ln._device(case.td, kind)[0].cpu().numpy()
                want = _reference_values(ref, case.e[kind], kind, mode)
                err = float(np.max(np.abs(F64(got - want)) / v_scale))
                print("%s engine, %s, %s, %s: %.2e of the terms summed" % (case.name, label, mode, kname, err))
                assert np.isfinite(got).all() and err <= MR.BAR
        a_hat = ln.conditional(case.td)[0].cpu().numpy()
        err = float(np.max(np.abs(F64(a_hat - ref["alpha_hat"])) / a_scale))
        print("%s engine, %s, alpha_hat: %.2e of the terms summed" % (case.name, label, err))
        assert err <= MR.BAR
        assert (np.abs(F64(ln.cov - ref["Finv"])) <= 1e-10 * np.abs(F64(ref["Finv"])).max()).all()


def test_same_bits_across_chunks_and_pointers(pkg, N, case):
    eng = case.eng
    for mode, ln in case.lns.items():
        for _, kind in KINDS:
            want = ln._device(case.td, kind)[0].cpu().numpy()
            alpha = ln.conditional(case.td)[0].cpu().numpy()
            draw = ln.recover(case.td, seed=3).cpu().numpy()
            try:
                for chunk in MS.CHUNKS:
                    N.set_library_chunk(eng, chunk)
                    assert np.array_equal(_bits(ln._device(case.td, kind)[0].cpu().numpy()), _bits(want)), (case.name, chunk)
                    assert np.array_equal(_bits(ln.conditional(case.td)[0].cpu().numpy()), _bits(alpha)), (case.name, chunk)
                    assert np.array_equal(_bits(ln.recover(case.td, seed=3).cpu().numpy()), _bits(draw)), (case.name, chunk)
            finally:
                N.set_library_chunk(eng, 0)
            host = {0: ln.chi_squared, 1: ln.log_likelihood, 2: ln.log_probability}[kind](case.theta)  # host pointers
            assert np.array_equal(_bits(host), _bits(want)), (case.name, "host pointers")
            assert np.array_equal(_bits(ln.conditional(case.theta)[0]), _bits(alpha))
            assert np.array_equal(_bits(ln.recover(case.theta, seed=3)), _bits(draw))
    ln = case.lns["marginal"]
    f = ln.torch_log_prob()
    assert not hasattr(f, "engine")
    logp = ln.log_probability(case.theta)
    assert np.array_equal(_bits(f(case.td).cpu().numpy()), _bits(logp)) and np.array_equal(_bits(ln.log_probs_vectorized(case.theta)), _bits(logp))
    assert ln.log_probability(case.theta[0]) == logp[0] and isinstance(ln.log_probability(case.theta[0]), float)
    # a chain recovered in two pieces is the chain recovered at once
    S = len(case.theta)
    cut = S // 3
    whole = ln.recover(case.td, seed=9, row0=40).cpu().numpy()
    pieces = np.concatenate([ln.recover(case.td[:cut], seed=9, row0=40).cpu().numpy(),
                             ln.recover(case.td[cut:], seed=9, row0=40 + cut).cpu().numpy()])
    assert np.array_equal(_bits(whole), _bits(pieces)) and not np.array_equal(whole, ln.recover(case.td, seed=10, row0=40).cpu().numpy())


def test_against_an_engine_that_samples_the_offset(pkg, N, case):
    """chi2_prof and the conditional density against the second engine, both to 1e-10 of the largest chi^2 involved."""
    one, full = case.one, case.full
    a_hat = one.conditional(case.theta)[0][:, 0]
    at_hat = case.theta_full.copy()
    at_hat[:, 0] = M_REF + a_hat
    chi2_full = full.chi_squared(at_hat)
    prof = one.chi_squared(case.theta)
    # the chi^2 involved: the full engine's at the minimum and the one at M_ref that chi2_prof is formed from
    err = float(np.max(np.abs(prof - chi2_full)) / max(np.max(chi2_full), np.max(case.e[0])))
    print("%s engine: chi2_prof against the full engine at M_ref + alpha_hat: %.2e of the largest chi^2" % (case.name, err))
    assert err <= 1e-10
    # it is the minimum over M
    for d in (-1e-3, 1e-3):
        off = at_hat.copy()
        off[:, 0] += d
        assert (full.chi_squared(off) > chi2_full).all()
    # drawn alpha: ln L_full(theta', M_ref + alpha) - ln L_marg(theta') = ln N(alpha; alpha_hat, F^-1)
    alpha = one.recover(case.theta, seed=1)
    drawn = case.theta_full.copy()
    drawn[:, 0] = M_REF + alpha[:, 0]
    lhs = np.asarray(full.log_likelihood(drawn), dtype=LD) - np.asarray(one.log_likelihood(case.theta), dtype=LD)
    ref = MR.restate(case.syn["chol"], N.Templates.offset(case.eng.n_sn), case.rows)
    dens = MR.conditional_logpdf(ref, alpha, ref["alpha_hat"])
    top = max(float(np.max(full.chi_squared(drawn))), float(np.max(case.e[0])))
    err = float(np.max(np.abs(F64(lhs - dens))) / top)
    print("%s engine: conditional log-density of drawn alpha: %.2e of the largest chi^2" % (case.name, err))
    assert err <= 1e-10
    # the draws scatter as F^-1 says: the standardised draws have unit variance (a 6 sigma band on 257 / 65 draws of chi^2_1)
    z = (alpha[:, 0] - a_hat) / np.sqrt(one.cov[0, 0])
    assert abs(np.mean(z * z) - 1.0) <= 6.0 * np.sqrt(2.0 / z.size)


def test_the_integral_over_the_offset_by_quadrature(pkg, N, case):
    """The 2001-point trapezoid of the second engine's exp(ln L) over M, +-12 conditional sigma about M_ref + alpha_hat,
    reproduces ln L_marg to 1e-10 of the largest chi^2 on the grid (the engine's own parity bar on the terms summed; the
    quadrature error of the trapezoid rule on a Gaussian at this step is below 1e-30)."""
    one, full = case.one, case.full
    rows = np.arange(0, len(case.theta), max(1, len(case.theta) // 8))[:8]
    a_hat = one.conditional(case.theta[rows])[0][:, 0]
    sd = float(np.sqrt(one.cov[0, 0]))
    marg = one.log_likelihood(case.theta[rows])
    u = np.linspace(-12.0, 12.0, 2001)
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    worst = 0.0
    for i, r in enumerate(rows):
        grid = M_REF + a_hat[i] + sd * u
        th = np.repeat(case.theta_full[r][None, :], grid.size, axis=0)
        th[:, 0] = grid
        logl = full.log_likelihood(th)
        top = logl.max()
        got = top + np.log(trapezoid(np.exp(logl - top), grid))
        worst = max(worst, abs(got - marg[i]) / float(np.max(full.chi_squared(th))))
    print("%s engine: ln of the trapezoid over M against ln L_marg: %.2e of the largest chi^2 on the grid" % (case.name, worst))
    assert worst <= 1e-10


def test_rejected_rows_and_refusals(pkg, N, small):
    case, ln = small, small.lns["marginal"]
    lib, eng = pkg.lib(), case.eng
    clean = ln.log_probability(case.theta[:6])
    a_clean = ln.conditional(case.theta[:6])[0]
    out = case.theta[:6].copy()
    out[1, 0] = 95.0   # H0 beyond its box
    out[4, 1] = -0.1   # Om below its box
    res, a = ln.log_probability(out), ln.conditional(out)[0]
    keep = np.array([0, 2, 3, 5])
    assert res[1] == -np.inf and res[4] == -np.inf and np.array_equal(_bits(res[keep]), _bits(clean[keep]))
    # conditional() asks for the likelihood: the box does not reject there; through LOGP the rejected rows have NaN alpha
    al = np.empty((6, ln.m))
    pkg._lib.check(lib.cf_marg_eval(eng._h, ln._proj._p, out.ctypes.data, 6, 2, 1, None, None, al.ctypes.data))
    assert np.isnan(al[[1, 4]]).all() and np.array_equal(_bits(al[keep]), _bits(a_clean[keep])) and np.array_equal(_bits(a[keep]), _bits(a_clean[keep]))
    bad = case.theta[:4].copy()
    bad[2, 1] = np.nan
    for fn in (ln.chi_squared, ln.log_likelihood):
        r = fn(bad)
        assert not np.isfinite(r[2]) and np.isfinite(r[[0, 1, 3]]).all()
    assert np.isnan(ln.conditional(bad)[0][2]).all()
    mass = small.one.box_mass(case.theta[:6])
    assert mass.shape == (6, 1) and np.isnan(mass).all()  # no box given: nothing to report
    with N.LinearNuisance(eng, N.Templates.offset(eng.n_sn), box=[(-20.0 - M_REF, -19.0 - M_REF)]) as boxed:
        from scipy import stats

        mass = boxed.box_mass(case.td[:6]).cpu().numpy()
        a_hat, sd = boxed.conditional(case.theta[:6])[0], np.sqrt(boxed.cov[0, 0])
        want = stats.norm.cdf((-19.0 - M_REF - a_hat) / sd) - stats.norm.cdf((-20.0 - M_REF - a_hat) / sd)
        assert mass.shape == (6, 1) and ((mass >= 0.0) & (mass <= 1.0)).all() and (np.abs(mass - want) <= 1e-12).all()
        assert (np.abs(boxed.box_mass(case.theta[:6]) - want) <= 1e-12).all()  # host numbers in, numpy out
        assert abs((boxed.log_likelihood(case.theta[0]) - small.one.log_likelihood(case.theta[0])) - 0.0) <= 1e-12  # width 1: ln 1
    th, o = case.td, torch.empty(4, dtype=torch.float64, device=DEV)

    def call(h=eng._h, p=ln._proj._p, theta=th.data_ptr(), S=4, kind=2, mode=1, out=o.data_ptr(), alpha=None):
        return lib.cf_marg_eval_device(h, p, theta, S, kind, mode, None, out, alpha, None)

    assert call() == 0
    assert call(p=None) == -1 and b"null cf_marg" in lib.cf_last_error()
    assert call(S=-1) == -1 and call(theta=None) == -1 and call(kind=5) == -1 and call(mode=2) == -1
    assert call(out=None) == -1 and b"no output" in lib.cf_last_error()
    assert call(S=0, theta=None) == 0
    other = N.Projection(dict(Wt=np.ones((64, 1)), ct=np.zeros(1), U=np.ones((1, 1)), pmu=0.0, log_norm=0.0), device=0)
    assert call(p=other._p) == -1 and b"cf_marg.n is not" in lib.cf_last_error()
    other.close()
    assert lib.cf_marg_set_chunk(eng._h, 65537) == -1 and lib.cf_marg_set_chunk(eng._h, 0) == 0
    with pytest.warns(UserWarning, match="reads the slot 'offset'"):
        N.LinearNuisance(case.full, N.Templates.offset(eng.n_sn), slots=("offset",)).close()
    torch.cuda.synchronize()


def test_ensemble_on_the_marginalised_likelihood(pkg, N, small):
    ln = small.one
    W = 32
    start = _dev(pkg.synthetic.walkers(np.array([(66.0, 74.0), (0.2, 0.45), (-1.0, 1.0)]), W, seed=3))
    ens = pkg.ensemble.ShardedEnsemble(ln.torch_log_prob(), start, seed=11, moves=(("stretch", 1.0),))
    ens.run_mcmc(50)
    pos, logp = ens.full_state()
    pos, logp = pos.cpu().numpy(), logp.cpu().numpy()
    chain = ens.get_chain(flat=True).cpu().numpy()
    assert np.isfinite(chain).all() and np.isfinite(ens.get_log_prob(flat=True).cpu().numpy()).all()
    assert np.array_equal(_bits(ln.log_probability(pos)), _bits(logp))  # host pointers
    M = M_REF + ln.recover(pos, seed=2)[:, 0]  # the offset column restored
    assert np.isfinite(M).all() and (np.abs(M - M_REF) < 1.0).all()
