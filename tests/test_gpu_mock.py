"""GPU (-m gpu): the mock-data likelihood (csrc/cosmofit_mock.hip, cosmology-model-fit_amd/mocks.py).

Parity: engine A plus ``MockSet.from_shifts(d)`` against engines B_k built from the shifted data themselves, and against the
long-double restatement applied to ``engine.parts``' rows -- flat LCDM with the velocity step at n_sn around the pitch of the
residual rows, one joint shape (SN + BAO + CMB, physical E(z), thawing).  Bits against position / chunking / pointer kind / the
order of the set.  The special rows.  ``cf_mock_normals`` against the restatement.  End to end: the linear case against its
closed form and the chi^2(1) law, a Union3-shaped nonlinear case against ``optimize.best_fit`` on rebuilt engines.  The
``problem_index`` keyword of ``optimize.maximize``.

Measured on an MI355X (printed by the tests; profiles/NOTES_mock.md keeps the record): see the docstrings below."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import stats

import mock_reference as MR
import resid_shapes as RS
from conftest import golden
from test_mock_cpu import GEN_SEED, linear_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
BAR = 1e-10          # the project's parity bar, on the scale |chi2| + 2 sum |x_b| + c of the terms summed
N_MOCKS = 3
ROWS = (1, 4, 5, 257)
KINDS = (0, 1, 2)    # CF_OUT_CHI2, CF_OUT_LOGL, CF_OUT_LOGP


@pytest.fixture(scope="module")
def M(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.mocks


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


# ---- the shapes ------------------------------------------------------------------------------------------------------------
def _joint_data(pkg):
    """n_sn 65, 13 BAO data (the DESI set of the golden fixture without its last datum), Planck + ACT compression."""
    g = golden("bao_desi_cmb_des5y")
    syn = pkg.synthetic.pantheon_like(n_sn=65, seed=7, rank=40)
    inv = np.linalg.inv(g["bao_cov"][:13, :13])
    return dict(syn=syn, bao_z=g["bao_z"][:13], bao_val=g["bao_val"][:13], bao_qty=g["bao_qty"][:13], bao_inv=0.5 * (inv + inv.T),
                comp=dict(pkg.cmb_data.PLANCK_ACT))


def _joint_engine(pkg, jd, d_sn=0.0, d_bao=0.0, d_cmb=0.0):
    comp = dict(jd["comp"])
    comp["cmb_prior"] = np.asarray(comp["cmb_prior"], dtype=np.float64) + d_cmb
    s = jd["syn"]
    return pkg.likelihoods.DesiCmbDes5y(s["z_cmb"], s["z_hel"], s["obs"] + d_sn, None, jd["bao_z"], jd["bao_val"] + d_bao, jd["bao_qty"],
                                        jd["bao_inv"], chol=s["chol"], comp=comp, fde="thawing")


def _joint_thetas(pkg, S):
    box = np.array([(-19.5, -19.2), (64.0, 72.0), (0.0215, 0.0232), (0.112, 0.126), (-1.0, 1.0), (-0.99, -0.6)])
    return pkg.synthetic.walkers(box, S, seed=12)


class Case:
    """Engine A, the shifts of N_MOCKS mocks, the set, the engines B_k of the shifted data, 257 rows of theta -- built once per
    shape and shared; nothing of it is changed by a test."""

    def __init__(self, pkg, M, name):
        rng = np.random.default_rng(31)
        self.name, self.S = name, max(ROWS)
        if name == "joint":
            jd = _joint_data(pkg)
            self.lk = _joint_engine(pkg, jd)
            self.theta = _joint_thetas(pkg, self.S)
            sig = np.sqrt(np.diag(jd["syn"]["cov"]))
            self.d = dict(sn=rng.standard_normal((N_MOCKS, 65)) * sig,
                          bao=rng.standard_normal((N_MOCKS, 13)) * 0.02 * np.abs(jd["bao_val"]),
                          cmb=rng.standard_normal((N_MOCKS, 3)) * np.sqrt(np.diag(jd["comp"]["cmb_cov"])))
            self.others = [_joint_engine(pkg, jd, self.d["sn"][k], self.d["bao"][k], self.d["cmb"][k]) for k in range(N_MOCKS)]
            self.chol, self.bao_val, self.bao_inv = jd["syn"]["chol"], jd["bao_val"], jd["bao_inv"]
            self.cmb_prior, self.cmb_inv = np.asarray(jd["comp"]["cmb_prior"], float), np.asarray(jd["comp"]["cmb_inv_cov"], float)
        else:
            n = int(name)
            self.lk, syn = RS.sn_likelihood(pkg, n)
            self.theta = RS.sn_thetas(pkg, self.S)
            self.d = dict(sn=rng.standard_normal((N_MOCKS, n)) * np.sqrt(np.diag(syn["cov"])))
            self.others = [pkg.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"] + self.d["sn"][k], chol=syn["chol"])
                           for k in range(N_MOCKS)]
            self.chol = syn["chol"]
        self.engine = self.lk.engine
        self.set = M.MockSet.from_shifts(self.engine, **self.d)
        self.x = _dev(self.theta)
        self.mock = np.arange(self.S, dtype=np.int32) % N_MOCKS
        self.mk = _dev(self.mock)
        M.set_library_chunk(self.engine, 0)
        self.ref = {kind: tuple(t.cpu().numpy() for t in self.set.log_prob(self.x, self.mk, kind, cross=True)) for kind in KINDS}


_CASES = {}


@pytest.fixture(scope="module", params=[str(n) for n in RS.N_SN] + ["joint"])
def case(request, pkg, M):
    if request.param not in _CASES:
        _CASES[request.param] = Case(pkg, M, request.param)
    return _CASES[request.param]


# ---- 7: shifted-data parity --------------------------------------------------------------------------------------------------
def test_parity_with_engines_built_from_the_shifted_data(case, pkg, M):
    """Measured on an MI355X: largest |A + set - B_k| / (bar x scale) over every shape, kind and S: see profiles/NOTES_mock.md."""
    c, worst = case, 0.0
    M.set_library_chunk(c.engine, 96)
    try:
        for kind in KINDS:
            want = np.empty(c.S)
            for k in range(N_MOCKS):
                rows = np.nonzero(c.mock == k)[0]
                want[rows] = c.others[k].engine.torch_log_prob(kind)(c.x[_dev(rows)].contiguous()).cpu().numpy()
            chi2, cross = c.ref[0]
            scale = np.abs(chi2) + 2 * np.abs(cross).sum(axis=1) + c.set.c.cpu().numpy()[c.mock]
            for S in ROWS:
                got = c.set.log_prob(c.x[:S].contiguous(), c.mk[:S].contiguous(), kind).cpu().numpy()
                assert np.all(np.isfinite(got))
                f = 1.0 if kind == 0 else 0.5
                ratio = float(np.max(np.abs(got - want[:S]) / (f * BAR * scale[:S])))
                worst = max(worst, ratio)
    finally:
        M.set_library_chunk(c.engine, 0)
    print(f"{c.name}: largest |A + mock set - engine of the shifted data| / bar = {worst:.3g}")
    assert worst <= 1.0


def _restated(c, rows):
    """chi2_k of the rows in long double from ``engine.parts``' residual rows and the engine's own chi^2 of the observed data."""
    p = c.engine.parts(c.theta[rows])
    base = c.engine.chi_squared(c.theta[rows])
    Lf = np.tril(c.chol).astype(LD)
    gc = {}
    for k in range(N_MOCKS):
        g, cc = MR.g_and_c(Lf, c.d["sn"][k])
        gs, ctot = [g], cc
        if c.name == "joint":
            for A, d in ((c.bao_inv, c.d["bao"][k]), (c.cmb_inv, c.d["cmb"][k])):
                g, cc = MR.g_and_c_inv(A, d)
                gs.append(g)
                ctot = ctot + cc
        gc[k] = (gs, ctot)
    out, xs, scale, shift = [], [], [], []
    for j, s in enumerate(rows):
        r = [p["delta"][j]]
        if c.name == "joint":
            r += [c.bao_val - p["bao_theory"][j], c.cmb_prior - p["cmb_vector"][j]]
        gs, ctot = gc[int(c.mock[s])]
        v, x = MR.shifted(base[j], r, gs, ctot)
        out.append(float(v))
        xs.append([float(t) for t in x] + [0.0] * (3 - len(x)))
        scale.append(MR.scale(base[j], x, ctot))
        shift.append(v - LD(base[j]))
    return np.array(out), np.array(xs), np.array(scale), np.array(shift, dtype=LD)


def test_parity_with_the_long_double_restatement(case):
    c = case
    rows = np.arange(c.S)
    want, xs, scale, shift = _restated(c, rows)
    chi2, cross = c.ref[0]
    worst = float(np.max(np.abs(chi2[rows] - want) / (BAR * scale)))
    worst_x = float(np.max(np.abs(cross[rows] - xs) / (BAR * scale[:, None])))
    # the log-likelihood and log-posterior kinds: the engine's own value of the kind minus half the restated shift
    worst_l = 0.0
    for kind, base in ((1, c.engine.log_likelihood(c.theta[rows])), (2, c.engine.log_probability(c.theta[rows]))):
        want_l = (base.astype(LD) - shift / LD(2)).astype(np.float64)
        worst_l = max(worst_l, float(np.max(np.abs(c.ref[kind][0][rows] - want_l) / (0.5 * BAR * scale))))
        assert np.array_equal(_bits(c.ref[kind][1]), _bits(cross))  # the cross terms do not depend on the kind
    print(f"{c.name}: largest |device - restatement| / bar = {worst:.3g} (chi2), {worst_l:.3g} (log L, log P), {worst_x:.3g} (cross terms)")
    assert worst <= 1.0 and worst_x <= 1.0 and worst_l <= 1.0
    if c.name != "joint":
        assert np.all(cross[:, 1:] == 0.0)  # blocks not shifted


# ---- 8: bits -----------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_position_chunking_pointers_or_the_order_of_the_set(case, pkg, M):
    c = case
    L = pkg._lib
    for kind in (0, 2):
        ref, ref_x = c.ref[kind]
        for s in (0, 1, 95, 96, 256):
            one, one_x = c.set.log_prob(c.x[s:s + 1].contiguous(), c.mk[s:s + 1].contiguous(), kind, cross=True)
            assert np.array_equal(_bits(one.cpu().numpy()), _bits(ref[s:s + 1])), (kind, s)
            assert np.array_equal(_bits(one_x.cpu().numpy()), _bits(ref_x[s:s + 1]))
        try:
            for chunk in RS.CHUNKS:
                M.set_library_chunk(c.engine, chunk)
                got, got_x = c.set.log_prob(c.x, c.mk, kind, cross=True)
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref)), (kind, chunk)
                assert np.array_equal(_bits(got_x.cpu().numpy()), _bits(ref_x))
            # host pointers: the set's arrays, theta, the mock indices and the outputs in host memory
            M.set_library_chunk(c.engine, 96)
            host = {b: t.cpu().numpy() for b, t in c.set.g.items()}
            hc = c.set.c.cpu().numpy()
            hs = L.cf_mock_set()
            hs.struct_size, hs.n_mocks = C.sizeof(L.cf_mock_set), N_MOCKS
            for b, a in host.items():
                setattr(hs, "n_" + b, a.shape[1])
                setattr(hs, "g_" + b, a.ctypes.data)
            hs.c = hc.ctypes.data
            out, cross = np.empty(c.S), np.empty((c.S, 3))
            th = np.ascontiguousarray(c.theta)
            L.check(pkg.lib().cf_mock_eval(c.engine._h, C.byref(hs), th.ctypes.data, c.S, c.mock.ctypes.data, kind, out.ctypes.data,
                                           cross.ctypes.data))
            assert np.array_equal(_bits(out), _bits(ref)) and np.array_equal(_bits(cross), _bits(ref_x)), kind
        finally:
            M.set_library_chunk(c.engine, 0)
        # the set's rows permuted, the indices permuted to match
        perm = np.array([2, 0, 1])
        inv = np.argsort(perm)
        pset = M.MockSet(c.engine, {b: t[_dev(perm)].contiguous() for b, t in c.set.g.items()}, c.set.c[_dev(perm)].contiguous(), {})
        got = pset.log_prob(c.x, _dev(inv[c.mock].astype(np.int32)), kind).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ref)), kind


# ---- 9: special rows ---------------------------------------------------------------------------------------------------------
def test_host_pointers_beyond_one_piece_have_the_bits_of_the_device_path(pkg, M):
    """cf_mock_eval stages its rows through the device in pieces of 65536: 65537 rows of the smallest SN engine cross one
    boundary, so the second piece's row and mock index are read from behind the first's and its out / cross land behind them."""
    L, n, S = pkg._lib, RS.N_SN[0], 65537
    lk, syn = RS.sn_likelihood(pkg, n)
    try:
        d_sn = np.random.default_rng(32).standard_normal((N_MOCKS, n)) * np.sqrt(np.diag(syn["cov"]))
        mset = M.MockSet.from_shifts(lk.engine, sn=d_sn)
        theta = np.ascontiguousarray(RS.sn_thetas(pkg, S))
        mock = np.arange(S, dtype=np.int32) % N_MOCKS
        want, want_x = (t.cpu().numpy() for t in mset.log_prob(_dev(theta), _dev(mock), 0, cross=True))
        g, hc = mset.g["sn"].cpu().numpy(), mset.c.cpu().numpy()
        hs = L.cf_mock_set()
        hs.struct_size, hs.n_mocks, hs.n_sn, hs.g_sn, hs.c = C.sizeof(L.cf_mock_set), N_MOCKS, n, g.ctypes.data, hc.ctypes.data
        out, cross = np.full(S, np.nan), np.full((S, 3), np.nan)
        L.check(pkg.lib().cf_mock_eval(lk.engine._h, C.byref(hs), theta.ctypes.data, S, mock.ctypes.data, 0, out.ctypes.data,
                                       cross.ctypes.data))
        assert np.isfinite(out).all() and np.isfinite(cross).all()
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(cross), _bits(want_x))
    finally:
        lk.engine.close()


def test_special_rows(case, pkg):
    c = case
    S = 12
    th = c.theta[:S].copy()
    mock = (np.arange(S) % N_MOCKS).astype(np.int32)
    mock[[1, 6]] = -1          # the observed data
    mock[4] = N_MOCKS          # no such mock
    mock[9] = 2**31 - 1
    th[7, 1] = np.nan
    boxed = c.name != "joint"  # the SN mirror has sn/pantheon.py's prior box, the joint one has none
    if boxed:
        th[3, 2] = -0.01       # Omega_m below the box (E(z) stays real)
        th[10, 0] = -30.0      # M below the box
    x, mk = _dev(th), _dev(mock)
    for kind in KINDS:
        got, cross = (t.cpu().numpy() for t in c.set.log_prob(x, mk, kind, cross=True))
        base = c.engine.torch_log_prob(kind)(x).cpu().numpy()
        chi2, cr = (t.cpu().numpy() for t in c.set.log_prob(_dev(c.theta[:S]), _dev((np.arange(S) % N_MOCKS).astype(np.int32)), 0, cross=True))
        scale = np.abs(chi2) + 2 * np.abs(cr).sum(axis=1) + c.set.c.cpu().numpy().max()
        for s in (1, 6):       # k = -1: cf_eval_device's value (the accessor path against the production path)
            assert abs(got[s] - base[s]) <= BAR * scale[s], (kind, s)
            assert np.all(cross[s] == 0.0)
        assert np.isnan(got[4]) and np.isnan(got[9])
        assert (np.isnan(got[7]) and np.isnan(base[7])) or got[7] == base[7] == -np.inf  # what cf_eval_device gives for it
        if boxed and kind == 2:
            assert got[3] == -np.inf and got[10] == -np.inf
        ordinary = [s for s in range(S) if s not in (1, 3, 4, 6, 7, 9, 10)]
        assert np.all(np.isfinite(got[ordinary])), kind
        if kind == 0:          # NaN only where theta is NaN or the mock does not exist
            assert np.array_equal(np.nonzero(np.isnan(got))[0], [4, 7, 9])
        if c.name != "joint":
            assert np.all(cross[:, 1:] == 0.0)


def test_boxed_joint_engine_with_the_l_A_only_cmb_block(pkg, M):
    """bao/desi_des5y_bbn_theta_star.py's shape (SN + BAO + CMB mode 2, thawing, a prior box and a Gaussian prior): the set's
    g_cmb counts the l_A entry alone, as the handle does; rows outside the box stay -inf."""
    jd = _joint_data(pkg)
    s, rng = jd["syn"], np.random.default_rng(41)
    box = np.array([(-20.0, -19.0), (50.0, 90.0), (0.010, 0.030), (0.05, 0.30), (-1.0, -1 / 3)])

    def build(d_sn=0.0, d_bao=0.0, d_cmb=0.0):
        comp = dict(jd["comp"])
        comp["cmb_prior"] = np.asarray(comp["cmb_prior"], dtype=np.float64) + d_cmb
        return pkg.likelihoods.DesiDes5yBbnThetaStar(s["z_cmb"], s["z_hel"], s["obs"] + d_sn, None, jd["bao_z"], jd["bao_val"] + d_bao,
                                                     jd["bao_qty"], jd["bao_inv"], chol=s["chol"], comp=comp, bounds=box)

    d = dict(sn=rng.standard_normal((N_MOCKS, 65)) * np.sqrt(np.diag(s["cov"])),
             bao=rng.standard_normal((N_MOCKS, 13)) * 0.02 * np.abs(jd["bao_val"]),
             cmb=rng.standard_normal((N_MOCKS, 3)) * np.sqrt(np.diag(jd["comp"]["cmb_cov"])))
    lk = build()
    ms = M.MockSet.from_shifts(lk.engine, **d)
    assert np.all(ms.g["cmb"].cpu().numpy()[:, [0, 2]] == 0.0)
    S = 33
    theta = pkg.synthetic.walkers(np.array([(-19.5, -19.2), (64.0, 72.0), (0.0215, 0.0232), (0.112, 0.126), (-0.99, -0.6)]), S, seed=13)
    theta[4, 4] = -0.2        # w0 above the box
    theta[9, 1] = 95.0        # H0 above the box
    x, mock = _dev(theta), np.arange(S, dtype=np.int32) % N_MOCKS
    chi2, cross = (t.cpu().numpy() for t in ms.log_prob(x, _dev(mock), 0, cross=True))
    scale = np.abs(chi2) + 2 * np.abs(cross).sum(axis=1) + ms.c.cpu().numpy()[mock]
    assert np.all(cross[:, 0] != 0.0) and np.all(cross[:, 1] != 0.0) and np.all(cross[:, 2] != 0.0)
    worst = 0.0
    for k in range(N_MOCKS):
        other = build(d["sn"][k], d["bao"][k], d["cmb"][k])
        rows = np.nonzero(mock == k)[0]
        for kind in KINDS:
            got = ms.log_prob(x, _dev(mock), kind).cpu().numpy()[rows]
            want = other.engine.torch_log_prob(kind)(x[_dev(rows)].contiguous()).cpu().numpy()
            inside = np.isfinite(want)
            if kind == 2:
                assert np.array_equal(np.nonzero(~np.isfinite(got))[0], np.nonzero(~inside)[0])
                assert np.all(got[~inside] == -np.inf) and np.all(want[~inside] == -np.inf)
            else:
                assert np.all(inside) and np.all(np.isfinite(got))
            f = 1.0 if kind == 0 else 0.5
            worst = max(worst, float(np.max(np.abs(got[inside] - want[inside]) / (f * BAR * scale[rows][inside]))))
        other.engine.close()
    out = ms.log_prob(x, _dev(mock), 2).cpu().numpy()
    assert out[4] == -np.inf and out[9] == -np.inf and np.all(np.isfinite(np.delete(out, [4, 9])))
    print(f"mode 2 joint: largest |A + mock set - engine of the shifted data| / bar = {worst:.3g}")
    assert worst <= 1.0
    lk.engine.close()


# ---- 10: normals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n", [(1, 1), (1, 63), (1, 64), (5, 13), (17, 241)])
def test_normals_against_the_restatement(M, K, n):
    key = M.mock_key(GEN_SEED, "sn")
    got = M.normals(key, K, n).cpu().numpy()
    want = MR.normals(key, 0, K, n)
    err = float(np.max(np.abs(got.astype(LD) - want)))
    print(f"K n = {K * n}: largest |device - restatement| = {err:.3g} (bar 2e-14)")
    assert err <= 2e-14
    k1 = K // 2
    pieces = torch.cat([M.normals(key, k1, n), M.normals(key, K - k1, n, k0=k1)]).cpu().numpy()
    assert np.array_equal(_bits(pieces), _bits(got))
    later = M.normals(key, K, n, k0=1000).cpu().numpy()
    assert float(np.max(np.abs(later.astype(LD) - MR.normals(key, 1000, K, n)))) <= 2e-14


# ---- 11, 12: end to end --------------------------------------------------------------------------------------------------------
class Linear:
    """The linear case of tests/test_mock_cpu.py on the device: 64 SNe, only the offset free, K = 512 mocks drawn at theta_fid;
    the closed form of every mock from the set's own shifts, in long double."""
    K = 512
    FID = np.array([-19.35])
    BOX = np.array([(-20.0, -19.0)])

    def __init__(self, pkg, M):
        cov, _, _ = linear_case(K=1)
        syn = pkg.synthetic.pantheon_like(n_sn=64, seed=2, rank=8)
        self.syn, self.chol = syn, np.linalg.cholesky(cov)
        self.engine = self.build(pkg, syn["obs"])
        self.set = M.MockSet.draw(self.engine, self.FID, self.K, seed=GEN_SEED)
        self.r_fid = self.engine.parts(self.FID)["delta"][0]
        self.shift = self.set.shifts["sn"].cpu().numpy()
        # the mock data's residual at theta_fid: delta_k = d_k + r(theta_fid)
        self.closed, self.closed_min, _ = MR.linear_laws(np.tril(self.chol).astype(LD), self.shift.astype(LD) + self.r_fid.astype(LD))

    def build(self, pkg, obs):
        P = pkg.Param
        return pkg.LikelihoodEngine(ndim=1, z_max=float(self.syn["z_cmb"].max() + 0.1), params=dict(offset=P(0), H0=P(fixed=70.0), Om=P(fixed=0.3)),
                                    sn=dict(z_cmb=self.syn["z_cmb"], z_hel=self.syn["z_hel"], obs=obs, chol=self.chol), bounds=self.BOX)


@pytest.fixture(scope="module")
def linear(pkg, M):
    return Linear(pkg, M)


@pytest.fixture(scope="module")
def e2e_bar(pkg, linear):
    """Ten times the largest discrepancy ``optimize.best_fit`` shows against the closed form on three engines rebuilt with the
    shifted data, never above 1e-6 in chi^2."""
    worst = 0.0
    for k in (0, 1, 2):
        eng = linear.build(pkg, linear.syn["obs"] + linear.shift[k])
        f = eng.torch_log_prob(pkg.CF_OUT_LOGL)
        fit = pkg.optimize.best_fit(f, linear.BOX, n_starts=4, seed=0)
        delta = float(eng.chi_squared(linear.FID)) - fit.chi2
        worst = max(worst, abs(delta - float(linear.closed[k])), abs(fit.chi2 - float(linear.closed_min[k])))
        eng.close()
    bar = min(10.0 * worst, 1e-6)
    print(f"optimize.best_fit on three rebuilt engines against the closed form: largest discrepancy {worst:.3g}; bar = {bar:.3g}")
    return bar


def test_end_to_end_linear(linear, e2e_bar):
    """Measured on an MI355X: see profiles/NOTES_mock.md."""
    res = linear.set.delta_chi2({0: float(linear.FID[0])}, bounds=linear.BOX, n_starts=4, seed=0)
    d = res["delta_chi2"]
    err = float(np.max(np.abs(d.astype(LD) - linear.closed)))
    err_min = float(np.max(np.abs(res["chi2_full"].astype(LD) - linear.closed_min)))
    p = stats.kstest(d, "chi2", args=(1,)).pvalue
    print(f"K = {linear.K}: largest |Delta chi2 - closed form| = {err:.3g}, |chi2_min - closed form| = {err_min:.3g} (bar {e2e_bar:.3g}); "
          f"smallest Delta chi2 = {d.min():.3g}; KS against chi2(1): p = {p:.3g}; statuses {res['full'].status_counts}")
    assert err <= e2e_bar
    assert np.all(d >= -e2e_bar)
    assert p >= 0.01


def test_end_to_end_nonlinear(pkg, M, e2e_bar):
    """Union3-shaped: 22 bins, v fixed at 0 against free, K = 256 mocks of the v = 0 best fit, four starts each."""
    g = golden("sn_union3_1")
    box = pkg.likelihoods.SnUnion3.PRIOR_BOX
    mk = lambda obs: pkg.likelihoods.SnUnion3(g["z_cmb"], g["z_hel"], obs, g["cov"], H0=float(g["H0"]), bounds=box)
    lk = mk(g["obs"])
    null = pkg.optimize.best_fit(lk.engine.torch_log_prob(pkg.CF_OUT_LOGL), box, n_starts=8, seed=0, fixed={2: 0.0})
    ms = M.MockSet.draw(lk.engine, null.x, 256, seed=3)
    res = ms.delta_chi2({2: 0.0}, n_starts=4, seed=0)
    shift = ms.shifts["sn"].cpu().numpy()
    worst = 0.0
    for k in (0, 1, 2):
        other = mk(g["obs"] + shift[k])
        f = other.engine.torch_log_prob(pkg.CF_OUT_LOGL)
        full = pkg.optimize.best_fit(f, box, n_starts=32, seed=0)
        nested = pkg.optimize.best_fit(f, box, n_starts=32, seed=0, fixed={2: 0.0})
        worst = max(worst, abs(res["chi2_full"][k] - full.chi2), abs(res["chi2_nested"][k] - nested.chi2),
                    abs(res["delta_chi2"][k] - (nested.chi2 - full.chi2)))
        other.engine.close()
    counts = {**res["full"].status_counts}
    print(f"three mocks against optimize.best_fit on rebuilt engines: largest discrepancy {worst:.3g} (bar {e2e_bar:.3g}); "
          f"statuses full {res['full'].status_counts}, nested {res['nested'].status_counts}; mocks below -tol: {res['n_below']}; "
          f"median Delta chi2 {np.median(res['delta_chi2']):.3g}")
    assert worst <= e2e_bar
    assert counts["iteration_cap"] == 0 and res["nested"].status_counts["iteration_cap"] == 0
    lk.engine.close()


# ---- 13: problem_index -------------------------------------------------------------------------------------------------------
def test_problem_index(pkg):
    opt = pkg.optimize
    B, ndim, K = 64, 3, 4
    rng = np.random.default_rng(8)
    box = np.array([(-2.0, 2.0)] * ndim)
    t = _dev(rng.uniform(-1.5, 1.5, (B, ndim)))
    x0 = rng.uniform(-1.9, 1.9, (B, ndim))
    seen = []

    def f(theta, problem):
        seen.append(problem.cpu().numpy().copy())
        assert problem.dtype == torch.int32 and problem.device == theta.device and problem.shape == (theta.shape[0],)
        return -((theta - t[problem.long()]) ** 2).sum(dim=1)

    res = opt.maximize(f, box, x0, problem_index=True)
    assert np.all(res.converged)
    assert float(np.max(np.abs(res.x - t.cpu().numpy()))) < 1e-6      # each problem ends at its own t_p
    assert np.array_equal(seen[0], np.arange(B))
    assert len(seen) == res.n_calls and sum(s.size for s in seen) == res.n_like
    active = np.arange(B)
    for i in range(1, len(seen), 2):
        st, tr = seen[i], seen[i + 1]
        act = st[:: 2 * ndim]
        assert np.array_equal(st, np.repeat(act, 2 * ndim)) and np.array_equal(tr, np.repeat(act, K))
        assert np.all(np.diff(act) > 0) and np.all(np.isin(act, active))  # the active list, compacted in order
        active = act
    # the default path: the objective is called with theta alone and the result has the bits of the indexed run of the same problem
    t0 = t[:1]
    plain = opt.maximize(lambda th: -((th - t0) ** 2).sum(dim=1), box, x0)
    again = opt.maximize(lambda th, p: -((th - t0) ** 2).sum(dim=1), box, x0, problem_index=True)
    for name in ("x", "log_prob", "status", "n_iter", "grad_norm"):
        assert np.array_equal(getattr(plain, name), getattr(again, name)), name
    assert plain.n_like == again.n_like
