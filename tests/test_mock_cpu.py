"""CPU: everything of the mock-data ensembles that needs no device -- the identity chi2_k = chi2 + 2 r.g_k + c_k in long double
and through the reference-order oracle, the restated generator, the chi^2 laws the whole pipeline must reproduce (closed form
of the linear case), the layout of ``cf_mock_set``, the argument rules of ``cf_mock_eval_device`` (stated without a handle by
``cf_mock_check_args``) and the Monte-Carlo arithmetic of ``mocks.significance`` / ``goodness_of_fit``."""
import ctypes as C
import dataclasses
import importlib
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import stats

import mock_reference as MR
import test_oracle_golden as TG
from conftest import ROOT, golden, load_pkg, synthetic_cov
from oracle import oracle_np as onp

amd = load_pkg()
L = amd._lib
M = importlib.import_module("cosmology-model-fit_amd.mocks")
LD = np.longdouble

# the key of the generator tests: mocks.mock_key(GEN_SEED, "sn").  Fixed, so that the statistical bars below are checked on one
# known sample of the RESTATEMENT; the device is then held to the restatement's bits.
GEN_SEED = 1


def _spd(n, rng):
    """diag + low rank, the structure of the SN covariances."""
    A = 0.05 * rng.standard_normal((n, max(1, n // 8)))
    return np.diag(rng.uniform(0.5, 2.0, n) ** 2 * 0.01) + A @ A.T


# ---- 1: the identity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_identity_in_long_double(n):
    rng = np.random.default_rng(100 + n)
    Lf = MR.cholesky(_spd(n, rng))
    worst = 0.0
    for _ in range(3):
        r, d = rng.standard_normal(n) * 0.15, rng.standard_normal(n) * 0.15
        chi2 = MR.quad_form(Lf, r)
        g, c = MR.g_and_c(Lf, d)
        got, x = MR.shifted(chi2, [r], [g], c)
        want = MR.quad_form(Lf, r.astype(LD) + d.astype(LD))
        ratio = abs(float(got - want)) / (1e-15 * n * MR.scale(chi2, x, c))
        worst = max(worst, ratio)
    print(f"n = {n}: largest |restated - direct| / bar = {worst:.3g}")
    assert worst <= 1.0


# ---- 2: the identity through the reference-order oracle ----------------------------------------------------------------------
def _oracle_rows(lk, th):
    """The oracle's residual rows (sn, bao, cmb) and block chi^2 at th."""
    rows = {}
    if lk.z_cmb is not None:
        rows["sn"] = onp.sn_parts(lk, th)[-1]
    if lk.bao_z is not None:
        rows["bao"] = lk.bao_val - onp.bao_theory(lk, th)
    if lk.cmb_mode:
        rows["cmb"] = lk.cmb_prior - onp.cmb_distances(lk, th)
    return rows


def _oracle_identity(lk, thetas, rng):
    Lf = np.tril(lk.chol).astype(LD)
    worst = 0.0
    for th in thetas:
        rows = _oracle_rows(lk, th)
        d = {b: rng.standard_normal(r.size) * 0.5 * (np.abs(r).mean() + 1e-3) for b, r in rows.items()}
        gs, c = {}, LD(0)
        for b in rows:
            g, cb = MR.g_and_c(Lf, d[b]) if b == "sn" else MR.g_and_c_inv(lk.bao_inv_cov if b == "bao" else lk.cmb_inv_cov, d[b])
            gs[b], c = g, c + cb
        chi2 = onp.chi_squared(lk, th)
        got, x = MR.shifted(chi2, [rows[b] for b in rows], [gs[b] for b in rows], c)
        moved = dataclasses.replace(lk, obs=lk.obs + d["sn"], **({"bao_val": lk.bao_val + d["bao"]} if "bao" in d else {}),
                                    **({"cmb_prior": lk.cmb_prior + d["cmb"]} if "cmb" in d else {}))
        want = onp.chi_squared(moved, th)
        worst = max(worst, abs(float(got) - want) / (1e-12 * MR.scale(chi2, x, c)))
    return worst


def test_identity_through_the_oracle_sn():
    g = golden("sn_union3_1")
    worst = _oracle_identity(TG.lk_sn_union3_1(g), g["thetas"][:4], np.random.default_rng(5))
    print(f"sn_union3_1: largest |restated - oracle on shifted data| / bar = {worst:.3g}")
    assert worst <= 1.0


def test_identity_through_the_oracle_joint():
    g = golden("bao_desi_cmb_des5y")
    lk = TG.lk_bao_desi_cmb_des5y(g, TG._chol_of(g))
    worst = _oracle_identity(lk, g["thetas"][:2], np.random.default_rng(6))
    print(f"bao_desi_cmb_des5y (SN + BAO + CMB): largest |restated - oracle on shifted data| / bar = {worst:.3g}")
    assert worst <= 1.0


# ---- 3: the generator -----------------------------------------------------------------------------------------------------------
def test_generator_value_depends_on_key_mock_and_index_only():
    key = M.mock_key(GEN_SEED, "sn")
    whole = MR.normals(key, 0, 37, 65)
    pieces = np.concatenate([MR.normals(key, 0, 5, 65), MR.normals(key, 5, 1, 65), MR.normals(key, 6, 31, 65)])
    assert np.array_equal(whole, pieces)
    assert whole[3, 7] == MR.normals(key, 3, 1, 65)[0, 7]
    assert not np.array_equal(whole, MR.normals(M.mock_key(GEN_SEED, "bao"), 0, 37, 65))
    assert len({M.mock_key(s, b) for s in range(4) for b in M.BLOCKS}) == 12
    with pytest.raises(ValueError):
        M.mock_key(0, "cc")


def test_generator_is_standard_normal():
    z = MR.normals(M.mock_key(GEN_SEED, "sn"), 0, 2000, 64).astype(np.float64)
    p = stats.kstest(z.reshape(-1), "norm").pvalue
    mean, n = float(z.mean()), z.size
    corr = float(np.corrcoef(z[:, :-1].reshape(-1), z[:, 1:].reshape(-1))[0, 1])
    print(f"KS p = {p:.3g}, mean = {mean:.3g} (4 / sqrt n = {4 / np.sqrt(n):.3g}), adjacent-column correlation = {corr:.3g}")
    assert p >= 0.01 and abs(mean) <= 4 / np.sqrt(n) and abs(corr) < 0.1
    assert abs(float(z.std()) - 1.0) < 4 / np.sqrt(2 * n)


# ---- 4: the laws, in closed form --------------------------------------------------------------------------------------------
def linear_case(K=2000, n=64, seed=GEN_SEED):
    """The linear case shared with the GPU test: C = diag + low rank, the noise delta_k = L n_k from the restated generator."""
    sigma = np.random.default_rng(11).uniform(0.08, 0.25, n)
    cov = synthetic_cov(sigma, seed=3, rank=8, amp=0.03)
    Lf = MR.cholesky(cov)
    z = MR.normals(M.mock_key(seed, "sn"), 0, K, n)
    return cov, Lf, z @ Lf.T


def test_closed_form_laws_of_the_linear_case():
    _, Lf, delta = linear_case()
    d, cmin, _ = MR.linear_laws(Lf, delta)
    p1 = stats.kstest(d.astype(np.float64), "chi2", args=(1,)).pvalue
    p63 = stats.kstest(cmin.astype(np.float64), "chi2", args=(63,)).pvalue
    print(f"KS of Delta chi2 against chi2(1): p = {p1:.3g}; of chi2_min against chi2(63): p = {p63:.3g}")
    assert p1 >= 0.01 and p63 >= 0.01


# ---- 5: the C side ------------------------------------------------------------------------------------------------------------
def test_mock_set_layout_matches_c(tmp_path):
    fields = [name for name, _ in L.cf_mock_set._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "cosmofit.h"\nint main(){printf("%zu %d", sizeof(cf_mock_set), ' \
           'CF_MOCK_CHUNK);' + "".join(f'printf(" %zu", offsetof(cf_mock_set, {f}));' for f in fields) + "return 0;}"
    src, exe = tmp_path / "mock.c", tmp_path / "mock"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals[:2] == [C.sizeof(L.cf_mock_set), L.CF_MOCK_CHUNK]
    for f, off in zip(fields, vals[2:]):
        assert getattr(L.cf_mock_set, f).offset == off, f


def _set(n_mocks=3, n_sn=100, n_bao=0, n_cmb=0, g_sn=1, g_bao=1, g_cmb=1, c=1, size=None):
    s = L.cf_mock_set()
    s.struct_size = C.sizeof(L.cf_mock_set) if size is None else size
    s.n_mocks, s.n_sn, s.n_bao, s.n_cmb = n_mocks, n_sn, n_bao, n_cmb
    s.g_sn, s.g_bao, s.g_cmb, s.c = g_sn or None, g_bao or None, g_cmb or None, c or None  # never dereferenced by the check
    return s


def _check(s=None, n_sn=100, n_bao=13, cmb=1, quasar=0, n_devices=1, theta=1, S=5, mock=1, kind=0, out=1, null_set=False):
    s = _set() if s is None else s
    return amd.lib().cf_mock_check_args(n_sn, n_bao, cmb, quasar, n_devices, None if null_set else C.byref(s), theta or None, S,
                                        mock or None, kind, out or None)


def test_argument_errors_are_reported_before_any_device_work():
    lib = amd.lib()
    inv, uns = -1, -5
    assert _check() == 0
    assert _check(_set(n_sn=100, n_bao=13, n_cmb=3)) == 0
    assert _check(_set(n_sn=0, n_bao=13, g_sn=0)) == 0       # an unshifted block needs no array
    assert _check(quasar=1) == uns and b"quasar" in lib.cf_last_error()
    assert _check(n_devices=2) == uns and b"several devices" in lib.cf_last_error()
    assert _check(null_set=True) == inv
    assert _check(_set(size=8)) == inv and b"struct_size" in lib.cf_last_error()
    assert _check(_set(n_mocks=0)) == inv and b"n_mocks" in lib.cf_last_error()
    assert _check(n_sn=0) == inv and b"no SN block" in lib.cf_last_error()
    assert _check(_set(n_bao=13), n_bao=0) == inv and b"no BAO block" in lib.cf_last_error()
    assert _check(_set(n_cmb=3), cmb=0) == inv and b"no CMB block" in lib.cf_last_error()
    assert _check(_set(n_sn=99)) == inv and _check(_set(n_bao=12)) == inv and _check(_set(n_cmb=2)) == inv
    assert _check(_set(n_sn=-100)) == inv
    assert _check(_set(g_sn=0)) == inv and b"null array" in lib.cf_last_error()
    assert _check(_set(n_bao=13, g_bao=0)) == inv and _check(_set(n_cmb=3, g_cmb=0)) == inv and _check(_set(c=0)) == inv
    assert _check(_set(n_sn=0)) == inv and b"no shifted block" in lib.cf_last_error()
    assert _check(kind=3) == inv and _check(kind=-1) == inv
    assert _check(S=-1) == inv and _check(S=2**31) == inv and _check(S=2**31 - 1) == 0
    assert _check(theta=0) == inv and _check(mock=0) == inv and _check(out=0) == inv
    assert _check(theta=0, mock=0, out=0, S=0) == 0            # no rows: a no-op, nothing is read
    assert lib.cf_mock_set_chunk(None, 96) == inv
    assert lib.cf_mock_normals(1, 0, 0, 5, None, None) == 0    # no mocks: a no-op
    assert lib.cf_mock_normals(1, -1, 1, 5, 1, None) == inv and lib.cf_mock_normals(1, 0, 1, 0, 1, None) == inv
    assert lib.cf_mock_normals(1, 0, 1, 5, None, None) == inv and lib.cf_mock_normals(1, 2**61, 2**61, 5, 1, None) == inv


def test_exports_cover_the_new_symbols():
    for name in ("cf_mock_eval_device", "cf_mock_eval", "cf_mock_check_args", "cf_mock_set_chunk", "cf_mock_normals"):
        assert name in L.EXPORTS and hasattr(amd.lib(), name)


# ---- 6: the Python arithmetic ---------------------------------------------------------------------------------------------------
def test_significance_arithmetic():
    null = np.concatenate([np.zeros(990), np.full(10, 9.0)])
    s = M.significance(6.61, null, k=1)
    assert s["n_mocks"] == 1000 and s["n_exceed"] == 10 and s["p"] == 11 / 1001
    lo, hi = s["p_interval"]
    assert lo < 10 / 1000 < hi
    a = 0.5 * (1 - s["level"])
    assert stats.binom.sf(9, 1000, lo) == pytest.approx(a, rel=1e-9)       # P(X >= 10 | lo) = a: the exact interval
    assert stats.binom.cdf(10, 1000, hi) == pytest.approx(a, rel=1e-9)
    assert s["sigma"] == pytest.approx(stats.norm.isf(0.5 * 11 / 1001), rel=1e-14)
    assert s["sigma_interval"][0] < s["sigma"] < s["sigma_interval"][1]
    assert s["wilks_sigma"] == amd.optimize.sigma_from_delta_chi2(6.61, 1) == np.sqrt(6.61)
    # the sigma conversion is the one of sigma_from_delta_chi2, at the same p
    for d, k in ((6.61, 1), (11.7, 1), (6.61, 2), (20.0, 3)):
        assert M.sigma_of_p(stats.chi2.sf(d, k)) == pytest.approx(amd.optimize.sigma_from_delta_chi2(d, k), rel=1e-12)
    none = M.significance(100.0, null)
    assert none["p"] == 1 / 1001 and none["p_interval"][0] == 0.0 and none["sigma_interval"][1] == np.inf
    every = M.significance(-1.0, null)
    assert every["p"] == 1.0 and every["p_interval"][1] == 1.0 and every["sigma"] == 0.0
    for bad in (([], 1.0), ([1.0, np.nan], 1.0), ([1.0], np.inf)):
        with pytest.raises(ValueError):
            M.significance(bad[1], bad[0])


def test_goodness_of_fit_arithmetic():
    mock = stats.chi2.ppf((np.arange(999) + 0.5) / 999, 19)
    gof = M.goodness_of_fit(22.15, mock, dof=19)
    x = int(np.sum(mock >= 22.15))
    assert gof["n_exceed"] == x and gof["p"] == (1 + x) / 1000
    assert gof["wilks_p"] == pytest.approx(stats.chi2.sf(22.15, 19), rel=1e-14)
    assert abs(gof["p"] - gof["wilks_p"]) < 2e-3                           # chi^2(19) mocks: the two agree
    assert gof["wilks_sigma"] == pytest.approx(M.sigma_of_p(gof["wilks_p"]))
    assert "wilks_p" not in M.goodness_of_fit(22.15, mock)
    with pytest.raises(ValueError):
        M.goodness_of_fit(22.15, mock, dof=0)


def _stub(unshiftable=(), quasar=False, multi=False):
    return SimpleNamespace(model_info=dict(quasar=quasar, multi_device=multi), n_sn=22, n_bao=0, ndim=3, bounds=None,
                           mock_data=dict(sn_chol=np.eye(22), bao_val=None, bao_inv_cov=None, cmb_prior=None, cmb_inv_cov=None,
                                          cmb_mode=0, unshiftable=list(unshiftable)))


def test_draw_refuses_what_it_cannot_shift():
    for blocks in (("cc",), ("fs8",), ("chi2_gauss",), ("cc", "fs8")):
        with pytest.raises(ValueError, match="cannot shift"):
            M.MockSet.draw(_stub(blocks), np.zeros(3), 4)
        M._check_unshiftable(_stub(blocks).mock_data, blocks)              # named in keep_observed: accepted
    with pytest.raises(ValueError, match="cannot shift"):
        M.MockSet.draw(_stub(("cc", "fs8")), np.zeros(3), 4, keep_observed=("cc",))
    with pytest.raises(ValueError, match="quasar"):
        M.MockSet.draw(_stub(quasar=True), np.zeros(3), 4)
    with pytest.raises(ValueError, match="several devices"):
        M.MockSet.from_shifts(_stub(multi=True), sn=np.zeros((2, 22)))
    with pytest.raises(ValueError, match="LikelihoodEngine"):
        M.MockSet.draw(object(), np.zeros(3), 4)
    with pytest.raises(ValueError, match="no BAO block"):
        M.MockSet.draw(_stub(), np.zeros(3), 4, blocks=("bao",))
    with pytest.raises(ValueError, match="n_mocks"):
        M.MockSet.draw(_stub(), np.zeros(3), 0)
    with pytest.raises(ValueError, match="at least one block"):
        M.MockSet.from_shifts(_stub())


def test_noise_factor_drops_the_components_without_information():
    A = np.zeros((4, 4))
    A[np.ix_([0, 2], [0, 2])] = np.linalg.inv(np.array([[4.0, 1.0], [1.0, 9.0]]))
    act, Lf = M.noise_factor(A)
    assert act.tolist() == [0, 2]
    np.testing.assert_allclose(Lf @ Lf.T, [[4.0, 1.0], [1.0, 9.0]], rtol=1e-13)
    md = dict(cmb_inv_cov=np.arange(1.0, 10.0).reshape(3, 3), cmb_mode=2)
    assert np.array_equal(M._sym_inverse(md, "cmb"), np.diag([0.0, 5.0, 0.0]))  # l_A alone
    md["cmb_mode"] = 1
    assert np.array_equal(M._sym_inverse(md, "cmb"), 0.5 * (md["cmb_inv_cov"] + md["cmb_inv_cov"].T))
