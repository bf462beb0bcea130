"""CPU: everything of the leave-group-out fits that needs no device -- the long-double restatement against the brute-force
deleted problem, the host half of ``cf_group_create``, the argument rules (``cf_group_check_args``, ``cf_group_quad_check_args``,
``cf_reweight_check_args``) and the keyword checks of ``leaveout``, the reweighting arithmetic against a Gaussian closed form,
and the tail index on exact generalized-Pareto draws."""
import ctypes as C
import importlib
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import infl_reference as IR
import infl_shapes as IS
import leaveout_reference as LR
import leaveout_shapes as LS
from conftest import ROOT, load_pkg

amd = load_pkg()
L = amd._lib
LO = importlib.import_module("cosmology-model-fit_amd.leaveout")
INV = -1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the restatement against brute force ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hard():
    cov = IS.covariance(amd, IS.N_HARD)
    chol = np.linalg.cholesky(cov)
    r = IS.residual_rows(chol, 1, seed=4)[0]
    K, _ = IR.precision(chol)
    g = IR.g_rows(chol, r[None, :])[0]
    return SimpleNamespace(cov=chol @ chol.T, chol=chol, r=r, K=K, g=g, chi2=float(np.asarray(r, dtype=IR.LD) @ g))


@pytest.mark.parametrize("m", LS.M_BRUTE)
def test_restatement_equals_the_deleted_problem(hard, m):
    """chi^2 - q_B is the chi^2 of the data without B solved from C_AA, and e_B = K_BB^-1 g_B is the group minus its conditional
    mean, on ``hard_cov`` at n = 257: bar 1e-10 relative (measured here: below 1e-13 for every size)."""
    idx = LS.shuffled_group(IS.N_HARD, m, seed=m)
    q, _, e = LR.group_q(hard.K, hard.g[None, :], idx)
    e_ref, chi2_sub = LR.deleted_group(hard.cov, hard.r, idx)
    rel_chi = abs(float((hard.chi2 - q[0]) / chi2_sub - 1))
    rel_e = float(np.max(np.abs(e[0] - e_ref)) / np.max(np.abs(e_ref)))
    print("m = %d: chi2 - q_B against the deleted problem %.2e relative, e_B against the conditional mean %.2e" % (m, rel_chi, rel_e))
    assert q[0] >= 0 and rel_chi <= 1e-10 and rel_e <= 1e-10


# ---- the host half of cf_group_create -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", LS.M_HOST)
def test_host_inverse_factor_is_rounded_once(m):
    """X_B entrywise against the long-double inverse factor of the same double K_BB, within 4 eps of (|X| |L| |X|)_ij: a shuffled
    index order, and NaN in the strict upper triangle of K, which is never read."""
    n = IS.N_HARD
    K = IS.host_precision(L, amd.lib(), np.linalg.cholesky(IS.covariance(amd, n)))[0]
    idx = LS.shuffled_group(n, m, seed=40 + m)
    dirty = np.ascontiguousarray(np.tril(K) + np.triu(np.full((n, n), np.nan), 1))
    X = np.full((m, m), np.nan)
    L.check(amd.lib().cf_selftest_group_host(_p(dirty), n, n, m, _p(idx), _p(X)))
    want, bound = LR.inverse_factor(K, idx)
    low = np.tril_indices(m)
    err = np.asarray(np.abs(X - want)[low] / bound[low], dtype=np.float64)
    print("m = %d: X_B against the long-double restatement, largest error %.2f eps of (|X| |L| |X|)_ij" % (m, err.max() / IR.EPS))
    assert err.max() <= 4 * IR.EPS
    assert not np.triu(X, 1).any() and (np.diag(X) > 0).all()


def test_host_half_names_a_non_positive_pivot():
    K = np.eye(6)
    K[4, 4] = 0.0
    idx = np.array([5, 4, 0], dtype=np.int32)
    X = np.zeros((3, 3))
    lib = amd.lib()
    assert lib.cf_selftest_group_host(_p(K), 6, 6, 3, _p(idx), _p(X)) == INV
    assert b"group 0: non-positive pivot at column 1" in lib.cf_last_error()
    K[4, 4], K[4, 0] = 1.0, 2.0   # K_BB = [[1, 0, 0], [0, 1, 2], [0, 2, 1]] in the order (5, 4, 0): indefinite
    assert lib.cf_selftest_group_host(_p(K), 6, 6, 3, _p(idx), _p(X)) == INV and b"column 2" in lib.cf_last_error()
    assert lib.cf_selftest_group_host(None, 6, 6, 3, _p(idx), _p(X)) == INV
    assert lib.cf_selftest_group_host(_p(K), 6, 5, 3, _p(idx), _p(X)) == INV and b"ld < n" in lib.cf_last_error()


# ---- argument rules ---------------------------------------------------------------------------------------------------------------
def _check(n, groups, kdiag=None):
    off, idx = LO.pack_groups(groups)
    kd = None if kdiag is None else _p(np.ascontiguousarray(kdiag, dtype=np.float64))
    lib = amd.lib()
    return lib.cf_group_check_args(n, kd, len(off) - 1, _p(off), _p(idx)), lib.cf_last_error()


def test_group_argument_rules_name_the_group():
    assert _check(10, [[0, 1], [9]])[0] == 0
    assert _check(10, [[3, 1, 2], [1, 2], [2]])[0] == 0                     # overlapping, unordered groups are fine
    rc, msg = _check(10, [[0], [1, 10]])
    assert rc == INV and b"group 1 has an index outside" in msg
    rc, msg = _check(10, [[0], [1, -1]])
    assert rc == INV and b"group 1" in msg
    rc, msg = _check(10, [[0, 4], [1], [2, 5, 2]])
    assert rc == INV and b"group 2 names datum 2 twice" in msg
    rc, msg = _check(2000, [[0], list(range(1025))])
    assert rc == INV and b"group 1 holds more than 1024 data" in msg
    assert _check(2000, [list(range(1024))])[0] == 0
    rc, msg = _check(2000, [[k] for k in range(1025)])
    assert rc == INV and b"n_groups must be in 1..1024" in msg
    rc, msg = _check(2000, [list(range(1024))] * 33)                        # 33 x 8 MiB of factors
    assert rc == INV and b"exceed 256 MB" in msg and b"group 32" in msg
    assert _check(2000, [list(range(1024))] * 32)[0] == 0
    kd = np.ones(10)
    kd[7] = 0.0
    rc, msg = _check(10, [[0, 1], [6, 7]], kd)
    assert rc == INV and b"group 1 holds datum 7, which the likelihood ignores" in msg
    assert _check(10, [[0, 1], [6, 8]], kd)[0] == 0
    lib = amd.lib()
    off, idx = np.array([0, 0], dtype=np.int64), np.array([0], dtype=np.int32)
    assert lib.cf_group_check_args(10, None, 1, _p(off), _p(idx)) == INV and b"group 0 is empty" in lib.cf_last_error()
    off = np.array([1, 2], dtype=np.int64)
    assert lib.cf_group_check_args(10, None, 1, _p(off), _p(idx)) == INV and b"offsets[0]" in lib.cf_last_error()
    assert lib.cf_group_check_args(10, None, 1, None, _p(idx)) == INV
    assert lib.cf_group_check_args(0, None, 1, _p(off), _p(idx)) == INV
    p = C.c_void_p()
    assert lib.cf_group_create(None, 1, _p(off), _p(idx), C.byref(p)) == INV and b"null cf_prec" in lib.cf_last_error()
    assert lib.cf_group_info(None, None, None, None) == INV
    assert lib.cf_group_quad_device(None, None, 4, 1, None, 1, None) == INV
    lib.cf_group_destroy(None)


def test_quad_and_reweight_argument_rules():
    lib = amd.lib()
    buf = np.zeros(64)
    b = _p(buf)
    assert lib.cf_group_quad_check_args(10, 3, b, 10, 4, b, 3) == 0
    assert lib.cf_group_quad_check_args(10, 3, None, 10, 0, None, 3) == 0
    assert lib.cf_group_quad_check_args(10, 3, b, 9, 4, b, 3) == INV and b"g_pitch below n" in lib.cf_last_error()
    assert lib.cf_group_quad_check_args(10, 3, b, 10, 4, b, 2) == INV and b"q_pitch" in lib.cf_last_error()
    assert lib.cf_group_quad_check_args(10, 3, b, 10, -1, b, 3) == INV
    assert lib.cf_group_quad_check_args(10, 3, None, 10, 4, b, 3) == INV and lib.cf_group_quad_check_args(10, 3, b, 10, 4, None, 3) == INV
    piv = np.zeros(16)
    ok = lambda **k: lib.cf_reweight_check_args(*[{**dict(lw=b, lp=3, S=8, G=3, x=b, xp=4, nc=4, pv=_p(piv), out=b), **k}[n]
                                                  for n in ("lw", "lp", "S", "G", "x", "xp", "nc", "pv", "out")])
    assert ok() == 0
    for bad in (dict(lw=None), dict(x=None), dict(pv=None), dict(out=None), dict(S=0), dict(S=2**31 + 1), dict(G=0), dict(G=4097),
                dict(nc=0), dict(nc=17, xp=17), dict(lp=2), dict(xp=3)):
        assert ok(**bad) == INV, bad
    piv[2] = np.nan
    assert ok() == INV and b"pivot must be finite" in lib.cf_last_error()
    piv[2] = 0.0
    assert ok(S=2**31, G=4096, lp=4096) == INV and b"exceed 1 GiB" in lib.cf_last_error()
    # with nothing valid to launch, the device entry refuses the same way without touching a device
    assert lib.cf_reweight_device(None, 3, 8, 3, None, b, 4, 4, _p(piv), b, None) == INV


def test_record_layout_matches_the_header(tmp_path):
    prog = ('#include <stdio.h>\n#include "cosmofit.h"\nint main(){printf("%d %d %d %d %d %d %d", CF_RW_NCOL(1), CF_RW_NCOL(6), '
            'CF_RW_NCOL(16), CF_RW_MEAN, CF_RW_SLICE, CF_RW_MAX_NCOL, CF_RW_MAX_G);return 0;}')
    (tmp_path / "rw.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "rw.c"), "-o", str(tmp_path / "rw")], check=True)
    vals = list(map(int, subprocess.run([str(tmp_path / "rw")], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [L.rw_ncol(1), L.rw_ncol(6), L.rw_ncol(16), L.CF_RW_MEAN, L.CF_RW_SLICE, L.CF_RW_MAX_NCOL, L.CF_RW_MAX_G]
    assert len(L.RW_SLOTS) == L.CF_RW_MEAN and L.RW_SLOTS == LR.RW_SLOTS and L.CF_RW_MEAN == LR.RW_MEAN


def test_python_layer_checks_before_any_device_call():
    eng = SimpleNamespace(model_info=dict(quasar=False, multi_device=False), n_sn=10, n_bao=0, ndim=3)
    t = torch.zeros((5, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="block must be one of"):
        LO.Groups(eng, [[0]], "cc")
    with pytest.raises(ValueError, match="no BAO block"):
        LO.group_chi2(eng, t, [[0]], "bao")
    with pytest.raises(ValueError, match="quasar"):
        LO.Groups(SimpleNamespace(model_info=dict(quasar=True, multi_device=False)), [[0]])
    with pytest.raises(ValueError, match="several devices"):
        LO.Groups(SimpleNamespace(model_info=dict(quasar=False, multi_device=True)), [[0]])
    with pytest.raises(amd.CosmofitError, match="group 1 has an index outside"):
        LO.Groups(eng, [[0], [10]])
    with pytest.raises(amd.CosmofitError, match="twice"):
        LO.group_chi2(eng, t, [[1, 1]])
    with pytest.raises(ValueError, match="non-empty list of integer"):
        LO.Groups(eng, [[0], []])
    with pytest.raises(ValueError, match="non-empty list of integer"):
        LO.Groups(eng, [[0.5]])
    with pytest.raises(ValueError, match="one per group"):
        LO.Groups(eng, [[0], [1]], names=["a"])
    with pytest.raises(ValueError, match="piece"):
        LO.group_chi2(eng, t, [[0]], piece=0)
    with pytest.raises(ValueError, match="there is no CPU implementation"):
        LO.leave_group_out(eng, t, [[0]])                         # a host tensor: refused, never computed on the host
    with pytest.raises(ValueError, match="float64 tensor"):
        LO.leave_group_out(eng, np.zeros((5, 3)), [[0]])
    with pytest.raises(TypeError, match="unexpected keyword.*thresholds"):
        LO.chain_leave_group_out(eng, t, groups=[[0]], thresholds=(1,))
    with pytest.raises(TypeError, match="needs groups="):
        LO.chain_leave_group_out(eng, t, block="sn")
    # reweight
    lw, x = torch.zeros(5, dtype=torch.float64), torch.zeros((5, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="there is no CPU implementation"):
        LO.reweight(lw, x)
    with pytest.raises(ValueError, match="there is no CPU implementation"):
        LO.reweight(lw.numpy(), x)
    with pytest.raises(ValueError, match="float64"):
        LO.reweight(lw.float(), x)
    with pytest.raises(ValueError, match="one row per sample"):
        LO.reweight(lw[:4], x)
    with pytest.raises(ValueError, match="at most 16 columns of x"):
        LO.reweight(lw, torch.zeros((5, 17), dtype=torch.float64))
    with pytest.raises(ValueError, match="one per column"):
        LO.reweight(lw, x, names=["a", "b"])
    with pytest.raises(ValueError, match=r"base_weights must be \[S\]"):
        LO.reweight(lw, x, base_weights=torch.ones(4, dtype=torch.float64))
    for cls, name in ((amd.ensemble.ShardedEnsemble, "leave_group_out"), (amd.nested.DeviceNestedSampler, "leave_group_out")):
        assert callable(getattr(cls, name))


def test_groups_from_labels_and_edges():
    groups, names = LO.groups_from_labels(["b", "a", "b", "c", "a"])
    assert names == ["b", "a", "c"] and [g.tolist() for g in groups] == [[0, 2], [1, 4], [3]]
    z = np.array([0.01, 0.5, 0.2, 1.0, 0.7, 2.0])
    groups, names = LO.groups_from_edges(z, [0.0, 0.3, 0.6, 0.65, 1.0])
    assert [g.tolist() for g in groups] == [[0, 2], [1], [3, 4]]           # the empty bin is dropped, the last edge is closed
    assert names == ["z[0,0.3)", "z[0.3,0.6)", "z[0.65,1]"]
    with pytest.raises(ValueError):
        LO.groups_from_edges(z, [0.3, 0.2])
    with pytest.raises(ValueError):
        LO.groups_from_edges(z, [3.0, 4.0])


# ---- the reweighting arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,s2", LS.GAUSS_CASES)
def test_reweight_arithmetic_against_the_gaussian_closed_form(d, s2):
    """Base N(0, 1), target N(d, s2): the ESS fraction, the evidence ratio (1: both are normalised), mean and variance of the
    restatement's record through ``summary_from_record`` at S = 2e5, each within 5 standard errors of its sample estimate (the
    ESS fraction's from the weights' own fourth moment by the delta method)."""
    S = 200000
    x = np.random.default_rng(11).standard_normal(S)
    lw = LR.gaussian_log_weight(x, d, s2)
    pivot = np.array([x.mean()])
    rec, _ = LR.reweight_record(lw, None, x[:, None], pivot)
    out = LO.summary_from_record(np.asarray(rec, dtype=np.float64), pivot)
    w = np.exp(lw)
    m1, m2 = w.mean(), (w * w).mean()
    inv_frac = m2 / m1**2
    se = np.std(w * w / m1**2 - 2.0 * m2 * w / m1**3) / np.sqrt(S)       # delta method on mean(w^2) / mean(w)^2
    want = LR.gaussian_inverse_ess_fraction(d, s2)
    print("d = %g, s2 = %g: ESS fraction %.4f against %.4f (1 / fraction off by %.2f standard errors)"
          % (d, s2, out["ess_fraction"][0], 1.0 / want, abs(inv_frac - want) / se))
    assert abs(1.0 / out["ess_fraction"][0] - want) <= 5 * se
    assert out["ess_fraction"][0] == pytest.approx(1.0 / inv_frac, rel=1e-12) and out["ess"][0] == pytest.approx(S / inv_frac, rel=1e-12)
    assert abs(np.exp(out["log_mean_weight"][0]) - 1.0) <= 5 * np.std(w) / np.sqrt(S)
    wn = w / w.sum()
    assert abs(out["mean"][0, 0] - d) <= 5 * np.sqrt((wn**2 * (x - d)**2).sum())
    assert abs(out["cov"][0, 0, 0] - s2) <= 5 * np.sqrt((wn**2 * ((x - d)**2 - s2)**2).sum())
    assert out["n_used"][0] == S and out["n_skipped"][0] == 0 and out["max_weight_share"][0] == pytest.approx(w.max() / w.sum())


@pytest.mark.parametrize("k", LS.GPD_K)
@pytest.mark.parametrize("seed", LS.GPD_SEEDS)
def test_khat_on_exact_generalized_pareto_draws(k, seed):
    """The fitted shape on M = 2000 exact draws within 4 (1 + k) / sqrt(M), four asymptotic standard deviations of the
    maximum-likelihood shape (the weak prior moves it by (0.5 - k) 10 / (M + 10), a hundredth of the bar)."""
    from scipy.stats import genpareto

    x = genpareto.rvs(k, size=LS.GPD_M, random_state=seed)
    got = LO.gpd_khat(x)
    bar = 4 * (1 + k) / np.sqrt(LS.GPD_M)
    print("k = %g, seed %d: khat = %.4f, off by %.2f of the bar" % (k, seed, got, abs(got - k) / bar))
    assert abs(got - k) <= bar
    assert LO.gpd_khat(x[:4]) == np.inf and LO.gpd_khat(np.r_[x, 0.0]) == np.inf and LO.gpd_khat(np.r_[x, np.nan]) == np.inf
    assert LO.tail_length(100) == 20 and LO.tail_length(262144) == 1536 and LO.tail_length(4) == 0
