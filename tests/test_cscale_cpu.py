"""CPU: everything of the scaled covariance C(s) = C0 + s C1 that needs no device -- ``covscale.decompose`` against the long-double
restatement, the identity T C(s) T^T = I + s diag(lambda), the host twin of the row arithmetic (``cf_selftest_cscale_host``)
with its domain rules, the closed forms, the argument rules of ``cf_cscale_eval_device`` (stated without a handle by
``cf_cscale_check_args``) and the constants of ``_lib`` against the compiled header."""
import ctypes as C
import importlib
import os
import subprocess
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import cscale_reference as CR
import cscale_shapes as CS
from conftest import ROOT, load_pkg

amd = load_pkg()
L = amd._lib
V = importlib.import_module("cosmology-model-fit_amd.covscale")
LD = CR.LD


def _host(y, lam, s):
    """(quad [n_s], logdet [n_s]) of cf_selftest_cscale_host for one row."""
    y, lam, s = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, lam, s))
    q, ld = np.full(s.size, -7.0), np.full(s.size, -7.0)
    L.check(amd.lib().cf_selftest_cscale_host(y.ctypes.data, lam.ctypes.data, y.size, s.ctypes.data, s.size, q.ctypes.data,
                                              ld.ctypes.data))
    return q, ld


class Case:
    """One (n, kind): the factor, C1, its decomposition, 5 residual rows, 16 amplitudes and the restatement for them."""

    def __init__(self, n, kind):
        self.cov = CS.covariance(amd, n)
        self.chol = np.linalg.cholesky(self.cov)
        self.c1 = CS.second_matrix(kind, self.cov)
        self.T, self.lam, self.info = V.decompose(self.chol, self.c1)
        self.rows = CS.residual_rows(self.chol, 5, seed=n)
        self.s = CS.amplitudes(self.info)
        self.quad, self.logdet = CR.quad_logdet(self.chol, self.c1, self.rows, self.s)
        self.q_scale, self.l_scale = CR.scales(self.T, self.lam, self.rows, self.s)


_CASES = {}


def case(n, kind):
    if (n, kind) not in _CASES:
        _CASES[(n, kind)] = Case(n, kind)
    return _CASES[(n, kind)]


def _worst(err, scale):
    live = scale > 0
    assert not np.asarray(err, dtype=np.float64)[~live].any()  # a zero scale is a zero row or s = 0: exact
    return float(np.max(np.asarray(err, dtype=np.float64)[live] / scale[live])) if live.any() else 0.0


@pytest.mark.parametrize("n", CS.N_ALL)
def test_decompose_against_the_restatement(n):
    worst_q = worst_l = worst_p = 0.0
    for kind in CS.KINDS:
        c = case(n, kind)
        assert c.lam.shape == (n,) and (np.diff(c.lam) >= 0).all() and c.info["s_min"] < 0 < c.info["s_max"]
        y = c.rows @ c.T.T
        quad = (y * y)[:, None, :] / (1.0 + c.s[None, :, None] * c.lam[None, None, :])
        worst_q = max(worst_q, _worst(np.abs(quad.sum(axis=2) - c.quad), c.q_scale))
        worst_l = max(worst_l, _worst(np.abs(np.log1p(c.s[:, None] * c.lam[None, :]).sum(axis=1) - c.logdet), c.l_scale))
        worst_p = max(worst_p, c.info["probe_rel"])
        assert c.info["probe_rel"] <= V.PROBE_LIMIT
    print("n = %d: quad via T %.2e, logdet %.2e of the scale of the terms; probe_rel %.2e" % (n, worst_q, worst_l, worst_p))
    assert worst_q <= CR.BAR and worst_l <= CR.BAR


@pytest.mark.parametrize("n", [5, 33, 65, 257])
@pytest.mark.parametrize("kind", CS.KINDS)
def test_t_diagonalises_the_scaled_covariance(n, kind):
    c = case(n, kind)
    T = np.asarray(c.T, dtype=LD)
    C0, c1 = np.asarray(c.chol, dtype=LD) @ np.asarray(c.chol, dtype=LD).T, CR.c1_matrix(c.c1, n)
    bound = np.abs(c.T) @ (np.abs(c.cov) + np.abs(np.asarray(c1, dtype=np.float64))) @ np.abs(c.T).T
    for s in (c.s[0], 0.0, c.s[-1]):
        got = T @ (C0 + LD(s) * c1) @ T.T
        want = np.eye(n) + s * np.diag(c.lam)
        assert float(np.max(np.abs(np.asarray(got - want, dtype=np.float64)) / bound)) <= CR.BAR


def test_rounding_noise_eigenvalues_are_zeroed_and_put_no_bound_on_s():
    c = case(65, "diag01")
    assert np.count_nonzero(c.lam == 0.0) == 65 - 32 == c.info["n_zeroed"] and (c.lam >= 0).all()
    assert np.isfinite(c.info["s_min"]) and c.info["s_max"] == np.inf
    T, lam, info = V.decompose(c.chol, np.zeros((65, 65)))
    assert not lam.any() and info["s_min"] == -np.inf and info["s_max"] == np.inf and info["probe_rel"] <= V.PROBE_LIMIT
    _, lam, info = V.decompose(c.chol, -1.0)  # a negative definite C1 bounds s from above only
    assert (lam < 0).all() and info["s_min"] == -np.inf and info["s_max"] == -1.0 / lam.min()


def test_garbage_above_the_diagonal_of_the_factor_is_ignored():
    c = case(33, "rank4")
    dirty = c.chol + np.triu(np.full((33, 33), 1e300), 1)
    T, lam, info = V.decompose(dirty, c.c1)
    assert np.array_equal(T, c.T) and np.array_equal(lam, c.lam) and info == c.info
    for bad in (np.ones((3, 4)), np.diag([1.0, 0.0, 1.0]), np.diag([1.0, np.nan])):
        with pytest.raises(ValueError):
            V.decompose(bad, 1.0)
    with pytest.raises(ValueError, match="C1 must be"):
        V.decompose(c.chol, np.ones(5))


@pytest.mark.parametrize("n", CS.N_ALL)
def test_host_twin_of_the_row_arithmetic(n):
    worst_q = worst_l = 0.0
    for kind in CS.KINDS:
        c = case(n, kind)
        y = c.rows @ c.T.T
        for i in range(c.rows.shape[0]):
            q, ld = _host(y[i], c.lam, c.s)
            worst_q = max(worst_q, _worst(np.abs(q - c.quad[i]), c.q_scale[i]))
            worst_l = max(worst_l, _worst(np.abs(ld - c.logdet), c.l_scale))
            assert ld[3] == 0.0 and c.s[3] == 0.0  # s = 0: logdet exactly 0
            assert abs(q[3] - float(np.sum(y[i] * y[i]))) <= 4 * n * CR.EPS * q[3]
        q, ld = _host(np.zeros(n), c.lam, c.s)  # a zero row: exact zeros in quad
        assert not q.any() and np.array_equal(ld, _host(y[0], c.lam, c.s)[1])
    print("n = %d: host twin, quad %.2e logdet %.2e of the scale of the terms" % (n, worst_q, worst_l))
    assert worst_q <= CR.BAR and worst_l <= CR.BAR


def test_host_twin_domain_and_special_values_stay_in_their_column():
    c = case(65, "indefinite")
    y = c.rows[0] @ c.T.T
    clean_q, clean_l = _host(y, c.lam, c.s)
    assert np.isfinite(clean_q).all() and np.isfinite(clean_l).all()
    lo, hi = c.info["s_min"], c.info["s_max"]
    for j, bad in ((0, lo * (1 + 1e-12)), (5, hi * (1 + 1e-12)), (7, 2 * lo), (9, np.nan), (11, np.inf), (15, -np.inf)):
        s = c.s.copy()
        s[j] = bad
        q, ld = _host(y, c.lam, s)
        keep = np.arange(16) != j
        assert np.isnan(q[j]) and np.isnan(ld[j]), (j, bad)
        assert np.array_equal(q[keep], clean_q[keep]) and np.array_equal(ld[keep], clean_l[keep]), (j, bad)
    # just inside the domain is finite
    q, ld = _host(y, c.lam, [lo * (1 - 1e-9), hi * (1 - 1e-9)])
    assert np.isfinite(q).all() and np.isfinite(ld).all()
    # a NaN in y reaches quad of every amplitude of that row, and no logdet
    ybad = y.copy()
    ybad[3] = np.nan
    q, ld = _host(ybad, c.lam, c.s)
    assert np.isnan(q).all() and np.array_equal(ld, clean_l)
    lib = amd.lib()
    one = np.ones(4)
    assert lib.cf_selftest_cscale_host(None, one.ctypes.data, 4, one.ctypes.data, 1, None, None) == -1
    assert lib.cf_selftest_cscale_host(one.ctypes.data, one.ctypes.data, 0, one.ctypes.data, 1, None, None) == -1
    assert lib.cf_selftest_cscale_host(one.ctypes.data, one.ctypes.data, 4, one.ctypes.data, 17, None, None) == -1
    assert lib.cf_selftest_cscale_host(one.ctypes.data, one.ctypes.data, 4, one.ctypes.data, 0, None, None) == -1


def test_closed_forms():
    c = case(257, "c0")  # C1 = C0: C(s) = (1 + s) C0
    assert np.max(np.abs(c.lam - 1.0)) <= 1e-11
    y = c.rows @ c.T.T
    chi2 = np.asarray(CR.quad_logdet(c.chol, 0.0, c.rows, [0.0])[0][:, 0], dtype=np.float64)
    s = c.s[c.s > -0.95]
    for i in range(c.rows.shape[0]):
        q, ld = _host(y[i], c.lam, s)
        assert np.allclose(q, chi2[i] / (1 + s), rtol=1e-10, atol=0) and np.allclose(ld, 257 * np.log1p(s), rtol=1e-10, atol=1e-12)
    T, lam, _ = V.decompose(c.chol, 0.0)  # C1 = 0: nothing depends on s
    q, ld = _host(c.rows[1] @ T.T, lam, [-3.0, 0.0, 0.5, 1e6])
    assert (q == q[0]).all() and q[0] > 0 and not ld.any()


# ---- the C side ----------------------------------------------------------------------------------------------------------------
def test_constants_match_c(tmp_path):
    prog = '#include <stdio.h>\n#include "cosmofit.h"\nint main(){printf("%d %d %d %d %d %d", CF_CSCALE_MAX_S, CF_CSCALE_CHUNK, ' \
           'CF_OUT_CHI2, CF_OUT_LOGL, CF_OUT_LOGP, CF_ABI_VERSION);return 0;}'
    src, exe = tmp_path / "c.c", tmp_path / "c"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [L.CF_CSCALE_MAX_S, L.CF_CSCALE_CHUNK, L.CF_OUT_CHI2, L.CF_OUT_LOGL, L.CF_OUT_LOGP, L.CF_ABI_VERSION]
    assert V.MAX_S == 16 == CS.MAX_S and amd.lib().cf_abi_version() == 11  # appended entry points: the descriptor did not change
    for name in ("cf_cscale_create", "cf_cscale_destroy", "cf_cscale_look", "cf_cscale_apply_device", "cf_cscale_eval_device",
                 "cf_cscale_eval", "cf_cscale_check_args", "cf_cscale_set_chunk", "cf_selftest_cscale_host"):
        assert name in L.EXPORTS and hasattr(amd.lib(), name)
    assert amd.covscale is V


def _check(n_sn=100, quasar=0, n_devices=1, hdev=0, has=1, cn=None, cdev=0, theta=1, s=1, n_s=3, S=5, kind=L.CF_OUT_LOGP, out=1,
           parts=0):
    return amd.lib().cf_cscale_check_args(n_sn, quasar, n_devices, hdev, has, n_sn if cn is None else cn, cdev, theta or None,
                                          s or None, n_s, S, kind, out or None, parts or None)


def test_argument_errors_are_reported_before_any_device_work():
    lib = amd.lib()
    said = set()

    def refused(rc, words):
        msg = lib.cf_last_error()
        assert rc == -1 and words in msg, (rc, msg)
        said.add(msg)

    assert _check() == 0
    refused(_check(quasar=1), b"quasar")
    refused(_check(n_devices=2), b"several devices")
    refused(_check(n_sn=0), b"no SN block")
    refused(_check(has=0), b"null cf_cscale")
    refused(_check(cn=99), b"cf_cscale.n is not")
    refused(_check(cdev=1), b"another device")
    refused(_check(S=-1), b"S out of range")
    refused(_check(n_s=0), b"n_s must be in 1..16")
    refused(_check(kind=3), b"out_kind must be")
    refused(_check(out=0), b"no output")
    refused(_check(theta=0), b"null theta")
    refused(_check(s=0), b"null amplitudes")
    assert len(said) == 12  # each refusal with its own message
    assert _check(S=2**31) == -1 and _check(S=2**31 - 1) == 0 and _check(n_s=17) == -1 and _check(n_s=16) == 0 and _check(kind=-1) == -1
    assert _check(out=0, parts=1) == 0 and _check(kind=L.CF_OUT_CHI2) == 0 and _check(kind=L.CF_OUT_LOGL) == 0
    assert _check(theta=0, s=0, S=0) == 0  # no rows: a no-op, nothing is read
    # null handles and objects, with or without a device
    assert lib.cf_cscale_eval_device(None, None, None, None, 1, 0, 0, None, None, None) == -1
    assert lib.cf_cscale_eval(None, None, None, None, 1, 0, 0, None, None) == -1
    assert lib.cf_cscale_apply_device(None, None, 4, 1, None, 1, None, None, None, None) == -1
    assert lib.cf_cscale_set_chunk(None, 32) == -1 and lib.cf_cscale_look(None, None, None) == -1
    lib.cf_cscale_destroy(None)


def test_create_refuses_bad_arguments():
    lib = amd.lib()
    p, eye, lam = C.c_void_p(), np.eye(4), np.ones(4)
    create = lambda T, n, ld, lm, out: lib.cf_cscale_create(T, n, ld, lm, 0, out)
    assert create(None, 4, 4, lam.ctypes.data, C.byref(p)) == -1 and create(eye.ctypes.data, 4, 4, None, C.byref(p)) == -1
    assert create(eye.ctypes.data, 4, 4, lam.ctypes.data, None) == -1
    assert create(eye.ctypes.data, 0, 4, lam.ctypes.data, C.byref(p)) == -1 and create(eye.ctypes.data, 32769, 32769, lam.ctypes.data, C.byref(p)) == -1
    assert create(eye.ctypes.data, 4, 3, lam.ctypes.data, C.byref(p)) == -1 and b"ld < n" in lib.cf_last_error()
    bad = eye.copy()
    bad[1, 3] = np.inf
    assert create(bad.ctypes.data, 4, 4, lam.ctypes.data, C.byref(p)) == -1 and b"non-finite entry of T" in lib.cf_last_error()
    badl = lam.copy()
    badl[2] = np.nan
    assert create(eye.ctypes.data, 4, 4, badl.ctypes.data, C.byref(p)) == -1 and b"non-finite eigenvalue" in lib.cf_last_error()
    if lib.cf_device_count() == 0:
        assert create(eye.ctypes.data, 4, 4, lam.ctypes.data, C.byref(p)) == -2 and b"no HIP device" in lib.cf_last_error()
    assert not p.value


def test_scaled_covariance_checks_its_engine_and_bounds():
    chol = np.linalg.cholesky(CS.covariance(amd, 17))
    eng = SimpleNamespace(model_info=dict(quasar=False, multi_device=False), ndim=3, n_sn=17, mock_data=dict(sn_chol=chol))
    with pytest.raises(ValueError, match="quasar engine"):
        V.ScaledCovariance(SimpleNamespace(model_info=dict(quasar=True)), 1.0, (0, 1))
    with pytest.raises(ValueError, match="several devices"):
        V.ScaledCovariance(SimpleNamespace(model_info=dict(quasar=False, multi_device=True)), 1.0, (0, 1))
    with pytest.raises(ValueError, match="no SN block"):
        V.ScaledCovariance(SimpleNamespace(model_info={}, mock_data=dict(sn_chol=None), n_sn=0), 1.0, (0, 1))
    with pytest.raises(ValueError, match="power must be"):
        V.ScaledCovariance(eng, 1.0, (0, 1), power=3)
    with pytest.raises(ValueError, match="finite interval"):
        V.ScaledCovariance(eng, 1.0, (1, 0))
    with pytest.raises(ValueError, match="must not go below 0"):
        V.ScaledCovariance(eng, 1.0, (-0.001, 1), power=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(UserWarning, match="cut to the domain"):
            V.ScaledCovariance(eng, 1.0, (-1e6, 1.0))
