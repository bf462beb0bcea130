"""CPU: everything of the fit report that needs no device -- the long-double restatement of the residual statistics against the
fixture the reference computed, its sequential accumulators against the defining sums and across chunkings, the layout of
``cf_resid_acc``, the argument rules of ``cf_resid_device`` (stated without a handle by ``cf_resid_check_args``), and the
centre / dof / keyword arithmetic of ``fit_report``."""
import ctypes as C
import importlib
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import resid_reference as R
import resid_shapes as RS
from conftest import ROOT, golden, load_pkg

amd = load_pkg()
L = amd._lib
F = importlib.import_module("cosmology-model-fit_amd.fit_report")


# ---- the restatement against the reference's own numbers -----------------------------------------------------------------------
@pytest.mark.parametrize("case", RS.FIXTURE_CASES)
def test_restatement_reproduces_the_fixture(case):
    g = golden("residuals")
    r, y = g[case + "/residuals"], g[case + "/y"]
    assert r.shape[0] == 8 and g[case + "/thetas"].shape[0] == 32
    worst = {}
    for k in range(r.shape[0]):
        got = R.sample_stats(r[k], y[k])
        for fx, col in RS.FIXTURE_COLUMNS.items():
            want = g[f"{case}/{fx}"][k]
            err = abs(float(got[col] - want)) if col in R.ABSOLUTE else abs(float(got[col] - want) / want)
            worst[col] = max(worst.get(col, 0.0), err)
    print(case, "largest error of the restatement against the fixture:", worst)
    for col, err in worst.items():
        assert err <= (RS.ABS if col in R.ABSOLUTE else RS.REL), (case, col, err)


def test_restatement_is_plain_ieee_at_the_corners():
    one = R.sample_stats([0.25], [3.0], [0.5])
    assert one["std"] == 0 and np.isnan(one["skew"]) and np.isnan(one["kurtosis"]) and one["r2"] == -np.inf
    assert one["max_pull"] == 0.5 and one["max_pull_index"] == 0
    flat = R.sample_stats([1.0, 1.0, 1.0], [1.0, 2.0, 4.0], [1.0, 1.0, 1.0])
    assert flat["std"] == 0 and np.isnan(flat["skew"]) and flat["max_pull_index"] == 0  # the first of equal pulls
    bad = R.sample_stats([1.0, np.nan, 5.0, np.nan], [1.0, 2.0, 3.0, 4.0], np.ones(4))
    assert np.isnan(bad["mean"]) and np.isnan(bad["max_pull"]) and bad["max_pull_index"] == 1  # the first NaN


# ---- the accumulators ----------------------------------------------------------------------------------------------------------
def _rows(weighted, seed=4, m=211, n=7):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((m, n)) * rng.uniform(0.1, 3.0, n) + rng.uniform(-2, 2, n)
    rows[17, 2] = np.nan
    rows[40, :] = np.inf
    w = None
    if weighted:
        w = rng.uniform(0.0, 1.0, m)
        w[[3, 99, 100]] = 0.0
    return rows, w, rng.uniform(0.5, 1.5, n)


@pytest.mark.parametrize("weighted", [False, True])
def test_accumulators_equal_the_two_pass_sums_and_do_not_depend_on_the_chunking(weighted):
    rows, w, sigma = _rows(weighted)
    m, n = rows.shape
    whole = R.accumulate(R.new_state(n, len(RS.THRESHOLDS)), rows, sigma, RS.THRESHOLDS, w)
    mean, std = R.two_pass(rows, w)
    fin = R.finish(whole, sigma)
    scale = np.abs(mean) + std
    assert float(np.max(np.abs(fin["mean"] - mean) / scale)) < 1e-17 * m
    assert float(np.max(np.abs(fin["std"] - std) / scale)) < 1e-17 * m
    skipped = 1 + (3 if weighted else 0)
    want_skipped = np.full(n, skipped)
    want_skipped[2] += 1
    assert np.array_equal(whole["n_skipped"], want_skipped) and np.array_equal(whole["n_used"], m - want_skipped)
    # exceedance: the weight of the used rows beyond each threshold
    wt = np.ones(m) if w is None else w
    for k, t in enumerate(RS.THRESHOLDS):
        with np.errstate(invalid="ignore"):
            beyond = np.isfinite(rows) & (np.abs(rows) > t * sigma[None, :]) & (wt > 0)[:, None]
        assert np.allclose(np.asarray(whole["exceed"][k], float), (beyond * wt[:, None]).sum(axis=0), rtol=1e-14, atol=0)
    for chunk in (1, 32, 96, m):
        st = R.new_state(n, len(RS.THRESHOLDS))
        for s0 in range(0, m, chunk):
            R.accumulate(st, rows[s0:s0 + chunk], sigma, RS.THRESHOLDS, None if w is None else w[s0:s0 + chunk])
        for key in whole:
            assert np.array_equal(st[key], whole[key]), (chunk, key)


# ---- the C side ----------------------------------------------------------------------------------------------------------------
def test_acc_layout_matches_c(tmp_path):
    fields = [name for name, _ in L.cf_resid_acc._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "cosmofit.h"\nint main(){printf("%zu %d %d %d", sizeof(cf_resid_acc), ' \
           'CF_RS_NCOL, CF_RESID_MAX_THR, CF_RESID_CHUNK);' + \
           "".join(f'printf(" %zu", offsetof(cf_resid_acc, {f}));' for f in fields) + "return 0;}"
    src, exe = tmp_path / "acc.c", tmp_path / "acc"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals[:4] == [C.sizeof(L.cf_resid_acc), L.CF_RS_NCOL, L.CF_RESID_MAX_THR, L.CF_RESID_CHUNK]
    assert len(L.RESID_COLUMNS) == L.CF_RS_NCOL and L.RESID_COLUMNS == R.COLUMNS
    for f, off in zip(fields, vals[4:]):
        assert getattr(L.cf_resid_acc, f).offset == off, f


def _check(n_sn=100, n_bao=13, quasar=0, n_devices=1, theta=1, S=5, block=L.CF_RB_SN, thr=(2.0, 3.0), n_thr=None, sample=1,
           blocks=0, acc=None):
    """cf_resid_check_args with non-null dummies (the function dereferences thresholds and acc only)."""
    t = np.asarray(thr, dtype=np.float64)
    return amd.lib().cf_resid_check_args(n_sn, n_bao, quasar, n_devices, theta or None, S, block, t.ctypes.data if t.size else None,
                                         t.size if n_thr is None else n_thr, sample or None, blocks or None, acc)


def test_argument_errors_are_reported_before_any_device_work():
    lib = amd.lib()
    inv, uns = -1, -5
    assert _check() == 0
    assert _check(quasar=1) == uns and b"quasar" in lib.cf_last_error()
    assert _check(n_devices=2) == uns and b"several devices" in lib.cf_last_error()
    assert _check(block=L.CF_RB_SN, n_sn=0) == inv and b"no SN block" in lib.cf_last_error()
    assert _check(block=L.CF_RB_BAO, n_bao=0) == inv and b"no BAO block" in lib.cf_last_error()
    assert _check(block=2) == inv and _check(block=-1) == inv
    assert _check(S=-1) == inv and _check(S=2**31) == inv
    assert _check(n_thr=5, thr=(1.0,) * 5) == inv and _check(n_thr=-1) == inv
    assert _check(thr=(), n_thr=2) == inv                     # thresholds announced, none given
    assert _check(thr=(1.0, np.nan)) == inv and _check(thr=(-1.0,)) == inv
    assert _check(theta=0) == inv and b"null theta" in lib.cf_last_error()
    assert _check(sample=0) == inv and b"no output" in lib.cf_last_error()
    assert _check(theta=0, S=0) == 0                          # no rows: a no-op, nothing is read
    acc, _ = RS.host_acc(L, 100, 2)
    assert _check(acc=C.byref(acc), sample=0) == 0
    assert _check(acc=C.byref(acc), block=L.CF_RB_BAO) == inv  # 100 data, the BAO block has 13
    assert _check(acc=C.byref(acc), thr=(1.0,)) == inv         # n_thr differs
    for field in ("w_sum", "mean", "m2", "exceed", "n_used", "n_skipped"):
        bad, _ = RS.host_acc(L, 100, 2)
        setattr(bad, field, None)
        assert _check(acc=C.byref(bad)) == inv, field
    bad, _ = RS.host_acc(L, 100, 2)
    bad.struct_size -= 8
    assert _check(acc=C.byref(bad)) == inv
    none, _ = RS.host_acc(L, 100, 0)
    none.exceed = None
    assert _check(acc=C.byref(none), thr=()) == 0             # no thresholds: exceed is not read
    # a null handle, with or without a device
    for fn, extra in ((lib.cf_resid_device, (None,)), (lib.cf_resid, ())):
        assert fn(None, None, 0, None, L.CF_RB_SN, None, 0, None, None, None, *extra) == inv
    assert lib.cf_resid_sigma(None, 0, None) == inv and lib.cf_resid_set_chunk(None, 32) == inv


# ---- fit_report's host arithmetic ----------------------------------------------------------------------------------------------
def _host_percentile(samples, q):
    return torch.from_numpy(np.percentile(samples.numpy(), q, axis=0))


def _host_weighted_quantile(x, w, q):
    out = np.empty((len(q), x.shape[1]))
    for c in range(x.shape[1]):
        idx = np.argsort(x[:, c].numpy(), kind="stable")
        cdf = np.cumsum(w.numpy()[idx])[:-1]
        cdf /= cdf[-1]
        out[:, c] = np.interp(q, np.append(0, cdf), x[:, c].numpy()[idx])
    return out


class _FakeEngine:
    """An engine of 4 parameters and 50 SNe whose 'statistics' are functions of the row, so the plumbing can be followed."""
    ndim, n_sn, n_bao = 4, 50, 0
    model_info = dict(quasar=False, multi_device=False)

    def chi_squared(self, theta):
        return float(np.sum(np.asarray(theta) ** 2))


def _fake_sample_stats(engine, samples, block="sn"):
    cols = torch.stack([samples.sum(dim=1) * (j + 1) for j in range(L.CF_RS_NCOL)], dim=1)
    return cols, torch.zeros((samples.shape[0], 10), dtype=torch.float64)


@pytest.fixture
def host_reductions(monkeypatch):
    monkeypatch.setattr(F._args, "on_device", lambda x, what: x)
    monkeypatch.setattr(F, "_percentile", _host_percentile)
    monkeypatch.setattr(F, "_weighted_quantile", _host_weighted_quantile)
    monkeypatch.setattr(F, "sample_stats", _fake_sample_stats)


def test_summary_centre_and_dof(host_reductions):
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.standard_normal((400, 4)) + np.array([-19.3, 70.0, 0.3, 0.0]))
    w = torch.from_numpy(rng.uniform(0, 1, 400))
    eng = _FakeEngine()
    s = F.summary(eng, x)
    assert np.array_equal(s["center"], np.percentile(x.numpy(), 50, axis=0))          # sn/pantheon.py:150
    assert s["dof"] == 50 - 4 and s["n_data"] == 50 and F.dof(1590, 4) == 1586         # sn/pantheon.py:181
    assert s["chi2"] == pytest.approx(float(np.sum(s["center"] ** 2)), rel=1e-15)
    assert s["at_center"]["ss_res"] == pytest.approx(3 * float(np.sum(s["center"])), rel=1e-14)
    want = np.percentile(x.numpy().sum(axis=1), [15.9, 50, 84.1])
    assert np.allclose(s["posterior"]["mean"], want, rtol=1e-14) and np.allclose(s["posterior"]["std"], 2 * want, rtol=1e-14)
    assert "max_pull_index" not in s["posterior"] and set(s["posterior"]) == set(F.COLUMNS[:-1])
    assert F.summary(eng, x, n_data=1829)["dof"] == 1825
    sm = F.summary(eng, x, center="mean")
    assert np.allclose(sm["center"], x.numpy().mean(axis=0), rtol=1e-14)
    sw = F.summary(eng, x, weights=w, center="mean")                                   # sn/pantheon_dipole_xyz.py:118
    assert np.allclose(sw["center"], (w.numpy()[:, None] * x.numpy()).sum(axis=0) / w.numpy().sum(), rtol=1e-13)
    sq = F.summary(eng, x, weights=w)                                                  # bao/desi_fs_lya.py:92-96
    assert np.array_equal(sq["center"], _host_weighted_quantile(x, w, [0.5])[0])
    assert np.array_equal(sq["posterior"]["mean"], _host_weighted_quantile(x.sum(dim=1)[:, None], w, np.array([0.159, 0.5, 0.841]))[:, 0])
    with pytest.raises(ValueError, match='"median" or "mean"'):
        F.summary(eng, x, center="mode")
    with pytest.raises(ValueError, match="at least one sample"):
        F.summary(eng, x[:0])


def test_keyword_and_argument_checks():
    eng = _FakeEngine()
    x = torch.zeros((5, 4), dtype=torch.float64)
    with pytest.raises(TypeError, match="unexpected keyword.*bins"):
        F.chain_report(eng, x, bins=40)
    for call in (lambda: F.sample_stats(eng, x), lambda: F.datum_stats(eng, x), lambda: F.report(eng, x), lambda: F.summary(eng, x)):
        with pytest.raises(ValueError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match=r"samples \[n, 4\]"):
        F.sample_stats(eng, torch.zeros((5, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        F.sample_stats(eng, x.float())
    with pytest.raises(ValueError, match="block must be one of"):
        F.sample_stats(eng, x, block="cc")
    with pytest.raises(ValueError, match="no BAO block"):
        F.sample_stats(eng, x, block="bao")
    with pytest.raises(ValueError, match="at most 4 thresholds"):
        F._thresholds((1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="finite and >= 0"):
        F._thresholds((1.0, -2.0))
    assert F._thresholds(()).size == 0 and F._thresholds(None).size == 0
    with pytest.raises(ValueError, match="chunk must be >= 1"):
        F.datum_stats(eng, x, chunk=0)
    quasar = SimpleNamespace(model_info=dict(quasar=True, multi_device=False), ndim=4, n_sn=50, n_bao=0)
    multi = SimpleNamespace(model_info=dict(quasar=False, multi_device=True), ndim=4, n_sn=50, n_bao=0)
    with pytest.raises(ValueError, match="quasar engine"):
        F.sample_stats(quasar, x)
    with pytest.raises(ValueError, match="several devices"):
        F.datum_stats(multi, x)
    with pytest.raises(ValueError, match="needs the likelihood's engine"):
        F.engine_of(lambda t: t)
    f = lambda t: t  # noqa: E731
    f.engine = eng
    assert F.engine_of(f) is eng and F.engine_of(lambda t: t, engine=eng) is eng


def test_samplers_refuse_weights_and_need_an_engine():
    import chain_gloo_worker as cw

    ens = cw.make_ensemble(24, (("stretch", 1.0),))
    ens.run_mcmc(2)
    with pytest.raises(TypeError, match="carry no weights"):
        ens.fit_report(weights=torch.ones(48, dtype=torch.float64))
    with pytest.raises(ValueError, match="needs the likelihood's engine"):
        ens.fit_report()
    with pytest.raises(ValueError, match="MI355X"):  # with an engine the next check is the device of the chain
        ens.fit_report(engine=SimpleNamespace(model_info=dict(quasar=False, multi_device=False), ndim=3, n_sn=50, n_bao=0))
