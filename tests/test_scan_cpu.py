"""CPU: everything of the template scan that needs no device -- ``scan.prepare`` against the long-double restatement
(tests/scan_reference.py, which never forms V), the restatement's block elimination against the brute-force joint fit, s_k^2
against ``nuisance.project``'s chi2_prof with and without the candidate, the candidate builders on hand-made inputs, the host
twin of the two reductions (``cf_selftest_scan_host``), the argument rules (``cf_scan_check_args``, ``cf_scan_create``), the
constants of ``_lib`` against the compiled header, the look-elsewhere arithmetic, and the seeds of the GPU kernel tests: the
restatement alone has no row whose two leading statistics lie within the tolerance of each other."""
import ctypes as C
import importlib
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import marg_shapes as MS
import scan_reference as SR
import scan_shapes as SS
from conftest import ROOT, load_pkg

amd = load_pkg()
L = amd._lib
N = importlib.import_module("cosmology-model-fit_amd.nuisance")
SC = importlib.import_module("cosmology-model-fit_amd.scan")
LD = SR.LD
F64 = lambda x: np.asarray(x, dtype=np.float64)


def _cpu_case(n, m0, kind):
    """factor, base (priors of `kind`; components beyond the data are Gaussian whatever the kind), 14 candidates: random
    columns, every fourth with a Gaussian prior, number 1 a copy of base column 0 (dead when that is flat), number 5 a copy of
    number 0 (equal scores), 5 residual rows."""
    chol = np.linalg.cholesky(SS.covariance(amd, n))
    A0, s0 = (None, None) if m0 == 0 else (MS.width(n, m0), MS.prior(kind, n, m0)[1])
    rng = np.random.default_rng(3100 + 7 * n + m0)
    A = rng.standard_normal((n, 14))
    sk = np.full(14, np.inf)
    sk[3::4] = 0.7
    if m0:
        A[:, 1] = A0[:, 0]
    A[:, 5] = A[:, 0]
    return chol, A0, s0, A, sk, SS.residual_rows(chol, 5, seed=n)


@pytest.mark.parametrize("kind", SS.PRIORS)
@pytest.mark.parametrize("m0", SS.M0_CPU)
@pytest.mark.parametrize("n", SS.N_CPU)
def test_prepare_against_the_restatement(n, m0, kind):
    chol, A0, s0, A, sk, rows = _cpu_case(n, m0, kind)
    p = SC.prepare(chol, A, base=A0, base_sigma=s0, cand_sigma=sk)
    ref = SR.restate(chol, A, rows, base=A0, base_sigma=s0, cand_sigma=sk)
    assert p["V"].shape == (n, 14) and p["F"].shape == p["live"].shape == (14,) and p["probe_rel"] <= SC.PROBE_LIMIT
    assert 0 in p["probe_columns"] and 13 in p["probe_columns"] and len(p["probe_columns"]) >= 8
    assert np.array_equal(p["live"], ref["live"]), (p["live"], ref["live"])
    if m0 and np.isinf(s0[0]):
        assert not p["live"][1]                                   # a copy of a flat base column
    if m0 >= n and kind == "flat":
        assert not p["live"][np.isinf(sk)].any()                  # the flat base spans the data: only a prior keeps a candidate alive
    assert not p["V"][:, ~p["live"]].any() and not p["F"][~p["live"]].any()
    s = rows @ p["V"]
    scale = SR.scale(p["V"], rows)[:, None]
    live_rows = scale[:, 0] > 0
    err = np.abs(F64(s - ref["s"]))
    # a row without a scale is a zero row, or every candidate has lost its whole direction to the base (n = 1): a score is at most
    # sqrt(chi^2) by Cauchy-Schwarz, and what is left of it there is the rounding of a complete cancellation
    assert (err[~live_rows] <= SR.EPS * np.sqrt(F64(ref["chi2_0"]))[~live_rows, None]).all()
    worst = float(np.max(err[live_rows] / scale[live_rows])) if live_rows.any() and p["live"].any() else 0.0
    f_err = float(np.max(np.abs(F64(p["F"] - ref["F"])) / np.maximum(F64(p["aKa"]) + 1.0 / sk ** 2, 1e-300)))
    print("n = %d m0 = %d %s: scores %.2e of the terms summed, F %.2e of a^T K a + 1 / sigma^2" % (n, m0, kind, worst, f_err))
    assert worst <= SR.BAR and f_err <= SR.BAR
    assert np.array_equal(s[:, 5], s[:, 0]) and p["F"][5] == p["F"][0]  # a candidate equal to another: equal scores
    assert not (rows @ p["V"][:, ~p["live"]]).any()                      # exactly 0.0


@pytest.mark.parametrize("m0", (0, 1, 3, 16))
@pytest.mark.parametrize("n", (2, 33, 65))
def test_the_restatement_against_the_brute_force_joint_fit(n, m0):
    chol, A0, s0, A, sk, rows = _cpu_case(n, m0, "gauss" if m0 >= n else "flat")
    ref = SR.restate(chol, A, rows, base=A0, base_sigma=s0, cand_sigma=sk)
    for k in (0, 2, 3, 13):
        if not ref["live"][k]:
            continue
        s, d, a, err = SR.fit_one(chol, A[:, k], rows, base=A0, base_sigma=s0, a_sigma=sk[k])
        top = np.maximum(F64(ref["chi2_0"]), 1.0)
        assert (np.abs(F64(d - ref["dchi2"][:, k])) <= 1e-13 * top * max(1.0, 1.0 / float(ref["F"][k] * err * err))).all()
        assert (np.abs(F64(s * s - d)) <= 1e-13 * top).all()              # score^2 IS the drop of the chi^2
        assert (np.abs(F64(s - ref["s"][:, k])) <= 1e-13 * np.sqrt(top)).all() and abs(float(err - ref["alpha_err"][k])) <= 1e-14 * float(err)
        assert (np.abs(F64(a - ref["alpha_hat"][:, k])) <= 1e-13 * np.sqrt(top) * float(err)).all()


@pytest.mark.parametrize("m0", (0, 1, 3))
@pytest.mark.parametrize("n", (33, 257))
def test_scores_squared_are_the_drop_of_the_profiled_chi2(n, m0):
    chol, A0, s0, A, sk, rows = _cpu_case(n, m0, "flat")
    p = SC.prepare(chol, A, base=A0, base_sigma=s0, cand_sigma=sk)
    s = rows @ p["V"]
    Ki = np.linalg.inv(chol @ chol.T)
    chi2_0 = np.einsum("si,ij,sj->s", rows, Ki, rows)

    def prof(cols, sigma):
        if cols is None:
            return chi2_0, np.abs(chi2_0)
        pr = N.project(chol, cols, sigma=sigma)
        t = rows @ pr["Wt"]
        return chi2_0 - (t * t).sum(axis=1), np.abs(chi2_0) + ((np.abs(rows) @ np.abs(pr["Wt"])) ** 2).sum(axis=1)

    base_chi2, _ = prof(A0, s0)
    for k in (0, 2, 3, 7, 13):
        both = A[:, k:k + 1] if A0 is None else np.column_stack([A0, A[:, k]])
        with_k, v_scale = prof(both, [sk[k]] if A0 is None else np.concatenate([s0, [sk[k]]]))
        some = v_scale > 0                                            # a zero row has no scale and no error
        assert not (s[~some, k] ** 2 - (base_chi2 - with_k)[~some]).any()
        err = float(np.max(np.abs(s[some, k] ** 2 - (base_chi2 - with_k)[some]) / v_scale[some]))
        print("n = %d m0 = %d k = %d: %.2e of the terms summed" % (n, m0, k, err))
        assert err <= SR.BAR


def test_prepare_refuses_bad_arguments():
    chol = np.linalg.cholesky(SS.covariance(amd, 17))
    A = np.random.default_rng(0).standard_normal((17, 5))
    with pytest.raises(ValueError, match="mean zero"):
        SC.prepare(chol, A, base=np.ones(17), base_mu=[0.1])
    assert SC.prepare(chol, A, base=np.ones(17), base_mu=[0.0])["m0"] == 1
    for kw in (dict(cand=np.ones((16, 2))), dict(cand=np.full((17, 2), np.nan)), dict(cand=A, cand_sigma=0.0),
               dict(cand=A, base=np.ones((17, 17))), dict(cand=A, base=np.ones(17), base_sigma=[-1.0]),
               dict(cand=A, base=np.column_stack([np.ones(17), 2 * np.ones(17)]))):
        with pytest.raises(ValueError):
            SC.prepare(chol, **kw)
    with pytest.raises(ValueError):
        SC.prepare(np.ones((3, 4)), np.ones(3))
    assert not SC.prepare(chol, np.zeros((17, 1)))["live"][0]            # a zero candidate is dead, not an error
    Vn = SC.null_matrix(chol, A)
    assert np.allclose(Vn, np.tril(chol).T @ A, rtol=0, atol=0)
    keys = {SC.null_key(s) for s in range(64)}
    assert len(keys) == 64 and all(0 <= k < 2**64 for k in keys) and SC.null_key(3) != N.recover_key(3)


# ---- the builders --------------------------------------------------------------------------------------------------------------
def test_candidate_builders_on_hand_made_inputs():
    Cd = SC.Candidates
    z = np.array([0.1, 0.3, 0.3, 0.5, 0.9])
    cols, tab = Cd.steps(z)
    assert [t["z_t"] for t in tab] == pytest.approx([0.2, 0.4, 0.7]) and all(t["kind"] == "step" for t in tab)
    assert np.array_equal(cols.T, [[0, 1, 1, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 0, 1]])
    cols, tab = Cd.steps(z, thresholds=[0.3, 2.0])                       # a tie at the threshold is not above it; nothing above 2
    assert np.array_equal(cols.T, [[0, 0, 0, 1, 1], [0, 0, 0, 0, 0]])
    cols, tab = Cd.windows(z, [0.0, 0.3, 0.5, 1.0])
    assert [(t["lo"], t["hi"]) for t in tab] == [(0.0, 0.3), (0.0, 0.5), (0.0, 1.0), (0.3, 0.5), (0.3, 1.0), (0.5, 1.0)]
    assert np.array_equal(cols.T, [[1, 0, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [0, 1, 1, 0, 0], [0, 1, 1, 1, 1], [0, 0, 0, 1, 1]])
    cols, tab = Cd.windows(z, [0.0, 0.3, 0.5, 1.0], max_bins=1)          # the lower edge is inside, the upper one is not
    assert [t["bins"] for t in tab] == [1, 1, 1] and np.array_equal(cols.sum(axis=1), np.ones(5))
    cols, _ = Cd.windows(z, [0.6, 0.7, 0.8])                             # empty windows: zero columns (dead in a scan)
    assert cols.shape == (5, 3) and not cols.any()
    with pytest.raises(ValueError):
        Cd.windows(z, [0.3, 0.3])
    dirs = np.array([[0, 0, 1.0], [0, 0, -2.0], [1.0, 0, 0], [0, 3.0, 0], [1.0, 1.0, 0]])
    cols, tab = Cd.hemispheres(dirs, [[0, 0, 5.0], [1.0, 0, 0]])
    assert np.array_equal(cols.T, [[1, -1, 0, 0, 0], [0, 0, 1, 0, 1]]) and tab[0]["centre"] == (0.0, 0.0, 1.0)
    cols, tab = Cd.caps(dirs, [[0, 0, 1.0], [1.0, 0, 0]], [44.0, 46.0, 180.0])
    assert [(t["centre"][2], t["radius_deg"]) for t in tab[:3]] == [(1.0, 44.0), (1.0, 46.0), (1.0, 180.0)]
    assert np.array_equal(cols[:, 0], [1, 0, 0, 0, 0]) and np.array_equal(cols[:, 2], np.ones(5))   # the pole itself; the whole sphere
    assert np.array_equal(cols[:, 3], [0, 0, 1, 0, 0]) and np.array_equal(cols[:, 4], [0, 0, 1, 0, 1])  # (1, 1, 0) is 45 degrees from x
    assert cols[0, 1] == 1 and cols[1, 1] == 0 and cols[1, 2] == 1       # the other pole is inside the whole sphere only
    with pytest.raises(ValueError):
        Cd.caps(dirs, [[0, 0, 0.0]], [10.0])
    cols, tab = Cd.labels(np.array(["b", "a", "b", "c", "a"]))
    assert [t["label"] for t in tab] == ["a", "b", "c"] and np.array_equal(cols.T, [[0, 1, 0, 0, 1], [1, 0, 1, 0, 0], [0, 0, 0, 1, 0]])
    cols, tab = Cd.singles(4)
    assert np.array_equal(cols, np.eye(4)) and [t["index"] for t in tab] == [0, 1, 2, 3]
    P = Cd.fibonacci_sphere(200)
    assert P.shape == (200, 3) and np.allclose(np.linalg.norm(P, axis=1), 1.0, atol=1e-15) and np.abs(P.mean(axis=0)).max() < 0.01
    assert np.allclose(Cd.fibonacci_sphere(1)[0, 2], 0.0) and Cd.fibonacci_sphere(2)[0, 2] == 0.5
    w = np.array([1.0, 0.5, 0.0, 2.0, 1.0])
    fam = Cd.steps(z)
    cols, tab = Cd.times(fam, w)
    assert np.array_equal(cols, fam[0] * w[:, None]) and all(t["weighted"] for t in tab) and "weighted" not in fam[1][0]
    both = Cd.stack(fam, Cd.singles(5))
    assert both[0].shape == (5, 8) and len(both[1]) == 8 and both[1][3]["kind"] == "single"
    with pytest.raises(ValueError):
        Cd.times(fam, w[:4])
    assert np.array_equal(SC.statistic(np.array([-2.0, 3.0]), 0), [4.0, 9.0])
    assert np.array_equal(SC.statistic(np.array([-2.0, 3.0]), 1), [0.0, 9.0]) and np.array_equal(SC.statistic(np.array([-2.0, 3.0]), -1), [4.0, 0.0])


# ---- the host twin of the reductions -----------------------------------------------------------------------------------------
def _selftest(m, live=None, sign=0, w=None, colacc=None, pitch=None):
    m = np.ascontiguousarray(m, dtype=np.float64)
    S, K = m.shape[0], (m.shape[1] if pitch is None else pitch[1])
    best, k, s = np.empty(S), np.empty(S, dtype=np.int32), np.empty(S)
    lv = None if live is None else np.ascontiguousarray(np.asarray(live, dtype=np.uint8))
    d = lambda a: None if a is None else a.ctypes.data
    L.check(amd.lib().cf_selftest_scan_host(d(m), S, K, m.shape[1], d(lv), sign, d(w), d(best), d(k), d(s), d(colacc)))
    return best, k, s


def test_host_twin_ties_nan_rows_dead_columns_and_signs():
    m = np.array([[1.0, -3.0, 3.0, 2.0], [0.5, 0.5, -0.5, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, np.nan, 2.0, 0.0], [np.inf, 0.0, 1.0, 2.0],
                  [-1.0, -2.0, -0.5, -4.0]])
    best, k, s = _selftest(m)
    assert np.array_equal(k, [1, 0, 0, -1, -1, 3])                        # ties go to the smallest k; a non-finite score: -1
    assert np.array_equal(best[[0, 1, 2, 5]], [9.0, 0.25, 0.0, 16.0]) and np.array_equal(s[[0, 1, 2, 5]], [-3.0, 0.5, 0.0, -4.0])
    assert np.isnan(best[[3, 4]]).all() and np.isnan(s[[3, 4]]).all()
    best, k, s = _selftest(m, sign=1)
    assert np.array_equal(k, [2, 0, 0, -1, -1, 0]) and np.array_equal(best[[0, 1, 2, 5]], [9.0, 0.25, 0.0, 0.0]) and s[5] == -1.0
    best, k, s = _selftest(m, sign=-1)
    assert np.array_equal(k, [1, 2, 0, -1, -1, 3]) and np.array_equal(best[[0, 1, 2, 5]], [9.0, 0.25, 0.0, 16.0])
    best, k, s = _selftest(m, live=[0, 0, 1, 1])                          # dead candidates never win, not even a tie at zero
    assert np.array_equal(k, [2, 2, 2, -1, -1, 3]) and np.array_equal(best[[0, 1, 2, 5]], [9.0, 0.25, 0.0, 16.0])
    best, k, s = _selftest(m, live=[0, 0, 0, 0])                          # nothing alive: nothing to report
    assert (k == -1).all() and np.isnan(best).all()
    best, k, s = _selftest(m, pitch=(6, 2))                               # the first two columns of a wider map
    assert np.array_equal(k, [1, 0, 0, -1, -1, 1])
    # best is the maximum of the statistics of the map's own scores, to the bit, across tile boundaries
    rng = np.random.default_rng(5)
    big = rng.standard_normal((70, 200))
    for sign in (0, 1, -1):
        best, k, s = _selftest(big, sign=sign)
        stat = SC.statistic(big, sign)
        assert np.array_equal(best, stat.max(axis=1)) and np.array_equal(k, stat.argmax(axis=1)) and np.array_equal(s, big[np.arange(70), k])
    lib = amd.lib()
    one = np.zeros((1, 1))
    assert lib.cf_selftest_scan_host(None, 1, 1, 1, None, 0, None, None, None, None, None) == -1
    assert lib.cf_selftest_scan_host(one.ctypes.data, 1, 1, 1, None, 2, None, None, None, None, None) == -1 and b"sign" in lib.cf_last_error()
    assert lib.cf_selftest_scan_host(one.ctypes.data, 1, 2, 1, None, 0, None, None, None, None, None) == -1
    assert lib.cf_selftest_scan_host(one.ctypes.data, 0, 1, 1, None, 0, None, None, None, None, None) == -1


def test_host_twin_block_order_of_the_column_sums():
    rng = np.random.default_rng(11)
    S, K = 150, 5                                                         # two whole blocks of 64 rows and a part of one
    m, w = rng.standard_normal((S, K)) * 10.0 ** rng.uniform(-3, 3, (S, 1)), rng.uniform(0.0, 2.0, S)
    for weights in (None, w):
        start = rng.standard_normal(2 * K + 1)
        acc = start.copy()
        _selftest(m, w=weights, colacc=acc)
        want = start.copy()
        ww = np.ones(S) if weights is None else weights
        for k in range(K):
            for r0 in range(0, S, SS.TILE):
                a1 = a2 = 0.0
                for r in range(r0, min(S, r0 + SS.TILE)):                 # ascending rows from 0.0, sum w s^2 by one fused multiply-add
                    ws = ww[r] * m[r, k]
                    a1 = a1 + ws
                    a2 = float(np.longdouble(ws) * np.longdouble(m[r, k]) + np.longdouble(a2))
                want[2 * k] += a1
                want[2 * k + 1] += a2
        for r0 in range(0, S, SS.TILE):
            sw = 0.0
            for r in range(r0, min(S, r0 + SS.TILE)):
                sw = sw + ww[r]
            want[2 * K] += sw
        assert np.array_equal(acc[0::2], want[0::2]), "sum w s and sum w"
        # the fused multiply-add rounds once: the long-double emulation above can differ from it by double rounding only
        assert (np.abs(acc[1::2] - want[1::2]) <= 4 * SR.EPS * np.abs(want[1::2])).all()
        two_pass = np.array([[np.sum(np.asarray(ww * m[:, k], dtype=LD)), np.sum(np.asarray(ww * m[:, k], dtype=LD) * m[:, k])] for k in range(K)])
        got = (acc - start)[:-1].reshape(K, 2)
        assert (np.abs(F64(got[:, 0] - two_pass[:, 0])) <= 1e-10 * (np.abs(m) * ww[:, None]).sum(axis=0)).all()
        assert (np.abs(F64(got[:, 1] - two_pass[:, 1])) <= 1e-10 * (m * m * ww[:, None]).sum(axis=0)).all()


# ---- the C side ----------------------------------------------------------------------------------------------------------------
def test_constants_match_c(tmp_path):
    prog = '#include <stdio.h>\n#include "cosmofit.h"\nint main(){printf("%d %d %lld %d", CF_SCAN_CHUNK, CF_SCAN_TILE, ' \
           '(long long)CF_SCAN_MAX_K, CF_ABI_VERSION);return 0;}'
    src, exe = tmp_path / "c.c", tmp_path / "c"
    src.write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert vals == [L.CF_SCAN_CHUNK, L.CF_SCAN_TILE, L.CF_SCAN_MAX_K, L.CF_ABI_VERSION]
    assert SS.TILE == L.CF_SCAN_TILE and L.CF_SCAN_MAX_K == 2**24 - 1 and amd.lib().cf_abi_version() == 11  # appended entry points only
    assert SC.MAX_BASE == 16 and SC.PROBE_LIMIT == N.PROBE_LIMIT
    for name in ("cf_scan_create", "cf_scan_destroy", "cf_scan_info", "cf_scan_apply_device", "cf_scan_eval_device", "cf_scan_eval",
                 "cf_scan_check_args", "cf_scan_set_chunk", "cf_selftest_scan_host"):
        assert name in L.EXPORTS and hasattr(amd.lib(), name)
    assert amd.scan is SC


def _check(n_sn=100, quasar=0, n_devices=1, hdev=0, has=1, sn=None, K=7, sdev=0, theta=1, S=5, sign=0, n_out=1, map_=0, map_pitch=0):
    return amd.lib().cf_scan_check_args(n_sn, quasar, n_devices, hdev, has, n_sn if sn is None else sn, K, sdev, theta or None, S, sign,
                                        n_out, map_ or None, map_pitch)


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
    refused(_check(has=0), b"null cf_scan")
    refused(_check(sn=99), b"cf_scan.n is not")
    refused(_check(sdev=1), b"another device")
    refused(_check(sign=2), b"sign must be")
    refused(_check(S=-1), b"S out of range")
    refused(_check(n_out=0), b"no output")
    refused(_check(map_=1, map_pitch=6), b"map pitch below K")
    refused(_check(theta=0), b"null theta")
    assert len(said) == 11  # each refusal with its own message
    assert _check(S=2**31) == -1 and _check(S=2**31 - 1) == 0 and _check(sign=-2) == -1 and _check(sign=-1) == 0 and _check(sign=1) == 0
    assert _check(map_=1, map_pitch=7) == 0 and _check(theta=0, S=0) == 0
    assert lib.cf_scan_eval_device(None, None, None, 0, 0, None, None, None, None, None, None, 0, None, None) == -1
    assert lib.cf_scan_eval(None, None, None, 0, 0, None, None, None, None, None, None, 0, None) == -1
    assert lib.cf_scan_apply_device(None, None, 4, 1, 0, None, None, None, None, None, 0, None, None) == -1
    assert lib.cf_scan_set_chunk(None, 32) == -1 and lib.cf_scan_info(None, None, None, None, None) == -1
    lib.cf_scan_destroy(None)


def test_create_refuses_bad_arguments():
    lib = amd.lib()
    p, V = C.c_void_p(), np.ones((4, 3))
    create = lambda V_, n=4, K=3, ld=3, out=C.byref(p): lib.cf_scan_create(V_, n, K, ld, None, 0, out)
    d = lambda a: a.ctypes.data
    assert create(None) == -1 and create(d(V), out=None) == -1
    assert create(d(V), n=0) == -1 and create(d(V), n=32769) == -1 and b"1..32768" in lib.cf_last_error()
    assert create(d(V), K=0) == -1 and create(d(V), K=2**24) == -1 and b"2^24" in lib.cf_last_error()
    assert create(d(V), ld=2) == -1 and b"pitch below K" in lib.cf_last_error()
    bad = V.copy()
    bad[3, 2] = np.inf
    assert create(d(bad)) == -1 and b"non-finite entry of V" in lib.cf_last_error()
    if lib.cf_device_count() == 0:
        assert create(d(V)) == -2 and b"no HIP device" in lib.cf_last_error()
    assert not p.value


def test_template_scan_checks_its_engine_and_arguments():
    chol = np.linalg.cholesky(SS.covariance(amd, 17))
    eng = SimpleNamespace(model_info=dict(quasar=False, multi_device=False), ndim=3, n_sn=17, mock_data=dict(sn_chol=chol))
    A = np.eye(17)
    with pytest.raises(ValueError, match="quasar engine"):
        SC.TemplateScan(SimpleNamespace(model_info=dict(quasar=True)), A)
    with pytest.raises(ValueError, match="several devices"):
        SC.TemplateScan(SimpleNamespace(model_info=dict(quasar=False, multi_device=True)), A)
    with pytest.raises(ValueError, match="no SN block"):
        SC.TemplateScan(SimpleNamespace(model_info={}, mock_data=dict(sn_chol=None), n_sn=0), A)
    with pytest.raises(ValueError, match="sign must be"):
        SC.TemplateScan(eng, A, sign=2)
    with pytest.raises(ValueError, match="one entry per candidate"):
        SC.TemplateScan(eng, (A, [dict(kind="single")]))
    with pytest.raises(ValueError, match=r"cand must be \[17, k\]"):
        SC.TemplateScan(eng, np.eye(16))


# ---- the look-elsewhere arithmetic --------------------------------------------------------------------------------------------
def test_global_p_and_its_binomial_interval():
    from scipy import stats

    null = np.arange(1.0, 1000.0)                                         # 999 draws: 1, 2, .. 999
    r = SC.global_p(990.0, null)
    assert r["n_exceed"] == 10 and r["n_draws"] == 999 and r["p_global"] == 11 / 1000
    lo, hi = r["p_interval"]
    a = 0.5 * (1 - 0.6827)
    assert lo == pytest.approx(stats.beta.ppf(a, 10, 990)) and hi == pytest.approx(stats.beta.ppf(1 - a, 11, 989)) and lo < 10 / 999 < hi
    assert r["sigma_global"] == pytest.approx(stats.norm.isf(0.5 * 0.011)) and r["local_sigma"] == pytest.approx(np.sqrt(990.0))
    assert r["p_local"] == pytest.approx(stats.chi2.sf(990.0, 1)) and r["n_trials"] == pytest.approx(0.011 / r["p_local"])
    r = SC.global_p(4.0, null, sign=1)
    assert r["p_local"] == pytest.approx(0.5 * stats.chi2.sf(4.0, 1)) and r["n_exceed"] == 996
    r = SC.global_p(1e6, null)                                            # never 0: the observed data count as one draw
    assert r["p_global"] == 1 / 1000 and r["p_interval"][0] == 0.0 and r["n_exceed"] == 0
    r = SC.global_p(0.0, null)
    assert r["p_global"] == 1.0 and r["p_interval"][1] == 1.0 and r["sigma_global"] == 0.0
    # K = 1 under the null: p_global is p_local within the interval
    rng = np.random.default_rng(3)
    draws = rng.standard_normal(20000) ** 2
    r = SC.global_p(3.0, draws)
    assert r["p_interval"][0] - 3 * (r["p_interval"][1] - r["p_interval"][0]) <= r["p_local"] <= r["p_interval"][1] + 3 * (r["p_interval"][1] - r["p_interval"][0])
    for bad in (dict(observed=np.nan, null=null), dict(observed=-1.0, null=null), dict(observed=1.0, null=[]), dict(observed=1.0, null=[np.inf])):
        with pytest.raises(ValueError):
            SC.global_p(**bad)


# ---- the seeds of the GPU kernel tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SS.KERNEL + (SS.LARGE,), ids=lambda s: "%d-%d-%d-%d" % s)
def test_the_restatement_has_no_near_ties_at_the_kernel_shapes(shape):
    c = SS.kernel_case(amd, shape)
    assert c.prep["probe_rel"] <= SC.PROBE_LIMIT and np.array_equal(c.prep["live"][c.cols], c.ref["live"])
    if shape == SS.LARGE:
        assert np.array_equal(c.prep["live"], c.live64)
    assert not c.excused.any(), np.nonzero(c.excused)[0]
    if c.K >= 3 and c.m0:
        assert not c.prep["live"][1]                                      # every shape with a base carries a dead candidate
    # what the GPU tests will hold the device to, held here to a float64 product with prepare's V
    s = c.rows @ c.prep["V"][:, c.cols]
    assert (np.abs(F64(s - c.ref["s"])) <= c.tol[:, None]).all()
