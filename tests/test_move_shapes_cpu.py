"""CPU: the cases of tests/move_shapes.py are fair before any of them runs on a GPU.

  conditions  every covariance is well conditioned, and a float64 numpy restatement of either kernel form (one pass over
              moments about the first row for ndim <= 8, two passes above; the log-sum-exp in chunks of 2048 with the running
              rescale) is within 1e-13 (fit) and 1e-12 (scaled log factor) of the long-double judge: the GPU bars, 1e-11 and 1e-9,
              are not asking for more than float64 can give.
  reach       every value of every list is reached; every multi-chunk case has rows whose maximum lies in the first and in a
              later chunk.
  sharpness   the bars see a dropped centre, an omitted rescale, nc for nc - 1, a dropped term or a shifted partner of the
              nested proposal.
  agreement   the judge agrees with scipy.stats.gaussian_kde and with oracle/moves_torch.py.
"""
import math
import types

import numpy as np
import pytest

import move_shapes as ms
import moves_reference as mr
import nested_reference as nr

LD = np.longdouble
KDE_BAR = 1e-9   # the GPU bar of the KDE factor, relative to |log kde(x)| + |log kde(q)| + 1
FIT_BAR = 1e-11  # the GPU bar of the fit, relative to each matrix's largest element


# ---- float64 restatements of the two kernel forms ------------------------------------------------------------------------
def fit_f64(comp):
    comp = np.asarray(comp, dtype=np.float64)
    nc, d = comp.shape
    h = (nc * (d + 2) / 4.0) ** (-1.0 / (d + 4))
    if d <= 8:  # kde_prepare_small: one pass, moments about the first row
        dd = comp - comp[0]
        s1, s2 = dd.sum(axis=0), dd.T @ dd
        cov = (s2 - np.outer(s1, s1) / nc) / (nc - 1) * (h * h)
    else:       # the run-time-dimension form: mean, then centred products
        cen = comp - comp.sum(axis=0) / nc
        cov = (cen.T @ cen) / (nc - 1) * (h * h)
    chol = mr.cholesky(cov)
    log_norm = -math.log(nc) - 0.5 * d * math.log(2.0 * math.pi) - np.log(np.diagonal(chol)).sum()
    return chol, np.ascontiguousarray(mr.lower_inverse(chol).T), log_norm


def chunked_lse_f64(e, rescale=True):
    """ens_kde_logfactor_kernel's streaming log-sum-exp over chunks of 2048 centres; rescale=False is the defect."""
    mx, s = np.full(e.shape[0], -np.inf), np.zeros(e.shape[0])
    for c0 in range(0, e.shape[1], ms.CHUNK):
        blk = e[:, c0:c0 + ms.CHUNK]
        new = np.maximum(mx, blk.max(axis=1))
        s = s * (np.exp(mx - new) if rescale else 1.0) + np.exp(blk - new[:, None]).sum(axis=1)
        mx = new
    return mx + np.log(s)


def factor_f64(key0, ids, x, comp, fit, rescale=True):
    d = comp.shape[1]
    j = mr.partner(key0, 0, ids, comp.shape[0])
    noise = np.stack([nr.normal(key0, 4 + 2 * k, ids) for k in range(d)], axis=1)
    q = comp[j] + noise @ fit[0].T
    wc = comp @ fit[1]
    lse = []
    for p in (x, q):
        wp = p @ fit[1]
        e = -0.5 * ((wp[:, None, :] - wc[None, :, :]) ** 2).sum(axis=2)
        lse.append(chunked_lse_f64(e, rescale) + fit[2])
    return lse[0] - lse[1]


def _rel(got, want):
    want = np.asarray(want, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - want)) / np.max(np.abs(want)))


def _fit_runs(pkg):
    for ndim, w_total, S in ms.FIT_CASES:
        pos = ms.fit_positions(ndim, w_total, S)
        for ki, split_key in enumerate(ms.split_keys()):
            for split in range(S):
                yield ndim, w_total, S, ki, split_key, split, pos


@pytest.fixture(scope="module")
def chunk_refs():
    """The long-double figures of every chunk case, computed once."""
    out = {}
    for ndim, nc in ms.CHUNK_CASES:
        pos, ids = ms.chunk_case(ndim, nc)
        comp, x = pos[1::2], pos[ids]
        fit = mr.kde_fit(comp)
        key0 = 900 + nc
        q, lf, lx, lq = mr.kde_propose(key0, ids, x, comp, fit)
        out[ndim, nc] = dict(pos=pos, ids=ids, comp=comp, x=x, fit=fit, key0=key0, q=q, lf=lf, lx=lx, lq=lq,
                             ex=mr.kde_exponents(x, comp, fit), eq=mr.kde_exponents(q, comp, fit))
    return out


# ---- conditions ------------------------------------------------------------------------------------------------------------
def test_the_judge_is_an_extended_type():
    assert np.finfo(LD).eps < 1e-18


def test_fit_cases_are_well_conditioned_and_float64_can_meet_the_bars(pkg):
    worst = dict(cond=0.0, fit=0.0, norm=0.0, lf=0.0)
    for ndim, w_total, S, ki, split_key, split, pos in _fit_runs(pkg):
        comp = pos[mr.comp_ids(split_key, S, split, w_total)]
        ids = mr.active_ids(split_key, S, split, w_total)
        assert comp.shape[0] > ndim and comp.shape[0] + ids.size == w_total
        cond = float(np.linalg.cond(mr.covariance(comp).astype(np.float64)))
        want, got = mr.kde_fit(comp), fit_f64(comp)
        e_fit = max(_rel(got[0], want[0]), _rel(got[1], want[1]))
        e_norm = float(abs(LD(got[2]) - want[2]))
        key0 = 1000 + 10 * ki + split
        _, lf, lx, lq = mr.kde_propose(key0, ids, pos[ids], comp, want)
        e_lf = float(np.max(np.abs(factor_f64(key0, ids, pos[ids], comp, got).astype(LD) - lf) / (np.abs(lx) + np.abs(lq) + 1)))
        tag = f"ndim={ndim} w_total={w_total} S={S} key#{ki} split={split}"
        assert cond <= 1e3, f"{tag}: condition number {cond:.3g}"
        assert e_fit <= 1e-13 and e_norm <= 1e-13, f"{tag}: fit {e_fit:.2e}, log_norm {e_norm:.2e}"
        assert e_lf <= 1e-12, f"{tag}: scaled log factor {e_lf:.2e}"
        worst = dict(cond=max(worst["cond"], cond), fit=max(worst["fit"], e_fit), norm=max(worst["norm"], e_norm), lf=max(worst["lf"], e_lf))
    print("fit cases, worst:", {k: f"{v:.3g}" for k, v in worst.items()})


def test_chunk_cases_are_well_conditioned_and_float64_can_meet_the_bar(chunk_refs):
    for (ndim, nc), r in chunk_refs.items():
        cond = float(np.linalg.cond(mr.covariance(r["comp"]).astype(np.float64)))
        got = fit_f64(r["comp"])
        e_fit = max(_rel(got[0], r["fit"][0]), _rel(got[1], r["fit"][1]))
        scale = np.abs(r["lx"]) + np.abs(r["lq"]) + 1
        e_lf = np.abs(factor_f64(r["key0"], r["ids"], r["x"], r["comp"], got).astype(LD) - r["lf"]) / scale
        print(f"ndim={ndim} nc={nc}: cond {cond:.3g}, fit {e_fit:.2e}, scaled factor {float(e_lf.max()):.2e} "
              f"(displaced rows {float(e_lf[ms.FAR].max()):.2e}, |log kde| up to {float(np.abs(r['lx']).max()):.2e})")
        assert cond <= 1e3 and e_fit <= 1e-13 and float(e_lf.max()) <= 1e-12
        assert np.all(np.isfinite(r["lf"].astype(np.float64)))
        assert float(np.abs(r["lx"][ms.FAR]).min()) > 1e5, "the displaced rows are far outside the cloud"


# ---- reach -----------------------------------------------------------------------------------------------------------------
def test_every_list_of_the_sweep_is_reached(chunk_refs):
    assert {d for d, _, _ in ms.FIT_CASES} == set(range(1, 17))
    assert {(d, w) for d, w, S in ms.FIT_CASES if w in (514, 600)} == {(d, w) for d in (3, 5, 7, 8, 9, 16) for w in (514, 600)}
    assert {(d, w, S) for d, w, S in ms.FIT_CASES if S == 3} == {(8, 100, 3), (9, 100, 3)}
    pc = ms.propose_cases()
    assert {d for d, _, _ in pc} == set(ms.PROPOSE_NDIM) and {w for _, w, _ in pc} == set(ms.PROPOSE_W)
    assert {(w, S) for _, w, S in pc} == {(w, S) for w in ms.PROPOSE_W for S in (2, 3)} - {(4, 3)}
    cases = [ms.ns_case(s) for s in range(ms.NS_DEFAULT)]
    assert {c["ndim"] for c in cases} == set(ms.NS_NDIM) and {c["n_surv"] for c in cases} == set(ms.NS_SURV)
    assert {c["m"] for c in cases} == set(ms.NS_M) and {c["prior_kind"] for c in cases} == set(ms.NS_PRIOR)
    assert {c["gs"] for c in cases} == set(ms.NS_GS)
    # every case with more than one chunk: the maximum of the log-sum-exp in a later chunk and in the first, ten rows each
    # (a row is a point at which the density is taken: the 96 walkers and their 96 proposals)
    for (ndim, nc), r in chunk_refs.items():
        e = np.concatenate([r["ex"], r["eq"]])
        first = e[:, :ms.CHUNK].max(axis=1)
        if nc <= ms.CHUNK:
            continue
        later = e[:, ms.CHUNK:].max(axis=1)
        n_later, n_first = int((later > first).sum()), int((first > later).sum())
        gap = (later - first)[later > first]
        print(f"ndim={ndim} nc={nc}: maximum in a later chunk {n_later} rows (first-chunk maximum {float(gap.min()):.1f} .. "
              f"{float(gap.max()):.3g} below it), in the first chunk {n_first} rows")
        assert n_later >= 10 and n_first >= 10
        if nc > 2 * ms.CHUNK:  # three chunks: the last holds 4 centres (three of the four waves idle) and some row's maximum
            assert nc - 2 * ms.CHUNK <= 64
        if nc == ms.CHUNK + 1:
            assert int(np.argmax(r["ex"][ms.N_IDS // 2])) == ms.CHUNK, "the walker next to the lone last row"


# ---- sharpness ---------------------------------------------------------------------------------------------------------------
def test_the_bars_see_a_dropped_centre_an_omitted_rescale_and_the_wrong_divisor(pkg, chunk_refs):
    near = np.setdiff1d(np.arange(ms.N_IDS), ms.FAR)
    for ndim, nc in [(9, 4100), (2, 4100)]:
        r = chunk_refs[ndim, nc]
        scale = (np.abs(r["lx"]) + np.abs(r["lq"]) + 1)[near]
        # the centre a proposal was drawn from, dropped from the sum of that proposal's density
        j = mr.partner(r["key0"], 0, r["ids"], nc)
        eq = r["eq"].copy()
        eq[np.arange(ms.N_IDS), j] = -np.inf
        moved = np.abs(mr.logsumexp(eq) - mr.logsumexp(r["eq"]))[near] / scale
        print(f"ndim={ndim} nc={nc}: one dropped centre moves the scaled factor by {float(moved.min()):.2e} .. {float(moved.max()):.2e}")
        assert float(moved.min()) > 1000 * KDE_BAR
    # sa * exp(mxa - na) without the factor: every row whose maximum lies in a later chunk keeps the whole first-chunk sum at
    # full weight.  The shift is ln(1 + sum_1 / sum_later) with both sums relative to their own maxima, so it is bounded by
    # ln(1 + 2048) = 7.6 in absolute terms; what the test needs is that it is far above the bar in the bar's own scale.
    for (ndim, nc), r in chunk_refs.items():
        if nc <= ms.CHUNK:
            continue
        got = fit_f64(r["comp"])
        good = factor_f64(r["key0"], r["ids"], r["x"], r["comp"], got)
        bad = factor_f64(r["key0"], r["ids"], r["x"], r["comp"], got, rescale=False)
        scale = (np.abs(r["lx"]) + np.abs(r["lq"]) + 1).astype(np.float64)
        moved = np.abs(bad - good) / scale
        later = (r["ex"][:, ms.CHUNK:].max(axis=1) > r["ex"][:, :ms.CHUNK].max(axis=1) + 10) | \
                (r["eq"][:, ms.CHUNK:].max(axis=1) > r["eq"][:, :ms.CHUNK].max(axis=1) + 10)
        later[ms.FAR] = False
        print(f"ndim={ndim} nc={nc}: no rescale moves {int(later.sum())} near rows by {float(moved[later].min()):.2e} .. "
              f"{float(moved[later].max()):.2e} scaled ({float(np.abs(bad - good)[later].max()):.2f} absolute at most); displaced rows "
              f"{float(moved[ms.FAR].max()):.2e}")
        assert int(later.sum()) >= 10 and float(moved[later].min()) > 1000 * KDE_BAR
    # nc in place of nc - 1 in the covariance
    least = math.inf
    for ndim, w_total, S, ki, split_key, split, pos in _fit_runs(pkg):
        if ki or split:
            continue
        comp = pos[mr.comp_ids(split_key, S, split, w_total)]
        good, bad = mr.kde_fit(comp), mr.kde_fit(comp, ddof=0)
        least = min(least, _rel(bad[0], good[0]), _rel(bad[1], good[1]))
    print(f"nc for nc - 1 moves chol and chol_inv_t by at least {least:.2e} of their largest element")
    assert least > 1e6 * FIT_BAR


def test_nested_proposal_bound_holds_for_float64_and_sees_defects():
    worst, least = 0.0, math.inf
    for seed in range(ms.NS_DEFAULT):
        c = ms.ns_case(seed)
        if c["n_surv"] < 2:
            c = ms.ns_case(seed, n_surv=2)
        want, bound = ms.ns_propose_ld(c["key"], c["gamma"], c["sigma"], c["su"], c["wu"])
        got = ms.ns_propose_f64(c["key"], c["gamma"], c["sigma"], c["su"], c["wu"])
        frac = float(np.max(np.abs(got.astype(LD) - want) / bound))
        worst = max(worst, frac)
        # a worst case over five operations is nearly reached when their roundings align (0.42 in seed 14): the restatement
        # has a factor 2 to spare, not the factor 5 that the bounds of sums over hundreds of terms leave (tests/chain_shapes.py)
        assert frac <= 0.5, f"seed {seed}: the float64 restatement is at {frac:.3f} of the bound"
        defects = []
        if c["gamma"] != 0.0:
            defects.append(ms.ns_propose_ld(c["key"], c["gamma"], c["sigma"], c["su"], c["wu"], drop="de")[0])
            if c["n_surv"] > 2:
                defects.append(ms.ns_propose_ld(c["key"], c["gamma"], c["sigma"], c["su"], c["wu"], shift_b=1)[0])
        if c["sigma"] != 0.0:
            defects.append(ms.ns_propose_ld(c["key"], c["gamma"], c["sigma"], c["su"], c["wu"], drop="noise")[0])
        for bad in defects:
            miss = float(np.median(np.abs(bad - want) / bound))
            least = min(least, miss)
            assert miss > 1e6, f"seed {seed}: a defect stays at {miss:.3g} of the bound"
    print(f"nested proposal: float64 at most {worst:.3f} of the bound; a defect at least {least:.3g} times the bound (median element)")


# ---- agreement with the other statements -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim,w_total", [(4, 120), (12, 200)])
def test_the_judge_agrees_with_scipy_and_the_tensor_statement(pkg, ndim, w_total):
    import torch
    from scipy import stats
    from oracle import moves_torch

    E = pkg.ensemble
    pos = ms.cloud(300 + ndim, w_total, ndim)
    seed, step = 11, 3
    tm = moves_torch.TensorMoves(E.stream_key)
    e = types.SimpleNamespace(seed=seed, step_count=step, a=2.0, ndim=ndim, de_sigma=1e-5)
    for S in (2, 3):
        split_key = E.stream_key(seed, step, 0, E._SPLIT_STREAM)
        sp = moves_torch.split_of(split_key, S, torch.arange(w_total)).numpy()
        np.testing.assert_array_equal(mr.split_of(split_key, S, w_total), sp)
        split = S - 1
        ids, cids = mr.active_ids(split_key, S, split, w_total), mr.comp_ids(split_key, S, split, w_total)
        x, comp, key0 = pos[ids], pos[cids], E.stream_key(seed, step, split)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        y, lf, _, _ = mr.stretch(key0, ids, x, comp)
        ty, tlf = tm.propose_stretch(e, t(x), t(ids), t(comp), split)
        np.testing.assert_allclose(ty.numpy(), y.astype(np.float64), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(tlf.numpy(), lf.astype(np.float64), rtol=1e-12, atol=1e-12)
        y, _, _, _ = mr.de(key0, ids, x, comp)
        ty, _ = tm.propose_de(e, t(x), t(ids), t(comp), split)
        np.testing.assert_allclose(ty.numpy(), y.astype(np.float64), rtol=1e-12, atol=1e-12)
        fit = mr.kde_fit(comp)
        q, lf, lx, lq = mr.kde_propose(key0, ids, x, comp, fit)
        scale = (np.abs(lx) + np.abs(lq) + 1).astype(np.float64)
        ty, tlf = tm.propose_kde(e, t(x), t(ids), t(comp), split)
        np.testing.assert_allclose(ty.numpy(), q.astype(np.float64), rtol=1e-12, atol=1e-12)
        assert np.max(np.abs(tlf.numpy() - lf.astype(np.float64)) / scale) <= 1e-12
        kde = stats.gaussian_kde(comp.T, bw_method="silverman")
        cov = (fit[0] @ fit[0].T).astype(np.float64)
        assert np.max(np.abs(kde.covariance - cov)) <= 1e-12 * np.max(np.abs(cov))
        q64 = q.astype(np.float64)
        assert np.max(np.abs(kde.logpdf(x.T) - kde.logpdf(q64.T) - lf.astype(np.float64)) / scale) <= 1e-12
        assert float(np.max(np.abs(fit[1].T @ fit[0] - np.eye(ndim)))) < 1e-17 * ndim * 1e3


def test_no_stretch_draw_of_the_sweep_sits_on_z_equal_one(pkg):
    """The stretch factor (ndim - 1) ln z is compared at rtol 1e-11.  z = t^2 / a carries three roundings of float64 (the sum
    in t, the square with t's error doubled), 3 u relative, which ln z returns as 3 u / |ln z|: below 7e-12 only while
    |ln z| > 5e-5.  The draws of the sweep are fixed by their keys, so this is a property of the cases."""
    least = math.inf
    for ndim, w_total, S in ms.propose_cases():
        for ki, split_key in enumerate(ms.split_keys()):
            for split in range(S):
                ids = mr.active_ids(split_key, S, split, w_total)
                _, _, _, z = mr.stretch(pkg.ensemble.stream_key(w_total, ndim + 100 * ki, split), ids, np.zeros((ids.size, ndim)),
                                        np.zeros((w_total - ids.size, ndim)))
                least = min(least, float(np.abs(np.log(z)).min()))
    assert least > 5e-5, least


def test_accept_of_the_judge_has_ieee_semantics():
    nan, inf = math.nan, math.inf
    lf = np.array([0.0, nan, 0.0, 0.0, 0.0, 0.0, 0.0, -1e3])
    new = np.array([nan, -1.0, inf, -inf, -1.0, -inf, -2.0, -2.0])
    old = np.array([-1.0, -1.0, -1.0, -1.0, -inf, -inf, -2.0, -2.0])
    u = np.full(8, 0.5)
    np.testing.assert_array_equal(mr.accept(lf, new, old, u), [False, False, True, False, True, False, True, False])
    assert mr.accept(0.0, -1.0, -1.0, 0.0)  # log 0 = -inf is below 0
