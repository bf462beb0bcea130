"""GPU (-m gpu): cf_ens_kde_prepare / cf_ens_propose / cf_ens_accept / cf_ens_accept_record (csrc/cosmofit_ensemble.hip) called
directly on torch buffers at the shapes the C entry points accept: every kde_prepare_small<1..8> and the run-time-dimension
form (ndim 9 .. 16) at the smallest regular set and past one pass of the 256-thread loops, three splits with a cut last
triple, the log-sum-exp over one, two and three chunks of 2048 centres, stretch and DE up to ndim 16, the accept kernel on
non-finite log P.

The judge is long double (tests/moves_reference.py); tests/test_move_shapes_cpu.py shows on the CPU that the cases are well
conditioned, that a float64 restatement of either kernel form meets these bars with two orders to spare, and that a dropped
centre, an omitted rescale or nc for nc - 1 misses them by three to eight orders.  What the kernels promise exactly is
asserted exactly: zero triangles, a zero DE factor, the same bits for a walker wherever it stands in the list of active
walkers, and no write outside an output.
"""
import numpy as np
import pytest
import torch

import move_shapes as ms
import moves_reference as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LD = np.longdouble
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def lib(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg._lib, pkg.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the cases are shared and read-only


def _f64(a):
    return np.asarray(a, dtype=LD).astype(np.float64)


def _fit(lib, dpos, w_total, ndim, S, split, split_key, nc):
    """cf_ens_kde_prepare into buffers one entry / one row longer than needed: (chol, chol_inv_t, log_norm, wc, the two buffers)."""
    L, so = lib
    params = torch.full((2 * ndim * ndim + 2,), SENTINEL, dtype=torch.float64, device=DEV)
    wc = torch.full((nc + 1, ndim), SENTINEL, dtype=torch.float64, device=DEV)
    assert so.cf_ens_comp_count(split_key, S, split, w_total) == nc
    L.check(so.cf_ens_kde_prepare(dpos.data_ptr(), w_total, ndim, S, split, split_key, params.data_ptr(), wc.data_ptr(), _stream()))
    torch.cuda.synchronize()
    p = params.cpu().numpy()
    assert p[-1] == SENTINEL, "cf_ens_kde_prepare wrote past kde_params[2 d^2]"
    assert bool((wc[nc] == SENTINEL).all()), "cf_ens_kde_prepare wrote past nc rows of wc"
    return p[:ndim * ndim].reshape(ndim, ndim), p[ndim * ndim:2 * ndim * ndim].reshape(ndim, ndim), p[2 * ndim * ndim], wc[:nc].cpu().numpy(), params, wc


def _propose(lib, kind, dpos, w_total, ndim, S, split, split_key, ids, key0, params=None, wc=None, a=2.0, sigma=1e-5):
    """cf_ens_propose into buffers one row longer than n_active: (y, log factor)."""
    L, so = lib
    n = len(ids)
    dids = _dev(np.asarray(ids, dtype=np.int64))
    y = torch.full((n + 1, ndim), SENTINEL, dtype=torch.float64, device=DEV)
    lf = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    L.check(so.cf_ens_propose(kind, dpos.data_ptr(), w_total, ndim, S, split, split_key, dids.data_ptr(), n, key0, a, sigma,
                              params.data_ptr() if params is not None else None, wc.data_ptr() if wc is not None else None,
                              y.data_ptr(), lf.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert bool((y[n] == SENTINEL).all()) and float(lf[n]) == SENTINEL, "cf_ens_propose wrote past n_active rows"
    return y[:n].cpu().numpy(), lf[:n].cpu().numpy()


def _assert_matrix(got, want, what):
    want = np.asarray(want, dtype=LD)
    err = float(np.max(np.abs(got.astype(LD) - want)) / np.max(np.abs(want)))
    assert err <= 1e-11, f"{what}: {err:.2e} of the largest element"
    return err


def _check_fit(lib, pos, dpos, ndim, w_total, S, split, split_key):
    cids = mr.comp_ids(split_key, S, split, w_total)
    comp = pos[cids]
    want = mr.kde_fit(comp)
    chol, inv_t, log_norm, wc, params, dwc = _fit(lib, dpos, w_total, ndim, S, split, split_key, len(cids))
    e = max(_assert_matrix(chol, want[0], "chol"), _assert_matrix(inv_t, want[1], "chol_inv_t"),
            _assert_matrix(wc, comp.astype(LD) @ want[1], "wc"))
    e_norm = float(abs(LD(log_norm) - want[2]))
    assert e_norm <= 1e-11, f"log_norm: {e_norm:.2e}"
    assert np.all(chol[np.triu_indices(ndim, 1)] == 0.0), "the strict upper triangle of chol is exactly 0.0"
    assert np.all(inv_t[np.tril_indices(ndim, -1)] == 0.0), "the strict lower triangle of chol_inv_t (as stored) is exactly 0.0"
    return comp, want, params, dwc, e, e_norm


def _check_kde_factor(lf, want_lf, lx, lq):
    assert np.all(np.isfinite(lf)), "every KDE factor is finite"
    err = np.abs(lf.astype(LD) - want_lf) / (np.abs(lx) + np.abs(lq) + 1)
    assert float(err.max()) <= 1e-9, f"KDE factor: {float(err.max()):.2e} of |log kde(x)| + |log kde(q)| + 1"
    return float(err.max())


@pytest.mark.parametrize("ndim,w_total,S", ms.FIT_CASES)
def test_kde_fit_and_proposal_against_long_double(lib, pkg, ndim, w_total, S):
    """kde_prepare_small<ndim> for ndim <= 8, the d > 8 branch of ens_kde_prepare_kernel above; KDE proposals of every active walker."""
    assert np.finfo(LD).eps < 1e-18, "the judge must be an extended type, not float64 judging float64"
    pos = ms.fit_positions(ndim, w_total, S)
    dpos = _dev(pos)
    worst = [0.0, 0.0, 0.0]
    for ki, split_key in enumerate(ms.split_keys()):
        for split in range(S):
            comp, fit, params, dwc, e, e_norm = _check_fit(lib, pos, dpos, ndim, w_total, S, split, split_key)
            ids = mr.active_ids(split_key, S, split, w_total)
            key0 = pkg.ensemble.stream_key(w_total, ndim + 100 * ki, split)
            q, want_lf, lx, lq = mr.kde_propose(key0, ids, pos[ids], comp, fit)
            y, lf = _propose(lib, 2, dpos, w_total, ndim, S, split, split_key, ids, key0, params, dwc)
            np.testing.assert_allclose(y, _f64(q), rtol=1e-11, atol=1e-12)
            worst = [max(worst[0], e), max(worst[1], e_norm), max(worst[2], _check_kde_factor(lf, want_lf, lx, lq))]
    print(f"ndim={ndim} w_total={w_total} S={S}: fit {worst[0]:.2e}, log_norm {worst[1]:.2e}, scaled factor {worst[2]:.2e}")


@pytest.fixture(scope="module")
def chunk_refs():
    """Long-double figures of the chunk cases, computed once per case and left unchanged."""
    cache = {}

    def get(ndim, nc):
        if (ndim, nc) not in cache:
            pos, ids = ms.chunk_case(ndim, nc)
            comp, key0 = pos[1::2], 900 + nc
            fit = mr.kde_fit(comp)
            cache[ndim, nc] = (pos, ids, comp, key0, fit, mr.kde_propose(key0, ids, pos[ids], comp, fit))
        return cache[ndim, nc]
    return get


@pytest.mark.parametrize("ndim,nc", ms.CHUNK_CASES)
def test_kde_factor_across_chunks_against_long_double(lib, chunk_refs, ndim, nc):
    """ens_kde_logfactor_kernel over one (nc = 2048), two (2049: a lone row in the second) and three chunks (4100: four rows in
    the third, three of its four waves idle), the maximum in the first or in a later chunk, walkers 1e3 outside the cloud."""
    pos, ids, comp, key0, fit, (q, want_lf, lx, lq) = chunk_refs(ndim, nc)
    dpos = _dev(pos)
    _, _, params, dwc, e, e_norm = _check_fit(lib, pos, dpos, ndim, 2 * nc, 2, 0, 0)
    y, lf = _propose(lib, 2, dpos, 2 * nc, ndim, 2, 0, 0, ids, key0, params, dwc)
    np.testing.assert_allclose(y, _f64(q), rtol=1e-11, atol=1e-12)
    err = _check_kde_factor(lf, want_lf, lx, lq)
    print(f"ndim={ndim} nc={nc}: fit {e:.2e}, log_norm {e_norm:.2e}, scaled factor {err:.2e}")


@pytest.mark.parametrize("ndim,nc", [(4, 2049), (9, 4100)])
def test_a_walker_keeps_its_bits_in_any_list_of_active_walkers(lib, chunk_refs, ndim, nc):
    pos, ids, comp, key0, fit, _ = chunk_refs(ndim, nc)
    dpos = _dev(pos)
    _, _, _, _, params, dwc = _fit(lib, dpos, 2 * nc, ndim, 2, 0, 0, nc)
    y, lf = _propose(lib, 2, dpos, 2 * nc, ndim, 2, 0, 0, ids, key0, params, dwc)
    # the full active set (ascending), of which the list is a subset
    y_all, lf_all = _propose(lib, 2, dpos, 2 * nc, ndim, 2, 0, 0, 2 * np.arange(nc), key0, params, dwc)
    np.testing.assert_array_equal(y_all[ids // 2], y)
    np.testing.assert_array_equal(lf_all[ids // 2], lf)
    # another position in the list
    perm = np.random.default_rng(nc).permutation(len(ids))
    y_p, lf_p = _propose(lib, 2, dpos, 2 * nc, ndim, 2, 0, 0, ids[perm], key0, params, dwc)
    np.testing.assert_array_equal(y_p, y[perm])
    np.testing.assert_array_equal(lf_p, lf[perm])
    # after a call on a different ensemble
    other = ms.fit_positions(5, 514, 2)
    dother = _dev(other)
    _, _, _, _, p2, wc2 = _fit(lib, dother, 514, 5, 2, 1, 0, 257)
    _propose(lib, 2, dother, 514, 5, 2, 1, 0, mr.active_ids(0, 2, 1, 514), 77, p2, wc2)
    _, _, _, _, params, dwc = _fit(lib, dpos, 2 * nc, ndim, 2, 0, 0, nc)
    y_2, lf_2 = _propose(lib, 2, dpos, 2 * nc, ndim, 2, 0, 0, ids, key0, params, dwc)
    np.testing.assert_array_equal(y_2, y)
    np.testing.assert_array_equal(lf_2, lf)


@pytest.mark.parametrize("ndim", ms.PROPOSE_NDIM)
def test_stretch_and_de_proposals_against_long_double(lib, pkg, ndim):
    """ens_propose_kernel, kinds 0 and 1, at every (w_total, n_splits) of the sweep, the fixed classes and a re-drawn partition,
    every split."""
    worst = 0.0
    for d, w_total, S in ms.propose_cases():
        if d != ndim:
            continue
        pos = ms.cloud(9000 + 10 * w_total + S, w_total, ndim)
        dpos = _dev(pos)
        for ki, split_key in enumerate(ms.split_keys()):
            for split in range(S):
                ids, cids = mr.active_ids(split_key, S, split, w_total), mr.comp_ids(split_key, S, split, w_total)
                x, comp = pos[ids], pos[cids]
                key0 = pkg.ensemble.stream_key(w_total, ndim + 100 * ki, split)
                tag = f"ndim={ndim} w_total={w_total} S={S} key#{ki} split={split}"
                # stretch
                want_y, want_lf, j, z = mr.stretch(key0, ids, x, comp)
                y, lf = _propose(lib, 0, dpos, w_total, ndim, S, split, split_key, ids, key0)
                np.testing.assert_allclose(y, _f64(want_y), rtol=1e-11, atol=1e-12, err_msg=tag)
                if ndim == 1:
                    assert np.all(lf == 0.0), "the stretch factor (ndim - 1) ln z is exactly 0.0 at ndim = 1"
                else:
                    np.testing.assert_allclose(lf, _f64(want_lf), rtol=1e-11, atol=0, err_msg=tag)
                    worst = max(worst, float(np.max(np.abs(lf.astype(LD) - want_lf) / np.abs(want_lf))))
                z64 = _f64(z)[:, None, None]
                pred = comp[None, :, :] + z64 * (x[:, None, :] - comp[None, :, :])  # the proposal every partner would give
                np.testing.assert_array_equal(((pred - y[:, None, :]) ** 2).sum(axis=2).argmin(axis=1), j, err_msg=tag)
                # DE
                want_y, j, k, gamma = mr.de(key0, ids, x, comp)
                assert np.all(j != k)
                y, lf = _propose(lib, 1, dpos, w_total, ndim, S, split, split_key, ids, key0)
                np.testing.assert_allclose(y, _f64(want_y), rtol=1e-11, atol=1e-12, err_msg=tag)
                assert np.all(lf == 0.0), "the DE proposal is symmetric: its log factor is exactly 0.0"
                # the pair recovered from y by a search over all ordered pairs.  The comparison of y above, at rtol 1e-11 on
                # every row, already pins the partners (another pair moves y by a centre-to-centre distance); the search costs
                # rows x nc^2 x ndim, so it runs on the first 16 rows, or 4 where the complementary set has more than 90 walkers
                rows = np.arange(len(ids))[: 16 if len(cids) <= 90 else 4]
                diff = comp[:, None, :] - comp[None, :, :]  # [j, k] = c_j - c_k
                pred = x[rows, None, None, :] + _f64(gamma)[rows, None, None, None] * diff[None]
                res = ((pred - y[rows, None, None, :]) ** 2).sum(axis=3).reshape(len(rows), -1)
                best = res.argmin(axis=1)
                np.testing.assert_array_equal(best // len(cids), j[rows], err_msg=tag)
                np.testing.assert_array_equal(best % len(cids), k[rows], err_msg=tag)
    print(f"ndim={ndim}: stretch factor, largest relative error {worst:.2e}")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("ndim", ms.ACCEPT_NDIM)
@pytest.mark.parametrize("n_active", ms.ACCEPT_N)
def test_accept_and_accept_record_on_planted_rows(lib, n_active, ndim):
    """ens_accept_kernel: NaN / +inf / -inf log P of the proposal, a -inf old state, a NaN factor, an equal proposal; the rows
    cf_ens_accept_record writes for accepted and rejected walkers; shards that start at walker 0 and 5."""
    L, so = lib
    for start in (0, 5):
        c = ms.accept_case(n_active, ndim, start)
        n, w_local = c["n"], c["w_local"]
        ids, idx = _dev(c["ids"]), _dev(c["local_idx"])
        y, lp_new, lf = _dev(c["y"]), _dev(c["lp_new"]), _dev(c["lf"])
        x, logp = _dev(c["x"]), _dev(c["logp"])
        count = torch.full((2,), 0, dtype=torch.int64, device=DEV)
        count[0], count[1] = 1000, -7
        ex, elp, total = c["x"].copy(), c["logp"].copy(), 1000
        li = c["local_idx"]

        def expect(key0):
            acc = np.asarray(mr.accept(c["lf"], c["lp_new"], elp[li], mr.uniform(key0, 2, c["ids"])), dtype=bool)
            ex[li[acc]], elp[li[acc]] = c["y"][acc], c["lp_new"][acc]
            return acc

        def same_state():
            np.testing.assert_array_equal(_bits(x.cpu().numpy()), _bits(ex))     # rejected and inactive rows keep their bits
            np.testing.assert_array_equal(_bits(logp.cpu().numpy()), _bits(elp))
            assert int(count[0]) == total and int(count[1]) == -7

        # 1. cf_ens_accept
        key0 = 4000 + n_active
        acc = expect(key0)
        want_planted = [False, True, False, True, False, False, True, True][: c["planted"]]
        assert acc[: c["planted"]].tolist() == want_planted
        L.check(so.cf_ens_accept(ids.data_ptr(), idx.data_ptr(), n, ndim, key0, y.data_ptr(), lp_new.data_ptr(), lf.data_ptr(),
                                 x.data_ptr(), logp.data_ptr(), count.data_ptr(), _stream()))
        torch.cuda.synchronize()
        total += int(acc.sum())
        same_state()
        # 2. cf_ens_accept_record on the state the first call left: n_accepted adds up, it is not reset
        slot = torch.full((w_local + 1, ndim), SENTINEL, dtype=torch.float64, device=DEV)
        lp_slot = torch.full((w_local + 1,), SENTINEL, dtype=torch.float64, device=DEV)
        wacc0 = 100 + np.arange(w_local + 1, dtype=np.int64)
        wacc = _dev(wacc0)
        key0 += 1
        acc = expect(key0)
        L.check(so.cf_ens_accept_record(ids.data_ptr(), idx.data_ptr(), n, ndim, key0, y.data_ptr(), lp_new.data_ptr(), lf.data_ptr(),
                                        x.data_ptr(), logp.data_ptr(), count.data_ptr(), slot.data_ptr(), lp_slot.data_ptr(),
                                        wacc.data_ptr(), _stream()))
        torch.cuda.synchronize()
        total += int(acc.sum())
        same_state()
        want_slot, want_lp = np.full((w_local + 1, ndim), SENTINEL), np.full(w_local + 1, SENTINEL)
        want_slot[li], want_lp[li] = ex[li], elp[li]  # the end-of-step state of every active walker, accepted or not
        np.testing.assert_array_equal(_bits(slot.cpu().numpy()), _bits(want_slot))  # inactive rows: the sentinel
        np.testing.assert_array_equal(_bits(lp_slot.cpu().numpy()), _bits(want_lp))
        want_wacc = wacc0.copy()
        want_wacc[li] += acc
        np.testing.assert_array_equal(wacc.cpu().numpy(), want_wacc)
        # 3. no slots, counts only
        key0 += 1
        acc = expect(key0)
        L.check(so.cf_ens_accept_record(ids.data_ptr(), idx.data_ptr(), n, ndim, key0, y.data_ptr(), lp_new.data_ptr(), lf.data_ptr(),
                                        x.data_ptr(), logp.data_ptr(), count.data_ptr(), None, None, wacc.data_ptr(), _stream()))
        torch.cuda.synchronize()
        total += int(acc.sum())
        same_state()
        want_wacc[li] += acc
        np.testing.assert_array_equal(wacc.cpu().numpy(), want_wacc)
        np.testing.assert_array_equal(_bits(slot.cpu().numpy()), _bits(want_slot))


def test_kde_prepare_refuses_a_singular_set(lib, pkg):
    L, so = lib
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)
    with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*more than ndim walkers"):
        L.check(so.cf_ens_kde_prepare(buf.data_ptr(), 8, 4, 2, 0, 0, buf.data_ptr(), buf.data_ptr(), _stream()))
