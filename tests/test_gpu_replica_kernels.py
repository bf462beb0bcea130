"""GPU (-m gpu): the kernels of the replica ensembles (csrc/cosmofit_replica.hip).

The main test is an equivalence, asserted bit for bit: replica r of a batched run IS the chain of a stand-alone
``ShardedEnsemble`` on the library's stand-alone kernels with replica r's seed and start -- positions, log P and per-walker accept
counts, for every move, at the shapes of tests/replica_shapes.py (waves that straddle replicas, more than one block, the
run-time-dimension KDE fit, the ndim = 1 edge).  What the stand-alone kernels do not have -- the inverse temperature, the box, the
swap -- is judged on planted rows against the long-double statements of tests/replica_reference.py, every row planted at least
1e-6 away from its decision boundary so that none is excused."""
import numpy as np
import pytest
import torch

import replica_reference as rr
import replica_shapes as rs
import resid_shapes as RS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def RP(pkg):
    if pkg.lib().cf_device_count() < 1:
        pytest.fail("GPU tests need an MI355X; no HIP device visible (there is no fallback path)")
    return pkg.replicas


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scheduled(pkg, schedule_seed):
    E = pkg.ensemble

    class Scheduled(E.ShardedEnsemble):
        """The move of a step drawn from the batch's seed: the stand-alone ensemble follows the batch's schedule."""

        def _pick_move(self):
            u = E.uniform01_scalar(E.stream_key(schedule_seed, self.step_count, 0, E._MOVE_STREAM), 0)
            acc = 0.0
            for name, wt in self.moves:
                acc += wt
                if u < acc:
                    return name
            return self.moves[-1][0]

    return Scheduled


def _assert_replicas_are_stand_alone(pkg, ens, f, x, seeds, moves, de_splits, n_steps, schedule_seed):
    chain, lp = ens.get_chain(), ens.get_log_prob()
    wacc = ens._walker_acc.reshape(ens.R, ens.w)
    cls = _scheduled(pkg, schedule_seed)
    for r in range(ens.R):
        one = cls(f, x[r], seed=seeds[r], moves=moves, de_splits=de_splits)
        one.run_mcmc(n_steps)
        assert torch.equal(one.get_chain(), chain[:, r]), f"replica {r}: positions"
        assert torch.equal(one.get_log_prob(), lp[:, r]), f"replica {r}: log P"
        assert torch.equal(one._walker_acc, wacc[r]), f"replica {r}: per-walker accept counts"
        assert int(ens._n_acc[r]) == one.n_accepted == int(wacc[r].sum())
    assert float(chain.std()) > 0 and int(ens._n_acc.min()) > 0  # the chains moved


# ---- 1. equivalence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rs.MOVE_SETS))
@pytest.mark.parametrize("shape", rs.SHAPES, ids=lambda s: "R%d_w%d_d%d" % s)
def test_replica_r_is_the_stand_alone_chain_bit_for_bit(pkg, RP, shape, name):
    R, w, ndim = shape
    moves, de_splits = rs.MOVE_SETS[name]
    f = rs.columnwise_log_prob(ndim)
    x = torch.from_numpy(rs.starts(R, w, ndim, seed=3)).to(DEV)
    seeds = rs.seeds_for(R)
    ens = RP.ReplicaEnsemble(f, x, seeds=seeds, seed=77, moves=moves, de_splits=de_splits)
    ens.run_mcmc(30)
    assert ens.get_chain().shape == (30, R, w, ndim)
    _assert_replicas_are_stand_alone(pkg, ens, f, x, seeds, moves, de_splits, 30, 77)


def test_equivalence_on_the_likelihood_engine(pkg, RP):
    """The same with ``engine.torch_log_prob()`` of a 65-SN engine as the callable, on the reference's move mix."""
    lk, _ = RS.sn_likelihood(pkg, 65)
    try:
        R, w, ndim = 3, 24, 4
        f = lk.engine.torch_log_prob()
        x = torch.from_numpy(RS.sn_thetas(pkg, R * w, seed=21).reshape(R, w, ndim)).to(DEV)
        seeds = rs.seeds_for(R, seed=1)
        ens = RP.ReplicaEnsemble(f, x, seeds=seeds, seed=5, moves=rs.MIXED)
        ens.run_mcmc(30)
        _assert_replicas_are_stand_alone(pkg, ens, f, x, seeds, rs.MIXED, 3, 30, 5)
    finally:
        lk.engine.close()


def test_beta_one_in_a_wide_box_changes_no_bit(pkg, RP):
    """betas=[1.0] and a box that holds the whole run: the tempered accept at beta = 1 is the untempered one to the bit."""
    R, w, ndim = 3, 24, 4
    moves, de_splits = rs.MOVE_SETS["mixed"]
    f = rs.columnwise_log_prob(ndim)
    x = torch.from_numpy(rs.starts(R, w, ndim, seed=3)).to(DEV)
    seeds = rs.seeds_for(R)
    ens = RP.ReplicaEnsemble(f, x, seeds=seeds, seed=77, moves=moves, de_splits=de_splits, betas=[1.0],
                             bounds=np.array([[-1e3, 1e3]] * ndim))
    assert (ens.C, ens.T) == (3, 1)
    ens.run_mcmc(30)
    assert float(ens.get_chain().abs().max()) < 1e3
    _assert_replicas_are_stand_alone(pkg, ens, f, x, seeds, moves, de_splits, 30, 77)


# ---- 2. accept on planted rows -------------------------------------------------------------------------------------------------
def _active_rows(E, seeds, step, R, w, S, split, randomize=True):
    """(replica, local index) of every active row i = r n_act + m, from the Python statement of the splits."""
    rows = []
    for r in range(R):
        sk = E.stream_key(seeds[r], step, 0, E._SPLIT_STREAM) if randomize else 0
        for m in range(w // S):
            rows.append((r, S * m + E.split_perm(sk, S, m).index(split)))
    return rows


@pytest.mark.parametrize("R,w,ndim,S,split", [(3, 6, 1, 3, 2), (5, 150, 4, 2, 1), (3, 24, 9, 3, 0), (3, 24, 4, 2, 0)])
def test_accept_on_planted_rows(pkg, RP, R, w, ndim, S, split):
    E, L, so = pkg.ensemble, pkg._lib, pkg.lib()
    step, seeds = 1000003, rs.seeds_for(R, seed=2)
    betas_r = np.array([(0.0, 0.3, 1.0)[r % 3] for r in range(R)])
    rows = _active_rows(E, seeds, step, R, w, S, split)
    n = len(rows)
    assert n == R * (w // S)
    rng = np.random.default_rng(n)
    lo, hi = np.full(ndim, -2.0), np.full(ndim, 3.0)
    x0 = rng.uniform(-1.5, 2.5, (R, w, ndim))
    l0 = -3.0 + rng.standard_normal((R, w))
    y = rng.uniform(-1.5, 2.5, (n, ndim))
    l_new = -3.0 + rng.standard_normal(n)
    lf = 0.3 * rng.standard_normal(n)
    # planted rows: (row, what) -- spread over the replicas so that each kind meets beta 0, 0.3 or 1
    per = w // S
    plant = {}
    if per >= 8:
        r0 = [r * per for r in range(R)]
        l_new[r0[0] + 0] = -np.inf                      # beta 0: 0 * -inf is NaN, rejected
        l_new[r0[1] + 0] = -np.inf                      # beta 0.3: -inf, rejected
        l_new[r0[2] + 0] = np.nan                       # NaN, rejected
        y[r0[0] + 1, 0] = lo[0]                         # on a face
        y[r0[1] + 1, ndim - 1] = hi[ndim - 1]
        y[r0[2] + 1, 0] = np.nextafter(hi[0], np.inf)   # one ulp outside
        y[r0[0] + 2, 0] = np.nextafter(lo[0], -np.inf)
        for k in (0, 1, 2):
            lf[r0[k] + 1], lf[r0[k] + 2] = 50.0, 50.0   # log_q alone would accept them
        y[r0[1] + 3, 0] = np.nextafter(lo[0], np.inf)   # one ulp inside: log_q decides
        lf[r0[1] + 3] = 50.0
        y[r0[2] + 3, ndim - 1] = np.nextafter(hi[ndim - 1], -np.inf)
        lf[r0[2] + 3] = -50.0
        lf[r0[0] + 4] = np.nan                          # a NaN factor
        plant = {"rejected": [r0[0], r0[1], r0[2], r0[0] + 1, r0[1] + 1, r0[2] + 1, r0[0] + 2, r0[2] + 3, r0[0] + 4],
                 "accepted": [r0[1] + 3]}
    lf[n - 2], lf[n - 1] = 50.0, -50.0                  # at every shape one sure accept and one sure reject
    ids = np.array([l for _, l in rows], dtype=np.int64)
    rep = np.array([r for r, _ in rows])
    keys = [E.stream_key(seeds[r], step, split, 0) for r in range(R)]

    def decide():
        acc, margin = np.zeros(n, dtype=bool), np.zeros(n)
        for r in range(R):
            sel = np.where(rep == r)[0]
            a, m = rr.accept_decisions(keys[r], ids[sel], lf[sel], l_new[sel], l0[r, ids[sel]], betas_r[rep[sel]], y[sel], lo, hi)
            acc[sel], margin[sel] = a, m
        return acc, margin

    acc, margin = decide()
    close = np.isfinite(margin) & (np.abs(margin) < 1e-6)
    lf[close] += 1.0  # no row is excused: move the close ones away from their boundary
    acc, margin = decide()
    assert np.all(~np.isfinite(margin) | (np.abs(margin) >= 1e-6))
    assert 0 < acc.sum() < n
    for i in plant.get("rejected", []):
        assert not acc[i], i
    for i in plant.get("accepted", []):
        assert acc[i], i

    base = _dev(np.array([RP.replica_base(s) for s in seeds], dtype=np.uint64).view(np.int64))
    for tempered in (True, False):
        dx, dl = _dev(x0), _dev(l0)
        dy, dln, dlf = _dev(y), _dev(l_new), _dev(lf)
        dbeta, dlo, dhi = _dev(betas_r), _dev(lo), _dev(hi)
        n_acc0 = 1000 + np.arange(R + 1, dtype=np.int64)
        dn = _dev(n_acc0)
        slot = torch.full((R * w + 1, ndim), SENTINEL, dtype=torch.float64, device=DEV)
        l_slot = torch.full((R * w + 1,), SENTINEL, dtype=torch.float64, device=DEV)
        wacc0 = 100 + np.arange(R * w + 1, dtype=np.int64)
        dw = _dev(wacc0)
        if tempered:
            want = acc
        else:  # no beta, no box: the stand-alone accept on the same rows
            want = np.zeros(n, dtype=bool)
            for r in range(R):
                sel = np.where(rep == r)[0]
                want[sel], m = rr.accept_decisions(keys[r], ids[sel], lf[sel], l_new[sel], l0[r, ids[sel]], np.ones(len(sel)))
                assert np.all(~np.isfinite(m) | (np.abs(m) >= 1e-7))
        L.check(so.cf_rep_accept_record(dy.data_ptr(), dln.data_ptr(), dlf.data_ptr(), R, w, ndim, S, split, base.data_ptr(), step, 1,
                                        dbeta.data_ptr() if tempered else None, dlo.data_ptr() if tempered else None,
                                        dhi.data_ptr() if tempered else None, dx.data_ptr(), dl.data_ptr(), dn.data_ptr(),
                                        slot.data_ptr(), l_slot.data_ptr(), dw.data_ptr(), _stream()))
        torch.cuda.synchronize()
        ex, el = x0.copy(), l0.copy()
        ex[rep[want], ids[want]], el[rep[want], ids[want]] = y[want], l_new[want]
        np.testing.assert_array_equal(_bits(dx.cpu().numpy()), _bits(ex))  # rejected and inactive rows keep their bits
        np.testing.assert_array_equal(_bits(dl.cpu().numpy()), _bits(el))
        want_n = n_acc0.copy()
        want_n[:R] += np.bincount(rep[want], minlength=R)
        np.testing.assert_array_equal(dn.cpu().numpy(), want_n)
        g = rep * w + ids
        want_slot, want_ls = np.full((R * w + 1, ndim), SENTINEL), np.full(R * w + 1, SENTINEL)
        want_slot[g], want_ls[g] = ex[rep, ids], el[rep, ids]
        np.testing.assert_array_equal(_bits(slot.cpu().numpy()), _bits(want_slot))  # inactive rows: the sentinel
        np.testing.assert_array_equal(_bits(l_slot.cpu().numpy()), _bits(want_ls))
        want_w = wacc0.copy()
        want_w[g] += want
        np.testing.assert_array_equal(dw.cpu().numpy(), want_w)


# ---- 3. swap on planted rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("C,T,w", [(1, 2, 6), (3, 2, 6), (1, 3, 24), (3, 3, 6), (1, 8, 6), (3, 8, 70)])
def test_swap_on_planted_rows(pkg, RP, C, T, w, parity):
    L, so = pkg._lib, pkg.lib()
    ndim, step, R = 3, 17 + parity, C * T
    seeds = rs.seeds_for(R, seed=3)
    betas = np.linspace(0.0, 1.0, T) ** 2 if T > 2 else np.array([0.2, 1.0])
    rng = np.random.default_rng(100 * C + 10 * T + parity)
    x0 = rng.standard_normal((R, w, ndim))
    ll = -2.0 + 3.0 * rng.standard_normal((R, w))
    ll[0, 1] = np.nan   # a NaN difference never swaps (rung 0 pairs with rung 1 at parity 0)
    ll[R - 1, 2] = np.nan
    sw, margin = rr.swap_decisions(seeds, step, parity, C, T, w, betas, ll)
    close = np.isfinite(margin) & (np.abs(margin) < 1e-6)
    for c, t, l in zip(*np.where(close)):
        ll[c * T + t + 1, l] += 1.0
    sw, margin = rr.swap_decisions(seeds, step, parity, C, T, w, betas, ll)
    assert np.all(~np.isfinite(margin) | (np.abs(margin) >= 1e-6))
    n_pairs = (T - parity) // 2
    if n_pairs:
        assert 0 < sw.sum() < C * n_pairs * w
        if parity == 0:
            assert not sw[0, 0, 1]
    dx, dl = _dev(x0), _dev(ll)
    count0 = 500 + np.arange(C * (T - 1) + 1, dtype=np.int64)
    dc = _dev(count0)
    base = _dev(np.array([RP.replica_base(s) for s in seeds], dtype=np.uint64).view(np.int64))
    L.check(so.cf_rep_swap(dx.data_ptr(), dl.data_ptr(), C, T, w, ndim, _dev(np.tile(betas, C)).data_ptr(), base.data_ptr(), step, parity,
                           dc.data_ptr(), _stream()))
    torch.cuda.synchronize()
    ex, el, want_c = x0.copy(), ll.copy(), count0.copy()
    for c in range(C):
        for t in range(parity, T - 1, 2):
            m, ra = sw[c, t], c * T + t
            ex[ra, m], ex[ra + 1, m] = x0[ra + 1, m], x0[ra, m]
            el[ra, m], el[ra + 1, m] = ll[ra + 1, m], ll[ra, m]
            want_c[c * (T - 1) + t] += int(m.sum())
    # accepted pairs exchange exactly; rungs of the other parity and a top rung without a partner keep their bits (they equal x0)
    np.testing.assert_array_equal(_bits(dx.cpu().numpy()), _bits(ex))
    np.testing.assert_array_equal(_bits(dl.cpu().numpy()), _bits(el))
    np.testing.assert_array_equal(dc.cpu().numpy(), want_c)


# ---- 4. independence -----------------------------------------------------------------------------------------------------------
def test_a_ladder_is_the_same_alone_in_any_slot_repeated_and_on_a_second_stream(pkg, RP):
    betas, w, n = [0.0, 0.05, 0.3, 1.0], 24, 30
    x = torch.from_numpy(rs.starts(4, w, 2, seed=8)).to(DEV)
    other = torch.from_numpy(rs.starts(4, w, 2, seed=9)).to(DEV)
    seeds, filler = [21, 22, 23, 24], [31, 32, 33, 34]

    def run(pos, sd, stream=None):
        def go():
            e = RP.ReplicaEnsemble(rs.gaussian_ll, pos, seeds=sd, seed=3, betas=betas, bounds=rs.BOX, moves=rs.MIXED)
            e.run_mcmc(n)
            return e

        if stream is None:
            return go()
        stream.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(stream):
            e = go()
        stream.synchronize()
        return e

    alone = run(x, seeds)
    assert int(alone._n_swapped.sum()) > 0
    for slot in range(3):
        parts = [other, other, other]
        parts[slot] = x
        sd = filler * 3
        sd[4 * slot: 4 * slot + 4] = seeds
        three = run(torch.cat(parts), sd)
        assert torch.equal(three.get_chain()[:, 4 * slot: 4 * slot + 4], alone.get_chain()), slot
        assert torch.equal(three.get_log_prob()[:, 4 * slot: 4 * slot + 4], alone.get_log_prob()), slot
        assert torch.equal(three._n_swapped.reshape(3, 3)[slot], alone._n_swapped)
        assert torch.equal(three._n_acc[4 * slot: 4 * slot + 4], alone._n_acc)
    again = run(x, seeds)
    second = run(x, seeds, torch.cuda.Stream(DEV))
    for e in (again, second):
        assert torch.equal(e.get_chain(), alone.get_chain()) and torch.equal(e.get_log_prob(), alone.get_log_prob())
        assert torch.equal(e._n_swapped, alone._n_swapped)
