"""CPU: the replica ensembles without a GPU -- the key the kernels form against ``ensemble.stream_key``, the refusals of
``cf_rep_check_args``, the batched driver (``replicas.ReplicaEnsemble``) on a tensor statement against stand-alone
``ShardedEnsemble``s replica by replica, and the two evidence estimators against long-double restatements."""
import numpy as np
import pytest
import torch

import replica_reference as rr
import replica_shapes as rs
from oracle import moves_torch


@pytest.fixture(scope="module")
def RP(pkg):
    import importlib

    return importlib.import_module(pkg.__name__ + ".replicas")


# ---- the key ----------------------------------------------------------------------------------------------------------------
def test_rep_key_is_stream_key(pkg, RP):
    lib, E = pkg.lib(), pkg.ensemble
    seeds = [0, 1, 42, 2 ** 31, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 977, 2 ** 64 - 1, -1, -12345678901234567]
    steps = [0, 1, 2, 1000003, 2 ** 31 + 5, 2 ** 40]
    for seed in seeds:
        base = RP.replica_base(seed)
        assert 0 <= base < 2 ** 64
        for step in steps:
            for split in (0, 1, 2):
                for stream in (0, 1, 2, 3, 36, 253, 254, 255):
                    assert lib.cf_rep_key(base, step, split, stream) == E.stream_key(seed, step, split, stream), (seed, step, split, stream)


# ---- the refusals -----------------------------------------------------------------------------------------------------------
def test_check_args_refuses_each_restriction_with_its_message(pkg):
    lib, L = pkg.lib(), pkg._lib

    def refuse(match, *args):
        with pytest.raises(pkg.CosmofitError, match="CF_ERR_INVALID.*" + match):
            L.check(lib.cf_rep_check_args(*args))

    #       R, w, ndim, n_splits, kind, T, has_bounds
    refuse("even number", 3, 7, 2, 2, 0, 0, 0)
    refuse("even number", 3, 2, 1, 2, 0, 0, 0)
    refuse("divisible by n_splits", 3, 8, 2, 3, 1, 0, 0)
    refuse("divisible by n_splits", 1, 152, 4, 3, 1, 0, 0)
    refuse("more than ndim walkers", 2, 8, 4, 2, 2, 0, 0)
    refuse("more than ndim walkers", 2, 32, 16, 2, 2, 0, 0)
    refuse("ndim must be in 1..16", 2, 8, 0, 2, 0, 0, 0)
    refuse("ndim must be in 1..16", 2, 64, 17, 2, 0, 0, 0)
    refuse(r"below 2\^31", 1 << 21, 1 << 10, 2, 2, 0, 0, 0)
    refuse(r"below 2\^31", 1 << 62, 4, 2, 2, 0, 0, 0)
    refuse("at least one replica", 0, 8, 2, 2, 0, 0, 0)
    refuse("n_splits must be 2 or 3", 2, 8, 2, 4, 0, 0, 0)
    refuse("kind must be", 2, 8, 2, 2, 3, 0, 0)
    refuse("multiple of the T rungs", 5, 8, 2, 2, 0, 2, 1)
    refuse("needs the box", 4, 8, 2, 2, 0, 2, 0)
    # the smallest legal shapes
    for args in ((1, 4, 1, 2, 0, 0, 0), (1, 4, 1, 2, 1, 0, 0), (1, 6, 1, 3, 1, 0, 0), (1, 4, 1, 2, 2, 0, 0), (1, 34, 16, 2, 2, 0, 0),
                 (1, 4, 16, 2, 0, 1, 1), (2, 4, 1, 2, 0, 2, 1), ((1 << 31) // 4 - 1, 4, 1, 2, 0, 0, 0)):
        L.check(lib.cf_rep_check_args(*args))


def test_constructor_refuses_before_any_launch(pkg, RP):
    f = rs.columnwise_log_prob(2)
    x = torch.from_numpy(rs.starts(2, 8, 2))
    imp = rr.TensorReplicaMoves()
    with pytest.raises(pkg.CosmofitError, match="divisible by n_splits"):
        RP.ReplicaEnsemble(f, x, moves=(("de", 1.0),), moves_impl=imp)
    RP.ReplicaEnsemble(f, x, moves=(("de", 1.0),), de_splits=2, moves_impl=imp)
    with pytest.raises(pkg.CosmofitError, match="more than ndim"):
        RP.ReplicaEnsemble(rs.columnwise_log_prob(4), torch.from_numpy(rs.starts(2, 8, 4)), moves=rs.MIXED, de_splits=2, moves_impl=imp)
    with pytest.raises(ValueError, match="one seed per replica"):
        RP.ReplicaEnsemble(f, x, seeds=[1], moves_impl=imp)
    with pytest.raises(ValueError, match="strictly ascending"):
        RP.ReplicaEnsemble(f, x, betas=[0.5, 0.5], bounds=rs.BOX, moves_impl=imp)
    with pytest.raises(ValueError, match="needs bounds"):
        RP.ReplicaEnsemble(f, x, betas=[0.0, 1.0], moves_impl=imp)
    with pytest.raises(ValueError, match="whole number of ladders"):
        RP.ReplicaEnsemble(f, x, betas=[0.0, 0.5, 1.0], bounds=rs.BOX, moves_impl=imp)
    bad = x.clone()
    bad[1, 3, 0] = 10.0  # on a face
    with pytest.raises(ValueError, match="strictly inside"):
        RP.ReplicaEnsemble(f, bad, betas=[0.0, 1.0], bounds=rs.BOX, moves_impl=imp)
    with pytest.raises(ValueError, match="finite log-likelihood"):
        RP.ReplicaEnsemble(lambda t: torch.full((t.shape[0],), -np.inf, dtype=torch.float64), x, betas=[0.0, 1.0], bounds=rs.BOX,
                           moves_impl=imp)
    with pytest.raises(RuntimeError, match="no tensor-library fallback"):
        RP.ReplicaEnsemble(f, x)


# ---- the driver against stand-alone ensembles -------------------------------------------------------------------------------
def _standalone(pkg, f, x_r, seed, moves, de_splits, schedule_seed=None):
    E = pkg.ensemble

    class Scheduled(E.ShardedEnsemble):
        """Follows the batch's schedule: the move of a step is drawn from the batch's seed, not from the ensemble's own."""

        def _pick_move(self):
            u = E.uniform01_scalar(E.stream_key(schedule_seed, self.step_count, 0, E._MOVE_STREAM), 0)
            acc = 0.0
            for name, wt in self.moves:
                acc += wt
                if u < acc:
                    return name
            return self.moves[-1][0]

    cls = E.ShardedEnsemble if schedule_seed is None else Scheduled
    return cls(f, x_r, seed=seed, moves=moves, de_splits=de_splits, moves_impl=moves_torch.TensorMoves(E.stream_key))


@pytest.mark.parametrize("name", ["stretch", "de3", "de2", "kde", "mixed"])
def test_replica_r_is_the_stand_alone_ensemble_with_its_seed(pkg, RP, name):
    moves, de_splits = rs.MOVE_SETS[name]
    R, w, ndim = 3, 12, 3
    f = rs.columnwise_log_prob(ndim)
    x = torch.from_numpy(rs.starts(R, w, ndim, seed=1))
    seeds = rs.seeds_for(R)
    ens = RP.ReplicaEnsemble(f, x, seeds=seeds, seed=77, moves=moves, de_splits=de_splits, moves_impl=rr.TensorReplicaMoves())
    ens.run_mcmc(20)
    chain, lp = ens.get_chain(), ens.get_log_prob()
    assert chain.shape == (20, R, w, ndim) and lp.shape == (20, R, w)
    if name == "mixed":
        picked = set()
        probe = RP.ReplicaEnsemble(f, x, seeds=seeds, seed=77, moves=moves, moves_impl=rr.TensorReplicaMoves())
        for s in range(20):
            probe.step_count = s
            picked.add(probe._pick_move())
        assert picked == {"kde", "de"}
    for r in range(R):
        one = _standalone(pkg, f, x[r], seeds[r], moves, de_splits, schedule_seed=77 if name == "mixed" else None)
        one.run_mcmc(20)
        assert torch.equal(one.get_chain(), chain[:, r]), (name, r)
        assert torch.equal(one.get_log_prob(), lp[:, r]), (name, r)
        assert torch.equal(ens.get_chain(replica=r), chain[:, r])
        assert int(ens._n_acc[r]) == one._n_accepted
        assert float(ens.acceptance_fraction()[r]) == pytest.approx(one.acceptance_fraction(), rel=1e-15)


def test_thinning_and_slicing_follow_the_stand_alone_ensemble(pkg, RP):
    R, w, ndim = 2, 8, 2
    f = rs.columnwise_log_prob(ndim)
    x = torch.from_numpy(rs.starts(R, w, ndim, seed=2))
    ens = RP.ReplicaEnsemble(f, x, seed=5, moves_impl=rr.TensorReplicaMoves())
    assert ens.seeds == [6, 7]
    ens.run_mcmc(4, thin_by=3).run_mcmc(3, thin_by=3)
    assert ens.iteration == 7 and ens.step_count == 21
    for r in range(R):
        one = _standalone(pkg, f, x[r], ens.seeds[r], rs.MOVE_SETS["stretch"][0], 3)
        one.run_mcmc(7, thin_by=3)
        for kw in (dict(), dict(discard=2), dict(discard=1, thin=2), dict(thin=3, flat=True)):
            assert torch.equal(ens.get_chain(replica=r, **kw), one.get_chain(**kw)), kw
            assert torch.equal(ens.get_log_prob(replica=r, **kw), one.get_log_prob(**kw)), kw
    full = ens.get_chain(discard=1, thin=2)
    assert full.shape == (3, R, w, ndim)
    assert torch.equal(ens.get_chain(discard=1, thin=2, flat=True), full.reshape(3 * R * w, ndim))
    assert torch.equal(ens.cold_chain(discard=1, thin=2), full)
    with pytest.raises(ValueError):
        ens.get_chain(replica=R)


def test_pass_replica_hands_every_row_its_replica(pkg, RP):
    R, w, ndim = 3, 8, 2
    shift = torch.tensor([0.0, 2.0, -1.0], dtype=torch.float64)
    seen = []

    def f(theta, rep):
        assert rep.dtype == torch.int32 and rep.shape == (theta.shape[0],)
        seen.append(rep.clone())
        z = theta[:, 0] - shift[rep.long()]
        return -0.5 * (z * z) - 0.5 * (theta[:, 1] * theta[:, 1])

    x = torch.from_numpy(rs.starts(R, w, ndim, seed=3))
    ens = RP.ReplicaEnsemble(f, x, seed=1, pass_replica=True, moves_impl=rr.TensorReplicaMoves())
    assert seen[0].tolist() == [r for r in range(R) for _ in range(w)]
    ens.run_mcmc(5)
    for r in range(R):
        one = _standalone(pkg, lambda t, r=r: -0.5 * ((t[:, 0] - shift[r]) * (t[:, 0] - shift[r])) - 0.5 * (t[:, 1] * t[:, 1]), x[r],
                          ens.seeds[r], rs.MOVE_SETS["stretch"][0], 3)
        one.run_mcmc(5)
        assert torch.equal(one.get_chain(), ens.get_chain(replica=r))


def test_tempered_driver_swaps_states_and_keeps_the_ladders_apart(pkg, RP):
    """The tensor statement of a tempered run: swaps exchange whole states (the multiset of (row, ll) pairs of a ladder's level-l
    walkers is only permuted by a swap round), ladders do not talk to each other, and the counters add up."""
    betas, w = [0.0, 0.1, 1.0], 8
    x = torch.from_numpy(rs.starts(6, w, 2, seed=4))
    seeds = rs.seeds_for(6)
    ens = RP.ReplicaEnsemble(rs.gaussian_ll, x, seeds=seeds, seed=3, betas=betas, bounds=rs.BOX, moves_impl=rr.TensorReplicaMoves())
    assert (ens.C, ens.T) == (2, 3) and ens.cold == [2, 5]
    ens.run_mcmc(40)
    alone = RP.ReplicaEnsemble(rs.gaussian_ll, x[3:], seeds=seeds[3:], seed=3, betas=betas, bounds=rs.BOX, moves_impl=rr.TensorReplicaMoves())
    alone.run_mcmc(40)
    assert torch.equal(alone.get_chain(), ens.get_chain()[:, 3:]) and torch.equal(alone.get_log_prob(), ens.get_log_prob()[:, 3:])
    sf = ens.swap_fraction()
    assert sf.shape == (2, 2) and bool(((sf > 0) & (sf < 1)).all())
    assert ens._swap_rounds.tolist() == [20, 20]
    assert torch.equal(ens.get_log_prob().reshape(-1), rs.gaussian_ll(ens.get_chain(flat=True)))  # ll travels with its row
    inside = (ens.get_chain(flat=True) > -10.0) & (ens.get_chain(flat=True) < 10.0)
    assert bool(inside.all())
    assert ens.cold_chain().shape == (40, 2, w, 2)


# ---- the estimators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [[0.0, 1.0], [0.0, 0.01, 0.1, 0.4, 1.0], list(rs.gauss_betas())])
def test_estimators_equal_their_long_double_restatement(RP, betas):
    rng = np.random.default_rng(len(betas))
    T, N = len(betas), 500
    ll = -3.0 + 2.0 * rng.standard_normal((T, N)) - 700.0 * (rng.random((T, N)) < 0.1)  # a tenth of the values near -700
    ll[0, :5] = [-745.0, -700.0, -690.0, 0.0, 3.0]
    ss, want = RP.stepping_stone(ll, betas), float(rr.stepping_stone_ld(ll, betas))
    assert abs(ss - want) <= 1e-12 * max(1.0, abs(want)), (ss, want)
    ti, disc = RP.thermodynamic_integration(ll, betas)
    want = float(rr.ti_ld(ll, betas))
    assert abs(ti - want) <= 1e-12 * max(1.0, abs(want)), (ti, want)
    keep = sorted(set(range(T - 1, -1, -2)) | {0})
    coarse = float(rr.ti_ld(ll[keep], np.asarray(betas)[keep]))
    assert abs(disc - abs(want - coarse)) <= 1e-12 * max(1.0, abs(want))
    if T == 2:
        assert disc == 0.0


def test_estimators_refuse_ladders_that_miss_zero_or_one(RP):
    ll = np.zeros((3, 4))
    for betas in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 0.5, 0.5]):
        with pytest.raises(ValueError):
            RP.stepping_stone(ll, betas)
        with pytest.raises(ValueError):
            RP.thermodynamic_integration(ll, betas)


def test_log_evidence_of_a_driver_run(pkg, RP):
    betas, w = [0.0, 0.05, 0.3, 1.0], 8
    x = torch.from_numpy(rs.starts(8, w, 2, seed=6))
    ens = RP.ReplicaEnsemble(rs.gaussian_ll, x, seed=3, betas=betas, bounds=rs.BOX, moves_impl=rr.TensorReplicaMoves())
    ens.run_mcmc(30)
    ll = ens.get_log_prob(discard=10)
    for method, fn in (("stepping_stone", RP.stepping_stone), ("ti", lambda a, b: RP.thermodynamic_integration(a, b)[0])):
        got = ens.log_evidence(discard=10, method=method)
        per = [fn(ll[:, c * 4:(c + 1) * 4].permute(1, 0, 2).reshape(4, -1), betas) for c in range(2)]
        assert np.array_equal(got["per_ladder"], np.array(per))
        assert got["log_z"] == pytest.approx(np.mean(per), rel=1e-15)
        assert got["log_z_err"] == pytest.approx(np.std(per, ddof=1) / np.sqrt(2), rel=1e-14)
    one = RP.ReplicaEnsemble(rs.gaussian_ll, x[:4], seed=3, betas=betas, bounds=rs.BOX, moves_impl=rr.TensorReplicaMoves())
    one.run_mcmc(12)
    assert np.isnan(one.log_evidence(method="stepping_stone")["log_z_err"])
    ti = one.log_evidence(method="ti")
    assert ti["log_z_err"] == ti["discretisation_err"] >= 0.0
    half = RP.ReplicaEnsemble(rs.gaussian_ll, x[:4], seed=3, betas=[0.1, 0.2, 0.5, 1.0], bounds=rs.BOX, moves_impl=rr.TensorReplicaMoves())
    half.run_mcmc(2)
    with pytest.raises(ValueError, match="starts at beta = 0"):
        half.log_evidence()
