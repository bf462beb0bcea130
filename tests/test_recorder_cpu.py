"""CPU: the chain recorder the two device-resident samplers share (``ensemble.ChainRecorder``) against the samplers as they
were while each carried its own copy of it.

``tests/golden/recorder_parent.npz`` holds what ``record`` below returned with the package of the commit before the recorder was
shared.  From a checkout of that commit, with this file copied into its ``tests/``:

    import importlib, sys
    import numpy as np
    sys.path[:0] = [".", "tests"]
    import test_recorder_cpu as t
    np.savez("tests/golden/recorder_parent.npz", **t.record(importlib.import_module("cosmology-model-fit_amd")))

Both samplers run on the tensor statements of their moves (``oracle.moves_torch.TensorMoves``,
``replica_reference.TensorReplicaMoves``) at fixed seeds with an analytic log-probability; every stored quantity must keep its
bits.  Those statements report no per-walker accept counts, so ``walker_acceptance_fraction`` stays with the GPU suite."""
import importlib

import numpy as np
import pytest
import torch

import replica_reference as rr
import replica_shapes as rs
from conftest import golden
from oracle import moves_torch

MOVES = (("kde", .3), ("de", .7))
SLICES = {"a": dict(discard=0, thin=1, flat=False), "b": dict(discard=1, thin=2, flat=True)}
BETAS = [0.0, 0.1, 1.0]


def _sharded(pkg, **kw):
    E = pkg.ensemble
    kw = {"moves": MOVES, "de_splits": 3, **kw}
    return E.ShardedEnsemble(rs.gaussian_ll, torch.from_numpy(rs.starts(1, 12, 2, seed=6)[0]), seed=11,
                             moves_impl=moves_torch.TensorMoves(E.stream_key), **kw)


def _replica(pkg, **kw):
    RP = importlib.import_module(pkg.__name__ + ".replicas")
    kw = {"moves": MOVES, "de_splits": 3, **kw}
    return RP.ReplicaEnsemble(rs.gaussian_ll, torch.from_numpy(rs.starts(6, 12, 2, seed=7)), seeds=rs.seeds_for(6), seed=13,
                              betas=BETAS, bounds=rs.BOX, swap_every=2, moves_impl=rr.TensorReplicaMoves(), **kw)


def record(pkg) -> dict:
    """Everything the fixture pins, as numpy arrays by name."""
    out = {}
    for name, ens in (("sharded", _sharded(pkg)), ("replica", _replica(pkg))):
        ens.run_mcmc(5, thin_by=2)
        ens.run_mcmc(3)  # the buffers grow with a non-empty chain in them
        out[f"{name}.iteration"] = np.array([ens.iteration, ens.step_count])
        out[f"{name}.acceptance_fraction"] = np.asarray(ens.acceptance_fraction())
        for tag, kw in SLICES.items():
            out[f"{name}.chain.{tag}"] = ens.get_chain(**kw).numpy()
            out[f"{name}.log_prob.{tag}"] = ens.get_log_prob(**kw).numpy()
            if name == "replica":
                out[f"{name}.chain.{tag}.r4"] = ens.get_chain(replica=4, **kw).numpy()
                out[f"{name}.log_prob.{tag}.r4"] = ens.get_log_prob(replica=4, **kw).numpy()
        if name == "replica":
            out[f"{name}.swap_fraction"] = ens.swap_fraction().numpy()
    return out


def test_recorded_chains_keep_the_bits_of_the_separate_recorders(pkg):
    want = golden("recorder_parent")
    got = record(pkg)
    assert set(got) == set(want.files)
    assert got["sharded.iteration"].tolist() == [8, 13] and got["replica.iteration"].tolist() == [8, 13]
    assert got["sharded.chain.a"].shape == (8, 12, 2) and got["replica.chain.a"].shape == (8, 6, 12, 2)
    assert got["replica.chain.b.r4"].shape == (3 * 12, 2) and got["replica.swap_fraction"].shape == (2, 2)
    for key in want.files:
        a, b = got[key], want[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert a.tobytes() == b.tobytes(), key


@pytest.mark.parametrize("make", [_sharded, _replica])
def test_refusals_keep_their_texts(pkg, make):
    with pytest.raises(ValueError, match=r"moves must be a non-empty sequence of \(name in \['de', 'kde', 'stretch'\], weight > 0\)"):
        make(pkg, moves=(("walk", 1.0),))
    with pytest.raises(ValueError, match=r"moves must be a non-empty sequence of \(name in \['de', 'kde', 'stretch'\], weight > 0\)"):
        make(pkg, moves=())
    with pytest.raises(ValueError, match=r"moves must be a non-empty sequence of \(name in \['de', 'kde', 'stretch'\], weight > 0\)"):
        make(pkg, moves=(("de", 0.0),), de_splits=4)  # the moves are checked first
    with pytest.raises(ValueError, match=r"de_splits must be 3 \(emcee's DEMove\) or 2"):
        make(pkg, de_splits=4)
    ens = make(pkg)
    with pytest.raises(AttributeError, match="you must run the sampler with run_mcmc before accessing the results"):
        ens.get_chain()
    with pytest.raises(AttributeError, match="you must run the sampler with run_mcmc before accessing the results"):
        ens.get_log_prob()
    with pytest.raises(ValueError, match="run_mcmc needs nsteps >= 0 and thin_by >= 1"):
        ens.run_mcmc(-1)
    with pytest.raises(ValueError, match="run_mcmc needs nsteps >= 0 and thin_by >= 1"):
        ens.run_mcmc(1, thin_by=0)
    assert ens.run_mcmc(0).iteration == 0 and ens.run_mcmc(2).iteration == 2
    with pytest.raises(ValueError, match="get_chain needs discard >= 0 and thin >= 1"):
        ens.get_chain(thin=0)
    with pytest.raises(ValueError, match="get_chain needs discard >= 0 and thin >= 1"):
        ens.get_log_prob(discard=-1)
