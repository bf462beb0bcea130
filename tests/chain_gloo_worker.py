"""One rank of the CPU (gloo) rehearsal of a recorded chain: tests/test_chain_cpu.py starts 2 or 3 of these with
torch.multiprocessing.spawn.  Each rank records only its slice of the walkers; get_chain / get_log_prob gather the full
[n, W_total, ...] on every rank with one collective."""
import os

import torch
import torch.distributed as dist

from conftest import load_pkg
from oracle import moves_torch

MU = torch.tensor([0.3, -1.0, 2.0], dtype=torch.float64)
SIG = torch.tensor([0.5, 2.0, 0.1], dtype=torch.float64)


def gauss_logp(theta):
    return -0.5 * (((theta - MU) / SIG) ** 2).sum(dim=1)


def make_ensemble(W, moves):
    g = torch.Generator().manual_seed(7)
    start = MU + SIG * torch.randn(W, 3, generator=g, dtype=torch.float64)
    amd = load_pkg()
    return amd.ensemble.ShardedEnsemble(gauss_logp, start, seed=11, moves=moves,
                                        moves_impl=moves_torch.TensorMoves(amd.ensemble.stream_key))


def record(ens, nsteps, thin_by):
    ens.run_mcmc(nsteps, thin_by=thin_by)
    return {"chain": ens.get_chain(), "logp": ens.get_log_prob(), "flat": ens.get_chain(discard=2, thin=2, flat=True),
            "iteration": ens.iteration}


def worker(rank, world, port, W, nsteps, thin_by, moves, path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ens = make_ensemble(W, moves)
    out = record(ens, nsteps, thin_by)
    out["local_rows"] = ens._chain.shape[1]
    torch.save(out, f"{path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()
