"""One rank of a sharded, device-resident ensemble that RECORDS its chain with the library's fused accept kernel
(cf_ens_accept_record) and reads emcee's results back: get_chain / get_log_prob gather the full chain on every rank,
get_autocorr_time runs the chain-statistics kernels on it.

Started by tests/test_gpu_chain.py as a fresh child process per rank; 2 or 3 such ranks share the one GPU of the test box
(gloo process group, all-gathers staged through the host), as in tests/sharded_rank_worker.py.

    python tests/chain_rank_worker.py --rank R --world N --port P --walkers W --steps K --thin-by T --out f.npz
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--walkers", type=int, required=True)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--thin-by", type=int, default=1)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()

    import torch
    import torch.distributed as dist

    if a.world > 1:  # the process group first: nothing has touched the GPU yet
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port))
        dist.init_process_group("gloo", rank=a.rank, world_size=a.world)
    amd = importlib.import_module("cosmology-model-fit_amd")
    if amd.lib().cf_device_count() < 1:
        sys.exit("chain_rank_worker needs an MI355X; there is no fallback path")
    dev = torch.device("cuda:0")
    syn = amd.synthetic.pantheon_like(n_sn=300, seed=3)
    lk = amd.sn_pantheon.PantheonLikelihood(syn["z_cmb"], syn["z_hel"], syn["obs"], chol=syn["chol"])
    start = amd.synthetic.THETA_TRUE + np.array([0.02, 1.0, 0.03, 0.3]) * np.random.default_rng(1).standard_normal((a.walkers, 4))
    ens = amd.ensemble.ShardedEnsemble(lk.engine.torch_log_prob(), torch.from_numpy(start).to(dev), seed=5,
                                       moves=amd.ensemble.REFERENCE_MOVES)
    assert isinstance(ens.impl, amd.ensemble.NativeMoves), "the library's kernels must run the moves"
    ens.run_mcmc(a.steps, thin_by=a.thin_by)
    chain, logp = ens.get_chain(), ens.get_log_prob(discard=3, flat=True)
    tau = ens.get_autocorr_time(discard=2, quiet=True)
    frac = ens.walker_acceptance_fraction()
    torch.cuda.synchronize()
    if a.rank == 0:
        np.savez(a.out, chain=chain.cpu().numpy(), logp=logp.cpu().numpy(), tau=tau, frac=frac.cpu().numpy(),
                 shard=np.array([ens.start, ens.stop]), local_rows=ens._chain.shape[1])
    if a.world > 1:
        dist.barrier()
        dist.destroy_process_group()
    lk.engine.close()


if __name__ == "__main__":
    main()
