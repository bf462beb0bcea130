"""
Replica ensembles: R independent emcee-style ensembles of w walkers each, stepped together, with optional tempering.

``ensemble.ShardedEnsemble`` runs ONE ensemble, and it is only efficient when that ensemble is large; the reference's scripts run
emcee with 100-200 walkers, where the GPU is mostly idle.  A bigger ensemble is not the same thing:

  * its walkers are not independent chains, so it gives no real Gelman-Rubin R-hat (``ShardedEnsemble.gelman_rubin`` reproduces
    the reference's call, in which the steps play the "chains"); R-hat needs several ensembles from different seeds and starts;
  * a walker that starts in the wrong mode never leaves it; a temperature ladder with swaps cures that, and the same run gives
    ln Z by stepping stone and by thermodynamic integration (beside ``laplace``, ``nested`` and ``evidence.bridge``);
  * ``mocks.MockSet.log_prob(theta, mock, kind)`` takes a mock index per row: one ensemble per mock in a single run
    (``pass_replica=True``) turns posterior-level coverage into one run.

``ReplicaEnsemble`` is the primitive all three need.  Positions are [R, w, ndim]; partners are drawn only inside a walker's own
replica; replica r has the random streams of a stand-alone ``ShardedEnsemble`` with ``seed = seeds[r]`` and, with the library's
kernels (csrc/cosmofit_replica.hip: the same device code as the stand-alone kernels), IS that ensemble's chain bit for bit.  The
move of a step is common to all replicas (drawn as ``ShardedEnsemble._pick_move`` does, from the batch's own ``seed``), so every
launch is uniform: three or four launches per split update for all replicas together, no host synchronisation in the step loop.

Tempering.  ``betas`` is a strictly ascending ladder of T inverse temperatures in [0, 1]; R = C T replicas form C independent
ladders, replica r = c T + t runs at betas[t].  The callable then returns the log-LIKELIHOOD, ``bounds`` [ndim, 2] is the flat
prior (strict lo < theta < hi, as the reference's ``log_prior``) and the accept uses
``log_q = (log_factor + beta ll_new) - beta ll_old``.  At the start of step s with s % swap_every == 0, before the split updates,
walker l of rung t and walker l of rung t + 1 (t of parity (s // swap_every) % 2) exchange their states when
``log u < (beta_t - beta_{t+1}) (ll_{t+1,l} - ll_{t,l})``.

Single process, single device (sharding replicas over ranks is not done here; the likelihood handle may still be a
``devices="all"`` one).  There is no tensor-library fallback: positions on the CPU need an explicit ``moves_impl`` (the test-suite
passes a tensor statement).
"""
from __future__ import annotations

import math
from typing import Callable

import numpy as np
import torch

from ._args import stream_of
from .ensemble import _KIND, _U64, STRETCH_ONLY, ChainRecorder, _mix_int

SWAP_STREAM = 253  # the swap uniforms: stream_key(seeds[c T + t], step, 0, 253); the moves use streams 0 .. 36, 254, 255


def replica_base(seed: int) -> int:
    """What the kernels keep per replica: stream_key(seed, step, split, stream) = mix(base ^ step) + (split << 8) + stream."""
    return _mix_int(seed * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D)


def _signed64(v: int) -> int:
    return v - (1 << 64) if v >= (1 << 63) else v


# ---- evidence estimators on the untempered log-likelihoods of a ladder's rungs ----------------------------------------------
def _check_ladder(betas):
    b = np.asarray(betas, dtype=np.float64)
    if b.ndim != 1 or b.size < 2 or not np.all(np.diff(b) > 0):
        raise ValueError("a ladder needs at least two strictly ascending betas")
    if b[0] != 0.0 or b[-1] != 1.0:
        raise ValueError("ln Z needs a ladder that starts at beta = 0 (the prior) and ends at beta = 1 (the posterior)")
    return b


def stepping_stone(ll, betas) -> float:
    """ln Z = sum_t log mean_n exp((beta_{t+1} - beta_t) ll[t, n]) over rung t's samples (log-sum-exp); ll: [T, N] the untempered
    log-likelihood of the samples of every rung (the top rung's are not used)."""
    b = _check_ladder(betas)
    ll = torch.as_tensor(ll, dtype=torch.float64)
    if ll.dim() != 2 or ll.shape[0] != b.size:
        raise ValueError("stepping_stone takes ll [T, N], one row per rung")
    db = torch.as_tensor(np.diff(b), dtype=torch.float64, device=ll.device)
    terms = torch.logsumexp(db[:, None] * ll[:-1], dim=1) - math.log(ll.shape[1])
    return float(terms.sum())


def _trapezoid(mean_ll: np.ndarray, b: np.ndarray) -> float:
    return float(np.sum(np.diff(b) * 0.5 * (mean_ll[1:] + mean_ll[:-1])))


def thermodynamic_integration(ll, betas):
    """(ln Z, discretisation error): ln Z = int_0^1 <ll>_beta d beta by the trapezoid rule over the rungs; the error is the
    difference to the same rule on every other rung (counted from the top, the bottom rung kept)."""
    b = _check_ladder(betas)
    ll = torch.as_tensor(ll, dtype=torch.float64)
    if ll.dim() != 2 or ll.shape[0] != b.size:
        raise ValueError("thermodynamic_integration takes ll [T, N], one row per rung")
    m = ll.mean(dim=1).cpu().numpy()
    full = _trapezoid(m, b)
    keep = sorted(set(range(b.size - 1, -1, -2)) | {0})
    return full, abs(full - _trapezoid(m[keep], b[keep]))


class NativeReplicaMoves:
    """The library's kernels (cf_rep_*) on device-resident tensors, asynchronous on torch's current stream."""

    def __init__(self, e):
        from . import _lib as L

        self.L, self.lib = L, L.lib()  # raises if the HIP library is missing
        dev, n_max = e.x.device, e.R * (e.w // 2)
        self.y = torch.empty((n_max, e.ndim), dtype=torch.float64, device=dev)
        self.logfac = torch.empty(n_max, dtype=torch.float64, device=dev)
        self.kde_params = torch.empty(e.R * (2 * e.ndim * e.ndim + 1), dtype=torch.float64, device=dev)
        self.kde_wc = torch.empty((e.R * e.w, e.ndim), dtype=torch.float64, device=dev)
        self.base = torch.tensor([_signed64(replica_base(s)) for s in e.seeds], dtype=torch.int64, device=dev)
        self.beta = None if e.betas is None else e.beta_r.to(dev)
        self.lo = None if e.bounds is None else torch.tensor(e.bounds[:, 0].copy(), dtype=torch.float64, device=dev)
        self.hi = None if e.bounds is None else torch.tensor(e.bounds[:, 1].copy(), dtype=torch.float64, device=dev)

    def split_step(self, e, move, n_splits, split, record=None):
        L, lib = self.L, self.lib
        kind = _KIND[move]
        stream = stream_of(e.x.device)
        n = e.R * (e.w // n_splits)
        step, rnd = e.step_count & _U64, int(e.randomize_split)
        if kind == 2:
            L.check(lib.cf_rep_kde_prepare(e.x.data_ptr(), e.R, e.w, e.ndim, n_splits, split, self.base.data_ptr(), step, rnd,
                                           self.kde_params.data_ptr(), self.kde_wc.data_ptr(), stream))
        y, logfac = self.y[:n], self.logfac[:n]
        L.check(lib.cf_rep_propose(kind, e.x.data_ptr(), e.R, e.w, e.ndim, n_splits, split, self.base.data_ptr(), step, rnd,
                                   float(e.a), float(e.de_sigma), self.kde_params.data_ptr(), self.kde_wc.data_ptr(), y.data_ptr(),
                                   logfac.data_ptr(), stream))
        l_new = e._call(y, n_splits)
        slot, l_slot, counts = record if record is not None else (None, None, None)
        L.check(lib.cf_rep_accept_record(y.data_ptr(), l_new.data_ptr(), logfac.data_ptr(), e.R, e.w, e.ndim, n_splits, split,
                                         self.base.data_ptr(), step, rnd, None if self.beta is None else self.beta.data_ptr(),
                                         None if self.lo is None else self.lo.data_ptr(),
                                         None if self.hi is None else self.hi.data_ptr(), e.x.data_ptr(), e.logp.data_ptr(),
                                         e._n_acc.data_ptr(), slot, l_slot, counts, stream))

    def swap(self, e, parity):
        stream = stream_of(e.x.device)
        self.L.check(self.lib.cf_rep_swap(e.x.data_ptr(), e.logp.data_ptr(), e.C, e.T, e.w, e.ndim, self.beta.data_ptr(),
                                          self.base.data_ptr(), e.step_count & _U64, parity, e._n_swapped.data_ptr(), stream))


class ReplicaEnsemble(ChainRecorder):
    _native = NativeReplicaMoves

    def __init__(self, log_prob_fn: Callable, positions: torch.Tensor, *, seeds=None, seed: int = 42, moves=STRETCH_ONLY,
                 a: float = 2.0, de_sigma: float = 1e-5, de_splits: int = 3, randomize_split: bool = True, betas=None, bounds=None,
                 swap_every: int = 1, pass_replica: bool = False, moves_impl=None):
        """positions: [R, w, ndim] float64 starts, replica-major.
        seeds: one per replica (default seed + 1 + r): replica r is the chain of ``ShardedEnsemble(..., seed=seeds[r])``.
        seed: the batch's own seed, which draws the move of every step (common to all replicas).
        moves, a, de_sigma, de_splits, randomize_split: as ``ShardedEnsemble``.  w must be even and divisible by the number of
            splits of every configured move (by 3 when DE runs with de_splits=3; de_splits=2 serves the other sizes), and
            w // 2 > ndim when KDE is configured.
        betas: None, or a strictly ascending ladder of T inverse temperatures in [0, 1]; R = C T, replica r = c T + t runs at
            betas[t].  The callable then returns the log-likelihood and ``bounds`` [ndim, 2] (required) is the flat prior.
        bounds: [ndim, 2]; a proposal on or outside a face is never accepted.  Without betas it is optional (a box on top of the
            callable's own log P).
        swap_every: swaps between neighbouring rungs at the start of every swap_every-th step (T > 1).
        pass_replica: call ``log_prob_fn(theta [n, ndim], replica [n] int32)`` (the hook for ``mocks.MockSet.log_prob``).
        moves_impl: None = the library's kernels (positions must live on a GPU); tests pass a tensor statement."""
        self._set_moves(moves, de_splits)
        if positions.dim() != 3 or positions.dtype != torch.float64:
            raise ValueError("positions must be [R, w, ndim] float64")
        self.R, self.w, self.ndim = (int(v) for v in positions.shape)
        self.a, self.de_sigma, self.randomize_split = a, de_sigma, bool(randomize_split)
        self.seed, self.step_count = int(seed), 0
        self.seeds = [int(seed) + 1 + r for r in range(self.R)] if seeds is None else [int(s) for s in seeds]
        if len(self.seeds) != self.R:
            raise ValueError(f"seeds must hold one seed per replica ({self.R})")
        self.swap_every = int(swap_every)
        if self.swap_every < 1:
            raise ValueError("swap_every must be >= 1")
        self.pass_replica, self.log_prob_fn = bool(pass_replica), log_prob_fn
        self.bounds = None
        if bounds is not None:
            self.bounds = np.array(bounds, dtype=np.float64)
            if self.bounds.shape != (self.ndim, 2) or not np.all(self.bounds[:, 0] < self.bounds[:, 1]):
                raise ValueError(f"bounds must be [{self.ndim}, 2] with lo < hi per parameter")
        self.betas, self.T, self.C = None, 1, self.R
        if betas is not None:
            b = np.array(betas, dtype=np.float64)
            if b.ndim != 1 or b.size < 1 or not np.all(np.diff(b) > 0) or b[0] < 0.0 or b[-1] > 1.0:
                raise ValueError("betas must be a strictly ascending list of inverse temperatures in [0, 1]")
            if self.bounds is None:
                raise ValueError("a tempered run needs bounds [ndim, 2]: the box of its flat prior")
            if self.R % b.size:
                raise ValueError(f"R = {self.R} replicas are not a whole number of ladders of T = {b.size} rungs")
            self.betas, self.T, self.C = b, int(b.size), self.R // int(b.size)
            self.beta_r = torch.tensor(np.tile(b, self.C), dtype=torch.float64)
        # the refusals of the library (a host function: no device needed), once per configured move
        from . import _lib as L

        for m, _ in self.moves:
            L.check(L.lib().cf_rep_check_args(self.R, self.w, self.ndim, self._splits_of(m), _KIND[m],
                                              0 if self.betas is None else self.T, int(self.bounds is not None)))
        self.x = positions.clone().contiguous()
        dev = self.x.device
        self._rep_idx = {}
        self.logp = self._call(self.x.reshape(self.R * self.w, self.ndim), 1).clone()
        if self.betas is not None:
            lo = torch.as_tensor(self.bounds[:, 0], device=dev)
            hi = torch.as_tensor(self.bounds[:, 1], device=dev)
            if not bool(torch.isfinite(self.logp).all()):
                raise ValueError("a tempered run needs a finite log-likelihood at every start")
            if not bool(((self.x > lo) & (self.x < hi)).all()):
                raise ValueError("a tempered run needs every start strictly inside the box")
        self._n_acc = torch.zeros(self.R, dtype=torch.int64, device=dev)
        self._n_swapped = torch.zeros(self.C * max(self.T - 1, 1), dtype=torch.int64, device=dev)
        self._swap_rounds = np.zeros(max(self.T - 1, 1), dtype=np.int64)
        self._n_steps = 0
        self._new_record((self.R, self.w), torch.float64)  # the chain is [n, R, w, ndim]: the layout of an emcee chain of R w walkers
        if moves_impl is None:
            if not self.x.is_cuda:
                raise RuntimeError("ReplicaEnsemble runs its moves in the library's HIP kernels: the positions must be on an "
                                   "MI355X (there is no tensor-library fallback; tests pass a tensor statement as moves_impl)")
            moves_impl = NativeReplicaMoves(self)
        self.impl = moves_impl

    # ---- plumbing ---------------------------------------------------------------------------------------------------
    def _call(self, theta: torch.Tensor, n_splits: int) -> torch.Tensor:
        """The callable on the rows of every replica (replica-major, the same number per replica)."""
        if not self.pass_replica:
            return self.log_prob_fn(theta)
        per = theta.shape[0] // self.R
        idx = self._rep_idx.get(per)
        if idx is None:
            idx = torch.arange(self.R, dtype=torch.int32, device=theta.device).repeat_interleave(per)
            self._rep_idx[per] = idx
        return self.log_prob_fn(theta, idx)

    @property
    def cold(self):
        """Indices of the replicas that sample the posterior: all of them without a ladder, the beta = 1 rung of each ladder
        with one."""
        if self.betas is None:
            return list(range(self.R))
        if self.betas[-1] != 1.0:
            raise ValueError("this ladder has no beta = 1 rung")
        return [c * self.T + self.T - 1 for c in range(self.C)]

    # ---- stepping ---------------------------------------------------------------------------------------------------
    def step(self):
        """[swaps] then, per split: [KDE fit] -> propose -> log P -> accept, for all replicas in the same launches."""
        self._step(None)

    def _step(self, record):
        s = self.step_count
        if self.T > 1 and s % self.swap_every == 0:
            parity = (s // self.swap_every) % 2
            self.impl.swap(self, parity)
            self._swap_rounds[parity: self.T - 1: 2] += 1
        move = self._pick_move()
        n_splits = self._splits_of(move)
        for split in range(n_splits):
            if record is None:
                self.impl.split_step(self, move, n_splits, split)
            else:
                self.impl.split_step(self, move, n_splits, split, record=record)
        self.step_count += 1
        self._n_steps += 1

    # ---- results ----------------------------------------------------------------------------------------------------
    def _stored(self, v: torch.Tensor, discard: int, thin: int, flat: bool, replica) -> torch.Tensor:
        v = self._stored_steps(v, discard, thin)
        if replica is not None:
            if not 0 <= int(replica) < self.R:
                raise ValueError(f"replica must be in 0..{self.R - 1}")
            v = v[:, int(replica)].contiguous()
            return v.reshape((v.shape[0] * v.shape[1],) + tuple(v.shape[2:])) if flat else v
        v = v.contiguous()
        return v.reshape((v.shape[0] * self.R * self.w,) + tuple(v.shape[3:])) if flat else v

    def get_chain(self, discard: int = 0, thin: int = 1, flat: bool = False, replica=None) -> torch.Tensor:
        """Stored positions [discard + thin - 1 :: thin] as [n, R, w, ndim] (flat: [n R w, ndim], step-major); replica=r: that
        replica's chain [n, w, ndim] (flat: [n w, ndim]), what a stand-alone ensemble's ``get_chain`` returns."""
        return self._stored(self._chain, discard, thin, flat, replica)

    def get_log_prob(self, discard: int = 0, thin: int = 1, flat: bool = False, replica=None) -> torch.Tensor:
        """The stored value of the callable, [n, R, w] (flat: [n R w]; replica=r: [n, w]).  With ``betas`` this is the
        UNTEMPERED log-likelihood of every rung's samples (not beta times it, and without the flat prior's constant)."""
        return self._stored(self._chain_logp, discard, thin, flat, replica)

    def acceptance_fraction(self) -> torch.Tensor:
        """Accepted / proposed moves per replica, [R] float64 on the ensemble's device."""
        return self._n_acc.to(torch.float64) / max(self._n_steps * self.w, 1)

    def walker_acceptance_fraction(self) -> torch.Tensor:
        """Per-slot accepted / steps made under run_mcmc, [R, w] float64 (emcee's ``sampler.acceptance_fraction`` per replica;
        a slot of a ladder follows the row, not the state a swap moved)."""
        if not isinstance(self.impl, NativeReplicaMoves):
            raise NotImplementedError("per-walker accept counts come from the library's accept kernel; this moves_impl reports none")
        if self._mcmc_steps == 0:
            raise AttributeError("you must run the sampler with run_mcmc before accessing the results")
        return self._walker_acc.reshape(self.R, self.w).to(torch.float64) / self._mcmc_steps

    def swap_fraction(self) -> torch.Tensor:
        """Accepted / proposed swaps per (ladder, pair of neighbouring rungs), [C, T - 1] float64."""
        if self.T < 2:
            raise AttributeError("swaps need a ladder of at least two rungs")
        prop = torch.as_tensor(np.maximum(self._swap_rounds * self.w, 1), dtype=torch.float64, device=self.x.device)
        return self._n_swapped.reshape(self.C, self.T - 1).to(torch.float64) / prop

    def get_autocorr_time(self, replica: int, discard: int = 0, thin: int = 1, c: float = 5, tol: float = 50, quiet: bool = False):
        """emcee's ``get_autocorr_time`` of one replica's chain."""
        from . import chain_stats

        return thin * chain_stats.integrated_time(self.get_chain(discard=discard, thin=thin, replica=replica), c=c, tol=tol, quiet=quiet)

    def cold_chain(self, discard: int = 0, thin: int = 1, flat: bool = False) -> torch.Tensor:
        """The beta = 1 replicas only, [n, M, w, ndim] (flat: [n M w, ndim]): the posterior samples ``marginals``, ``fit_report``,
        ``influence`` and ``leaveout`` take."""
        v = self.get_chain(discard=discard, thin=thin)[:, self.cold].contiguous()
        return v.reshape(-1, self.ndim) if flat else v

    def rhat(self, discard: int = 0) -> torch.Tensor:
        """Gelman-Rubin R-hat per parameter from INDEPENDENT chains: ``chain_stats.gelman_rubin`` on [M, N, ndim], M = the
        beta = 1 replicas, N = each replica's stored steps x walkers -- the orientation that function's docstring describes."""
        from . import chain_stats

        v = self.cold_chain(discard=discard)  # [n, M, w, ndim]
        n, m = v.shape[0], v.shape[1]
        return chain_stats.gelman_rubin(v.permute(1, 0, 2, 3).reshape(m, n * self.w, self.ndim).contiguous())

    def log_evidence(self, discard: int = 0, thin: int = 1, method: str = "stepping_stone") -> dict:
        """ln Z of the likelihood times the NORMALISED flat prior of the box, from the ladder: method "stepping_stone" or "ti"
        (thermodynamic integration, trapezoid rule).  Returns log_z (the mean of the C ladders' estimates), log_z_err (their
        scatter / sqrt(C); C = 1: nan for stepping stone, the every-other-rung difference for TI) and per_ladder [C]; TI also
        returns discretisation_err (the mean every-other-rung difference).  Refuses a ladder that does not run from 0 to 1."""
        if self.betas is None:
            raise ValueError("log_evidence needs a tempered run (betas=)")
        if method not in ("stepping_stone", "ti"):
            raise ValueError('method must be "stepping_stone" or "ti"')
        _check_ladder(self.betas)
        ll = self.get_log_prob(discard=discard, thin=thin)  # [n, R, w]
        n = ll.shape[0]
        ll = ll.reshape(n, self.C, self.T, self.w).permute(1, 2, 0, 3).reshape(self.C, self.T, n * self.w)
        per, disc = [], []
        for c in range(self.C):
            if method == "stepping_stone":
                per.append(stepping_stone(ll[c], self.betas))
            else:
                z, d = thermodynamic_integration(ll[c], self.betas)
                per.append(z)
                disc.append(d)
        per = np.array(per)
        err = float(np.std(per, ddof=1) / math.sqrt(self.C)) if self.C > 1 else float("nan")
        out = {"log_z": float(per.mean()), "log_z_err": err, "per_ladder": per}
        if method == "ti":
            out["discretisation_err"] = float(np.mean(disc))
            if self.C == 1:
                out["log_z_err"] = out["discretisation_err"]
        return out
