// cosmofit_ensemble.hip — proposal and accept kernels of a device-resident ensemble sampler.
//
// The reference hands its likelihood to emcee with KDEMove (30 %) + DEMove (70 %) (sn/pantheon.py:114-117) and emcee's
// default StretchMove elsewhere; with the ensemble resident in HBM the update of one split (a half, or a third for DE) is
//     all-gather of positions -> propose -> log P (cf_eval_device) -> accept,
// and the proposal / accept arithmetic is a handful of flops per walker: done with tensor-library calls it costs
// 8-20x the likelihood itself in launches and host round trips.  These kernels do it in two launches (three for KDE).
//
// Random numbers are counter-based (splitmix64 finaliser keyed by walker id, step, split and stream), bit-identical
// to cosmology-model-fit_amd/ensemble.py's uniform01 / normal01: a chain does not depend on how walkers are sharded.
// The splits of a step (two halves; three thirds for the DE move, as emcee's DEMove sets nsplits = 3): see ens_split_of (cf_ens_device.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"
#include "cf_rng.h"
// the splits (ens_split_of, ens_member_in, comp_row), the KDE fit, the log Hastings factor and the three proposals: device code
// shared with cosmofit_replica.hip
#include "cf_ens_device.h"

// host-side counts (no device needed): active walkers of split s in the shard [start, stop), size of the complementary set
static int64_t ens_count_in(uint64_t split_key, int S, int s, int64_t start, int64_t stop) {
  if (stop <= start) return 0;
  const int64_t c0 = start / S, c1 = (stop - 1) / S;
  int64_t n = c1 - c0 + 1;
  const int64_t id0 = S * c0 + ens_member_in(split_key, S, c0, s), id1 = S * c1 + ens_member_in(split_key, S, c1, s);
  if (id0 < start || id0 >= stop) --n;
  if (c1 > c0 && (id1 < start || id1 >= stop)) --n;
  return n;
}

// ---- KDE (scipy.stats.gaussian_kde, bw_method="silverman", as emcee's KDEMove uses it): ens_kde_prepare_body ------------
extern "C" __global__ void __launch_bounds__(256)
ens_kde_prepare_kernel(const double* __restrict__ all_pos, int64_t nc, int ndim, int S, int half, uint64_t split_key, double* __restrict__ params,
                       double* __restrict__ wc) {
  ens_kde_prepare_body(all_pos, nc, ndim, S, half, split_key, params, wc);
}

// log Hastings factor of the KDE move: one 256-thread WORKGROUP per active walker (ens_kde_logfactor_body)
extern "C" __global__ void __launch_bounds__(256)
ens_kde_logfactor_kernel(const double* __restrict__ all_pos, int64_t nc, int ndim, const int64_t* __restrict__ ids,
                         int64_t n_active, const double* __restrict__ kde_params, const double* __restrict__ wc,
                         const double* __restrict__ y, double* __restrict__ log_factor) {
  const int64_t i = blockIdx.x;
  ens_kde_logfactor_body(all_pos + ids[i] * ndim, nc, ndim, kde_params, wc, y + i * ndim, log_factor + i);
}

// y[i] = proposal of active walker i, log_factor[i] = log of the Hastings factor (ens_propose_row: kind 0 stretch, 1 DE, 2 KDE)
extern "C" __global__ void __launch_bounds__(256)
ens_propose_kernel(int kind, const double* __restrict__ all_pos, int64_t nc, int ndim, int S, int half, uint64_t split_key,
                   const int64_t* __restrict__ ids,
                   int64_t n_active, uint64_t key0, double a, double de_sigma, const double* __restrict__ kde_params,
                   const double* __restrict__ kde_wc, double* __restrict__ y, double* __restrict__ log_factor) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n_active) return;
  ens_propose_row(kind, all_pos, nc, ndim, S, half, split_key, ids[i], key0, a, de_sigma, kde_params, y + i * ndim, log_factor + i);
}

// accept with probability min(1, exp(log_factor + lp_new - lp_old)); NaN never accepts.
// Recording (cf_ens_accept_record; the pointers are kernel arguments, so the null checks are wave-uniform): the walker's row and
// log P after the accept go to its local slot of the chain, its accept bit to its counter.  The accept itself is the same code
// with and without recording.
extern "C" __global__ void __launch_bounds__(256)
ens_accept_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ local_idx, int64_t n_active, int ndim, uint64_t key0,
                  const double* __restrict__ y, const double* __restrict__ lp_new, const double* __restrict__ log_factor,
                  double* __restrict__ x_local, double* __restrict__ logp_local, unsigned long long* __restrict__ n_accepted,
                  double* __restrict__ chain_slot, double* __restrict__ logp_slot, long long* __restrict__ walker_accepted) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool acc = false;
  if (i < n_active) {
    const int64_t li = local_idx[i];
    const double log_q = log_factor[i] + lp_new[i] - logp_local[li];
    acc = log(ens_uniform(key0, 2, ids[i])) < log_q;
    if (acc) {
      for (int k = 0; k < ndim; ++k) x_local[li * ndim + k] = y[i * ndim + k];
      logp_local[li] = lp_new[i];
    }
    if (chain_slot) {
      for (int k = 0; k < ndim; ++k) chain_slot[li * ndim + k] = x_local[li * ndim + k];
      logp_slot[li] = logp_local[li];
    }
    if (walker_accepted) walker_accepted[li] += acc ? 1 : 0;
  }
  const unsigned long long m = __ballot(acc);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_accepted, (unsigned long long)__popcll(m));
}

// The active walkers of split s in the shard [shard_start, shard_stop): one thread per group c0 + i that touches the shard; its
// member in split s is written if the shard owns it, at position i less the first group's miss (only the first and the last
// group of a shard can be cut).  ens_count_in is the host's count of the entries written.
extern "C" __global__ void __launch_bounds__(256)
ens_active_set_kernel(uint64_t split_key, int S, int s, int64_t shard_start, int64_t shard_stop, int64_t* __restrict__ ids,
                      int64_t* __restrict__ local_idx) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t c0 = shard_start / S, c1 = (shard_stop - 1) / S;
  if (c0 + i > c1) return;
  const int64_t c = c0 + i, id = S * c + ens_member_in(split_key, S, c, s);
  if (id < shard_start || id >= shard_stop) return;
  const int64_t first = S * c0 + ens_member_in(split_key, S, c0, s);
  const int64_t pos = i - (first < shard_start ? 1 : 0);
  ids[pos] = id;
  local_idx[pos] = id - shard_start;
}

// ------------------------------------------------------------------------------------------------
static int ens_check(int64_t w_total, int32_t ndim, int32_t n_splits, int32_t split, const char* fn) {
  if (w_total < 4 || (w_total & 1)) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": the ensemble needs an even number (>= 4) of walkers");
  if (ndim < 1 || ndim > CF_ENS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": ndim must be in 1..16");
  if (n_splits != 2 && n_splits != 3) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": n_splits must be 2 or 3");
  if (split < 0 || split >= n_splits) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": split must be in 0..n_splits - 1");
  if (n_splits == 3 && w_total < 6) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": three splits need at least 6 walkers");
  return 0;
}

extern "C" int64_t cf_ens_active_count(uint64_t split_key, int32_t n_splits, int32_t split, int64_t shard_start, int64_t shard_stop) {
  if ((n_splits != 2 && n_splits != 3) || split < 0 || split >= n_splits || shard_start < 0 || shard_stop < shard_start) return -1;
  return ens_count_in(split_key, n_splits, split, shard_start, shard_stop);
}

extern "C" int64_t cf_ens_comp_count(uint64_t split_key, int32_t n_splits, int32_t split, int64_t w_total) {
  if ((n_splits != 2 && n_splits != 3) || split < 0 || split >= n_splits || w_total < 0) return -1;
  return w_total - ens_count_in(split_key, n_splits, split, 0, w_total);
}

extern "C" int cf_ens_kde_prepare(const double* d_all_pos, int64_t w_total, int32_t ndim, int32_t n_splits, int32_t split,
                                  uint64_t split_key, double* d_params, double* d_wc, void* hip_stream) {
  int rc = ens_check(w_total, ndim, n_splits, split, "cf_ens_kde_prepare");
  if (rc) return rc;
  if (!d_all_pos || !d_params || !d_wc) return cf_set_error(CF_ERR_INVALID, "cf_ens_kde_prepare: null argument");
  const int64_t nc = cf_ens_comp_count(split_key, n_splits, split, w_total);
  if (nc <= ndim)  // the covariance of nc <= ndim points is singular: NaN factors, and a chain that never moves
    return cf_set_error(CF_ERR_INVALID, "cf_ens_kde_prepare: the KDE move needs more than ndim walkers in the complementary set");
  hipLaunchKernelGGL(ens_kde_prepare_kernel, dim3(1), dim3(256), 0, (hipStream_t)hip_stream, d_all_pos, nc, (int)ndim, (int)n_splits,
                     (int)split, split_key, d_params, d_wc);
  return cf_launch_status("cf_ens_kde_prepare");
}

extern "C" int cf_ens_propose(int32_t kind, const double* d_all_pos, int64_t w_total, int32_t ndim, int32_t n_splits, int32_t split,
                              uint64_t split_key, const int64_t* d_ids, int64_t n_active, uint64_t key0, double a, double de_sigma,
                              const double* d_kde_params, const double* d_kde_wc, double* d_y, double* d_log_factor,
                              void* hip_stream) {
  int rc = ens_check(w_total, ndim, n_splits, split, "cf_ens_propose");
  if (rc) return rc;
  if (kind < 0 || kind > 2) return cf_set_error(CF_ERR_INVALID, "cf_ens_propose: kind must be 0 (stretch), 1 (DE) or 2 (KDE)");
  if (!d_all_pos || !d_ids || !d_y || !d_log_factor || (kind == 2 && (!d_kde_params || !d_kde_wc)))
    return cf_set_error(CF_ERR_INVALID, "cf_ens_propose: null argument");
  if (n_active <= 0) return CF_OK;
  const int64_t nc = cf_ens_comp_count(split_key, n_splits, split, w_total);
  hipLaunchKernelGGL(ens_propose_kernel, dim3((unsigned)((n_active + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, (int)kind,
                     d_all_pos, nc, (int)ndim, (int)n_splits, (int)split, split_key, d_ids, n_active, key0, a, de_sigma, d_kde_params,
                     d_kde_wc, d_y, d_log_factor);
  if (kind == 2)
    hipLaunchKernelGGL(ens_kde_logfactor_kernel, dim3((unsigned)n_active), dim3(256), 0, (hipStream_t)hip_stream,
                       d_all_pos, nc, (int)ndim, d_ids, n_active, d_kde_params, d_kde_wc, (const double*)d_y, d_log_factor);
  return cf_launch_status("cf_ens_propose");
}

extern "C" int cf_ens_accept(const int64_t* d_ids, const int64_t* d_local_idx, int64_t n_active, int32_t ndim, uint64_t key0,
                             const double* d_y, const double* d_lp_new, const double* d_log_factor, double* d_x_local,
                             double* d_logp_local, uint64_t* d_n_accepted, void* hip_stream) {
  if (ndim < 1 || ndim > CF_ENS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, "cf_ens_accept: ndim must be in 1..16");
  if (!d_ids || !d_local_idx || !d_y || !d_lp_new || !d_log_factor || !d_x_local || !d_logp_local || !d_n_accepted)
    return cf_set_error(CF_ERR_INVALID, "cf_ens_accept: null argument");
  if (n_active <= 0) return CF_OK;
  hipLaunchKernelGGL(ens_accept_kernel, dim3((unsigned)((n_active + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, d_ids,
                     d_local_idx, n_active, (int)ndim, key0, d_y, d_lp_new, d_log_factor, d_x_local, d_logp_local,
                     (unsigned long long*)d_n_accepted, (double*)nullptr, (double*)nullptr, (long long*)nullptr);
  return cf_launch_status("cf_ens_accept");
}

extern "C" int cf_ens_accept_record(const int64_t* d_ids, const int64_t* d_local_idx, int64_t n_active, int32_t ndim, uint64_t key0,
                                    const double* d_y, const double* d_lp_new, const double* d_log_factor, double* d_x_local,
                                    double* d_logp_local, uint64_t* d_n_accepted, double* d_chain_slot, double* d_logp_slot,
                                    int64_t* d_walker_accepted, void* hip_stream) {
  if (ndim < 1 || ndim > CF_ENS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, "cf_ens_accept_record: ndim must be in 1..16");
  if (!d_ids || !d_local_idx || !d_y || !d_lp_new || !d_log_factor || !d_x_local || !d_logp_local || !d_n_accepted)
    return cf_set_error(CF_ERR_INVALID, "cf_ens_accept_record: null argument");
  if (!d_chain_slot != !d_logp_slot)
    return cf_set_error(CF_ERR_INVALID, "cf_ens_accept_record: d_chain_slot and d_logp_slot must both be null or both be set");
  if (n_active <= 0) return CF_OK;
  hipLaunchKernelGGL(ens_accept_kernel, dim3((unsigned)((n_active + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, d_ids,
                     d_local_idx, n_active, (int)ndim, key0, d_y, d_lp_new, d_log_factor, d_x_local, d_logp_local,
                     (unsigned long long*)d_n_accepted, d_chain_slot, d_logp_slot, (long long*)d_walker_accepted);
  return cf_launch_status("cf_ens_accept_record");
}

extern "C" int cf_ens_active_set(uint64_t split_key, int32_t n_splits, int32_t split, int64_t shard_start, int64_t shard_stop,
                                 int64_t* d_ids, int64_t* d_local_idx, void* hip_stream) {
  if ((n_splits != 2 && n_splits != 3) || split < 0 || split >= n_splits)
    return cf_set_error(CF_ERR_INVALID, "cf_ens_active_set: n_splits must be 2 or 3 and split in 0..n_splits - 1");
  if (shard_start < 0 || shard_stop < shard_start) return cf_set_error(CF_ERR_INVALID, "cf_ens_active_set: bad shard range");
  if (!d_ids || !d_local_idx) return cf_set_error(CF_ERR_INVALID, "cf_ens_active_set: null argument");
  if (shard_stop == shard_start) return CF_OK;
  const int64_t n_groups = (shard_stop - 1) / n_splits - shard_start / n_splits + 1;
  hipLaunchKernelGGL(ens_active_set_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, split_key,
                     (int)n_splits, (int)split, shard_start, shard_stop, d_ids, d_local_idx);
  return cf_launch_status("cf_ens_active_set");
}
