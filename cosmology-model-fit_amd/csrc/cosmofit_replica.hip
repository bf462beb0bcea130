// cosmofit_replica.hip — R independent ensembles of w walkers each, stepped together by the launches of ONE split update, with
// an optional inverse temperature per ensemble and swaps between the rungs of a temperature ladder.
//
// The reference's scripts run emcee with 100-200 walkers; one such ensemble leaves the chip idle (a 75-walker likelihood call costs
// 31 us against 226 us for 4096 walkers).  Several ensembles from different seeds and starts are what a Gelman-Rubin R-hat, a
// tempered run (a ladder of beta with swaps, ln Z by stepping stone / thermodynamic integration) and one-ensemble-per-mock
// coverage runs need; here they share every launch.
//
// Layout: positions [R, w, ndim], global row id = r w + l (replica r, local walker l).  w is a multiple of n_splits, so every
// replica has exactly n_act = w / n_splits active walkers per split and nc = w - n_act complementary ones: active row
// i = r n_act + m is the member of local group m that belongs to the split (ens_member_in with the replica's split key) -- nothing
// is ragged and there is no active-set kernel.  Partners are drawn inside the walker's own replica only.
//
// Random numbers: replica r's streams are those of a stand-alone ensemble with seed = seeds[r] (ensemble.py: stream_key).  The host
// uploads base_r = mix(seeds[r] * 0x9E37..15 + 0x5851..2D) once; the kernels form key = mix(base_r ^ step) + (split << 8) + stream
// (rep_key) themselves, the counter is the LOCAL index l.  The per-element arithmetic and every reduction order are those of
// cosmofit_ensemble.hip (cf_ens_device.h: the same device functions), so replica r of a batched run is the stand-alone chain to the
// bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"
#include "cf_rng.h"
#include "cf_ens_device.h"

#define CF_REP_SPLIT_STREAM 254  // ensemble.py: _SPLIT_STREAM
#define CF_REP_SWAP_STREAM 253   // free: the moves use streams 0 .. 36, 254 and 255 are the split and the move draws

// ensemble.py's stream_key(seed, step, split, stream) from base = mix(seed * 0x9E3779B97F4A7C15 + 0x5851F42D4C957F2D)
__device__ __host__ __forceinline__ uint64_t rep_key(uint64_t base, uint64_t step, int split, int stream) {
  return ens_mix_h(base ^ step) + ((uint64_t)split << 8) + (uint64_t)stream;
}
__device__ __forceinline__ uint64_t rep_split_key(uint64_t base, uint64_t step, int randomize) {
  return randomize ? rep_key(base, step, 0, CF_REP_SPLIT_STREAM) : 0ull;
}

// One 256-thread workgroup per replica: the KDE fit of the replica's complementary set (ens_kde_prepare_body).
extern "C" __global__ void __launch_bounds__(256)
rep_kde_prepare_kernel(const double* __restrict__ pos, int w, int ndim, int S, int split, const uint64_t* __restrict__ base,
                       uint64_t step, int randomize, double* __restrict__ params, double* __restrict__ wc) {
  const int64_t r = blockIdx.x;
  const int64_t nc = w - w / S;
  ens_kde_prepare_body(pos + r * w * ndim, nc, ndim, S, split, rep_split_key(base[r], step, randomize),
                       params + r * (2 * ndim * ndim + 1), wc + r * nc * ndim);
}

// One thread per active row i = r n_act + m.
extern "C" __global__ void __launch_bounds__(256)
rep_propose_kernel(int kind, const double* __restrict__ pos, unsigned n_rows, int w, int ndim, int S, int split,
                   const uint64_t* __restrict__ base, uint64_t step, int randomize, double a, double de_sigma,
                   const double* __restrict__ params, double* __restrict__ y, double* __restrict__ log_factor) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const unsigned n_act = (unsigned)(w / S), r = i / n_act, m = i - r * n_act;
  const uint64_t b = base[r], sk = rep_split_key(b, step, randomize);
  const int64_t l = (int64_t)S * m + ens_member_in(sk, S, m, split);
  ens_propose_row(kind, pos + (int64_t)r * w * ndim, (int64_t)(w - n_act), ndim, S, split, sk, l, rep_key(b, step, split, 0), a,
                  de_sigma, params + (int64_t)r * (2 * ndim * ndim + 1), y + (int64_t)i * ndim, log_factor + i);
}

// One 256-thread workgroup per active row: the log Hastings factor of the KDE move (ens_kde_logfactor_body).  With nc = 75 of a
// 150-walker replica 181 of the 256 lanes idle in the distance pass; a one-wave form would reduce in another order (other bits).
extern "C" __global__ void __launch_bounds__(256)
rep_kde_logfactor_kernel(const double* __restrict__ pos, int w, int ndim, int S, int split, const uint64_t* __restrict__ base,
                         uint64_t step, int randomize, const double* __restrict__ params, const double* __restrict__ wc,
                         const double* __restrict__ y, double* __restrict__ log_factor) {
  const unsigned i = blockIdx.x;
  const unsigned n_act = (unsigned)(w / S), r = i / n_act, m = i - r * n_act;
  const uint64_t sk = rep_split_key(base[r], step, randomize);
  const int64_t l = (int64_t)S * m + ens_member_in(sk, S, m, split);
  const int64_t nc = w - n_act;
  ens_kde_logfactor_body(pos + ((int64_t)r * w + l) * ndim, nc, ndim, params + (int64_t)r * (2 * ndim * ndim + 1),
                         wc + (int64_t)r * nc * ndim, y + (int64_t)i * ndim, log_factor + i);
}

// adds, per distinct `slot` among the lanes of the wave that have `flag` set, the number of such lanes to counter[slot]: one
// integer atomic per (wave, slot).  Every lane of the wave must call it (lanes without work pass flag = false).
__device__ __forceinline__ void rep_count(bool flag, unsigned slot, unsigned long long* __restrict__ counter) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(flag);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const unsigned s = (unsigned)__shfl((int)slot, lead, 64);
    const unsigned long long same = __ballot(flag && slot == s);
    if (lane == lead) atomicAdd(counter + s, (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

// accept with probability min(1, exp((log_factor + beta l_new) - beta l_old)) inside the open box (lo, hi); NaN never accepts
// (0 * -inf included), a proposal on or outside a face never accepts.  beta = 1 gives cosmofit_ensemble.hip's
// log_factor + lp_new - lp_old to the bit, contracted or not: x * 1 and fma(1, x, y) round once, as x and x + y do.
// Recording as in ens_accept_kernel (null pointers are kernel arguments: wave-uniform).
extern "C" __global__ void __launch_bounds__(256)
rep_accept_kernel(const double* __restrict__ y, const double* __restrict__ l_new, const double* __restrict__ log_factor, unsigned n_rows,
                  int w, int ndim, int S, int split, const uint64_t* __restrict__ base, uint64_t step, int randomize,
                  const double* __restrict__ beta_r, const double* __restrict__ lo, const double* __restrict__ hi,
                  double* __restrict__ pos, double* __restrict__ lcur, unsigned long long* __restrict__ n_accepted,
                  double* __restrict__ chain_slot, double* __restrict__ l_slot, long long* __restrict__ walker_accepted) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool acc = false;
  unsigned r = 0;
  if (i < n_rows) {
    const unsigned n_act = (unsigned)(w / S);
    r = i / n_act;
    const unsigned m = i - r * n_act;
    const uint64_t b = base[r], sk = rep_split_key(b, step, randomize);
    const int64_t l = (int64_t)S * m + ens_member_in(sk, S, m, split);
    const int64_t row = (int64_t)r * w + l;
    const double beta = beta_r ? beta_r[r] : 1.0;
    const double* yi = y + (int64_t)i * ndim;
    const double log_q = (log_factor[i] + beta * l_new[i]) - beta * lcur[row];
    acc = log(ens_uniform(rep_key(b, step, split, 0), 2, l)) < log_q;
    if (lo) {
      bool inside = true;
      for (int k = 0; k < ndim; ++k) inside = inside && (yi[k] > lo[k]) && (yi[k] < hi[k]);
      acc = acc && inside;
    }
    if (acc) {
      for (int k = 0; k < ndim; ++k) pos[row * ndim + k] = yi[k];
      lcur[row] = l_new[i];
    }
    if (chain_slot) {
      for (int k = 0; k < ndim; ++k) chain_slot[row * ndim + k] = pos[row * ndim + k];
      l_slot[row] = lcur[row];
    }
    if (walker_accepted) walker_accepted[row] += acc ? 1 : 0;
  }
  rep_count(acc, r, n_accepted);
}

// Swaps between neighbouring rungs: one thread per (ladder c, pair k, walker l); the pair is rungs t = parity + 2 k and t + 1,
// replicas ra = c T + t and ra + 1.  Accepted when log u < (beta_t - beta_{t+1}) (l_{t+1,l} - l_{t,l}), u = the uniform of
// (stream_key(seeds[ra], step, 0, 253), counter l); a NaN difference never swaps.  An accepted pair exchanges its rows and its
// log-likelihoods exactly; every row belongs to at most one pair of a launch, so the threads touch disjoint rows.
extern "C" __global__ void __launch_bounds__(256)
rep_swap_kernel(double* __restrict__ pos, double* __restrict__ lcur, int T, int w, int ndim, int n_pairs, unsigned n_threads,
                const double* __restrict__ beta_r, const uint64_t* __restrict__ base, uint64_t step, int parity,
                unsigned long long* __restrict__ n_swapped) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool acc = false;
  unsigned slot = 0;
  if (i < n_threads) {
    const unsigned pair = i / (unsigned)w, l = i - pair * (unsigned)w;
    const unsigned c = pair / (unsigned)n_pairs, k = pair - c * (unsigned)n_pairs;
    const unsigned t = (unsigned)parity + 2u * k;
    const unsigned ra = c * (unsigned)T + t, rb = ra + 1;
    const int64_t rowa = (int64_t)ra * w + l, rowb = (int64_t)rb * w + l;
    const double la = lcur[rowa], lb = lcur[rowb];
    const double log_q = (beta_r[ra] - beta_r[rb]) * (lb - la);
    acc = log(ens_uniform(rep_key(base[ra], step, 0, CF_REP_SWAP_STREAM), 0, (int64_t)l)) < log_q;
    slot = c * (unsigned)(T - 1) + t;
    if (acc) {
      for (int d = 0; d < ndim; ++d) {
        const double xa = pos[rowa * ndim + d], xb = pos[rowb * ndim + d];
        pos[rowa * ndim + d] = xb;
        pos[rowb * ndim + d] = xa;
      }
      lcur[rowa] = lb;
      lcur[rowb] = la;
    }
  }
  rep_count(acc, slot, n_swapped);
}

// ------------------------------------------------------------------------------------------------
static int rep_check(int64_t R, int64_t w, int32_t ndim, int32_t n_splits, int32_t kind, int32_t T, int32_t has_bounds, const char* fn) {
  const std::string f(fn);
  if (R < 1) return cf_set_error(CF_ERR_INVALID, f + ": needs at least one replica");
  if (ndim < 1 || ndim > CF_ENS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, f + ": ndim must be in 1..16");
  if (n_splits != 2 && n_splits != 3) return cf_set_error(CF_ERR_INVALID, f + ": n_splits must be 2 or 3");
  if (kind < 0 || kind > 2) return cf_set_error(CF_ERR_INVALID, f + ": kind must be 0 (stretch), 1 (DE) or 2 (KDE)");
  if (w < 4 || (w & 1)) return cf_set_error(CF_ERR_INVALID, f + ": every replica needs an even number (>= 4) of walkers");
  if (w % n_splits)
    return cf_set_error(CF_ERR_INVALID, f + ": the walkers of a replica must be divisible by n_splits (every split of every replica "
                                            "has w / n_splits walkers; de_splits = 2 serves the sizes that 3 does not divide)");
  if (kind == 2 && w - w / n_splits <= ndim)
    return cf_set_error(CF_ERR_INVALID, f + ": the KDE move needs more than ndim walkers in the complementary set of a replica");
  if (R > INT64_MAX / w || R * w >= (int64_t)1 << 31) return cf_set_error(CF_ERR_INVALID, f + ": R * w must be below 2^31");
  if (T < 0) return cf_set_error(CF_ERR_INVALID, f + ": T must be 0 (no tempering) or the number of rungs of a ladder");
  if (T > 0 && R % T) return cf_set_error(CF_ERR_INVALID, f + ": R must be a multiple of the T rungs of a ladder (R = C T)");
  if (T > 0 && !has_bounds)
    return cf_set_error(CF_ERR_INVALID, f + ": a tempered run needs the box of its flat prior (bounds)");
  return CF_OK;
}

extern "C" int cf_rep_check_args(int64_t R, int64_t w, int32_t ndim, int32_t n_splits, int32_t kind, int32_t T, int32_t has_bounds) {
  return rep_check(R, w, ndim, n_splits, kind, T, has_bounds, "cf_rep_check_args");
}

extern "C" uint64_t cf_rep_key(uint64_t base, uint64_t step, int32_t split, int32_t stream) { return rep_key(base, step, split, stream); }

static int rep_split_ok(int32_t n_splits, int32_t split, const char* fn) {
  if (split < 0 || split >= n_splits) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": split must be in 0..n_splits - 1");
  return CF_OK;
}

extern "C" int cf_rep_kde_prepare(const double* d_pos, int64_t R, int64_t w, int32_t ndim, int32_t n_splits, int32_t split,
                                  const uint64_t* d_base, uint64_t step, int32_t randomize, double* d_params, double* d_wc,
                                  void* hip_stream) {
  int rc = rep_check(R, w, ndim, n_splits, 2, 0, 0, "cf_rep_kde_prepare");
  if (rc || (rc = rep_split_ok(n_splits, split, "cf_rep_kde_prepare"))) return rc;
  if (!d_pos || !d_base || !d_params || !d_wc) return cf_set_error(CF_ERR_INVALID, "cf_rep_kde_prepare: null argument");
  hipLaunchKernelGGL(rep_kde_prepare_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)hip_stream, d_pos, (int)w, (int)ndim,
                     (int)n_splits, (int)split, d_base, step, (int)randomize, d_params, d_wc);
  return cf_launch_status("cf_rep_kde_prepare");
}

extern "C" int cf_rep_propose(int32_t kind, const double* d_pos, int64_t R, int64_t w, int32_t ndim, int32_t n_splits, int32_t split,
                              const uint64_t* d_base, uint64_t step, int32_t randomize, double a, double de_sigma,
                              const double* d_params, const double* d_wc, double* d_y, double* d_log_factor, void* hip_stream) {
  int rc = rep_check(R, w, ndim, n_splits, kind, 0, 0, "cf_rep_propose");
  if (rc || (rc = rep_split_ok(n_splits, split, "cf_rep_propose"))) return rc;
  if (!d_pos || !d_base || !d_y || !d_log_factor || (kind == 2 && (!d_params || !d_wc)))
    return cf_set_error(CF_ERR_INVALID, "cf_rep_propose: null argument");
  const unsigned n_rows = (unsigned)(R * (w / n_splits));
  hipLaunchKernelGGL(rep_propose_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, (int)kind, d_pos, n_rows,
                     (int)w, (int)ndim, (int)n_splits, (int)split, d_base, step, (int)randomize, a, de_sigma, d_params, d_y, d_log_factor);
  if (kind == 2)
    hipLaunchKernelGGL(rep_kde_logfactor_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)hip_stream, d_pos, (int)w, (int)ndim,
                       (int)n_splits, (int)split, d_base, step, (int)randomize, d_params, d_wc, (const double*)d_y, d_log_factor);
  return cf_launch_status("cf_rep_propose");
}

extern "C" int cf_rep_accept_record(const double* d_y, const double* d_l_new, const double* d_log_factor, int64_t R, int64_t w,
                                    int32_t ndim, int32_t n_splits, int32_t split, const uint64_t* d_base, uint64_t step,
                                    int32_t randomize, const double* d_beta, const double* d_lo, const double* d_hi, double* d_pos,
                                    double* d_l, uint64_t* d_n_accepted, double* d_chain_slot, double* d_l_slot,
                                    int64_t* d_walker_accepted, void* hip_stream) {
  int rc = rep_check(R, w, ndim, n_splits, 0, 0, 0, "cf_rep_accept_record");
  if (rc || (rc = rep_split_ok(n_splits, split, "cf_rep_accept_record"))) return rc;
  if (!d_y || !d_l_new || !d_log_factor || !d_base || !d_pos || !d_l || !d_n_accepted)
    return cf_set_error(CF_ERR_INVALID, "cf_rep_accept_record: null argument");
  if (!d_lo != !d_hi) return cf_set_error(CF_ERR_INVALID, "cf_rep_accept_record: d_lo and d_hi must both be null or both be set");
  if (d_beta && !d_lo) return cf_set_error(CF_ERR_INVALID, "cf_rep_accept_record: a tempered run needs the box of its flat prior (bounds)");
  if (!d_chain_slot != !d_l_slot)
    return cf_set_error(CF_ERR_INVALID, "cf_rep_accept_record: d_chain_slot and d_l_slot must both be null or both be set");
  const unsigned n_rows = (unsigned)(R * (w / n_splits));
  hipLaunchKernelGGL(rep_accept_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, d_y, d_l_new, d_log_factor,
                     n_rows, (int)w, (int)ndim, (int)n_splits, (int)split, d_base, step, (int)randomize, d_beta, d_lo, d_hi, d_pos, d_l,
                     (unsigned long long*)d_n_accepted, d_chain_slot, d_l_slot, (long long*)d_walker_accepted);
  return cf_launch_status("cf_rep_accept_record");
}

extern "C" int cf_rep_swap(double* d_pos, double* d_l, int64_t C, int32_t T, int64_t w, int32_t ndim, const double* d_beta,
                           const uint64_t* d_base, uint64_t step, int32_t parity, uint64_t* d_n_swapped, void* hip_stream) {
  if (C < 1 || T < 2) return cf_set_error(CF_ERR_INVALID, "cf_rep_swap: needs C >= 1 ladders of T >= 2 rungs");
  if (w < 1 || ndim < 1 || ndim > CF_ENS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, "cf_rep_swap: w must be positive and ndim in 1..16");
  if (C > INT64_MAX / T / w || C * T * w >= (int64_t)1 << 31) return cf_set_error(CF_ERR_INVALID, "cf_rep_swap: R * w must be below 2^31");
  if (parity != 0 && parity != 1) return cf_set_error(CF_ERR_INVALID, "cf_rep_swap: parity must be 0 or 1");
  if (!d_pos || !d_l || !d_beta || !d_base || !d_n_swapped) return cf_set_error(CF_ERR_INVALID, "cf_rep_swap: null argument");
  const int n_pairs = (T - parity) / 2;  // t = parity, parity + 2, ... with t + 1 < T
  if (n_pairs == 0) return CF_OK;
  const unsigned n_threads = (unsigned)(C * n_pairs * w);
  hipLaunchKernelGGL(rep_swap_kernel, dim3((n_threads + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, d_pos, d_l, (int)T, (int)w,
                     (int)ndim, n_pairs, n_threads, d_beta, d_base, step, (int)parity, (unsigned long long*)d_n_swapped);
  return cf_launch_status("cf_rep_swap");
}
