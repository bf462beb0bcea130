// cosmofit_opt.hip — the per-iteration kernels of a batched box-constrained maximizer (optimize.py is the driver).
//
// B independent problems maximise one objective f(theta) (any torch callable, e.g. the engine's log P) inside a box.  A
// problem lives in box-scaled coordinates u = (theta - lo) / (hi - lo), confined to [delta, 1 - delta]; only the free
// coordinates move, the fixed ones keep their start values.  One iteration is
//     stencil (this file) -> f of 2 n_free rows per problem -> direction (this file) -> f of K trial rows per problem
//     -> accept (this file) -> compact (this file),
// asynchronous on the caller's stream; the host reads one integer per iteration (the number still active).
//
// Every problem reads and writes only its own rows and state, with sums in index order and no float atomics, so a problem's
// bits do not depend on the rest of the batch.  Floating-point contraction is off in every expression that
// tests/opt_reference.py restates in numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"

#define OPT_LANES 16  // lanes per problem in the direction kernel: lane i owns free coordinate i and row i of H^-1

// the ensemble's counter-based generator (cosmofit_ensemble.hip: ens_uniform), restated with the same bits
__device__ __forceinline__ uint64_t opt_mix(uint64_t x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ double opt_uniform(uint64_t key0, int stream, int64_t id) {
  const uint64_t x = opt_mix((uint64_t)id * 0x9E3779B97F4A7C15ull + key0 + (uint64_t)stream);
  return (double)(opt_mix(x + 0x9E3779B97F4A7C15ull) >> 11) * (1.0 / 9007199254740992.0);
}

// free slot of theta index c, or -1 for a fixed coordinate
__device__ __forceinline__ int opt_slot(const cf_opt_params& p, int c) {
  int s = -1;
  for (int j = 0; j < p.n_free; ++j) s = p.free_idx[j] == c ? j : s;
  return s;
}

__device__ __forceinline__ double opt_clamp(double v, double delta) {
  return fmin(fmax(v, delta), 1.0 - delta);
}

// trial k of the line search: P(u + 4^-k d)
__device__ __forceinline__ double opt_trial(double u, double d, int k, double delta) {
#pragma clang fp contract(off)
  return opt_clamp(u + ldexp(1.0, -2 * k) * d, delta);
}

// stencil form of a coordinate at u: 0 central (u +- h), +1 forward (u + h, u + 2h), -1 backward (u - h, u - 2h)
__device__ __forceinline__ int opt_form(double u, double h, double delta) {
#pragma clang fp contract(off)
  const double h2 = 2.0 * h;
  return (u - delta) < h2 ? 1 : ((1.0 - delta) - u < h2 ? -1 : 0);
}

// one thread per element (b, c): a free coordinate from stream c at counter b (random) or from x0, a fixed one from x0;
// u clamped to [delta, 1 - delta], theta = lo + u (hi - lo)
extern "C" __global__ void __launch_bounds__(256)
opt_starts_kernel(cf_opt_params p, int64_t n, const double* __restrict__ x0, uint64_t key, int random, double* __restrict__ u,
                  double* __restrict__ theta) {
#pragma clang fp contract(off)
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, d = p.ndim;
  if (e >= n * d) return;
  const int64_t b = e / d;
  const int c = (int)(e - b * d);
  const bool draw = random && opt_slot(p, c) >= 0;
  const double v = draw ? p.delta + opt_uniform(key, c, b) * (1.0 - 2.0 * p.delta)
                        : opt_clamp((x0[e] - p.lo[c]) / p.width[c], p.delta);
  u[e] = v;
  theta[e] = p.lo[c] + v * p.width[c];
}

// one thread per element of the stencil rows: active problem a, row r = 2 j + side (free slot j), coordinate c
extern "C" __global__ void __launch_bounds__(256)
opt_stencil_kernel(cf_opt_params p, cf_opt_state st, const int32_t* __restrict__ act, int64_t n_act, double* __restrict__ rows) {
#pragma clang fp contract(off)
  const int d = p.ndim, nr = 2 * p.n_free;
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n_act * nr * d) return;
  const int64_t row = e / d, a = row / nr;
  const int c = (int)(e - row * d), r = (int)(row - a * nr), j = r >> 1, side = r & 1;
  const int64_t pb = act[a];
  const double uc = st.u[pb * d + c];
  double v = uc;
  if (p.free_idx[j] == c) {
    const double h = p.h, h2 = 2.0 * h;
    const int fm = opt_form(uc, h, p.delta);
    v = fm == 0 ? (side ? uc - h : uc + h) : fm > 0 ? (side ? uc + h2 : uc + h) : (side ? uc - h2 : uc - h);
    if (side == 0) st.form[pb * CF_OPT_MAX_NDIM + j] = (int8_t)fm;
  }
  rows[e] = p.lo[c] + v * p.width[c];
}

// sum / max over the 16 lanes of a problem, in lane order, the same value on every lane
__device__ __forceinline__ double opt_sum(double v, int nf) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < OPT_LANES; ++j) {
    const double x = __shfl(v, j, OPT_LANES);
    s = j < nf ? s + x : s;
  }
  return s;
}
__device__ __forceinline__ double opt_max_abs(double v, int nf) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < OPT_LANES; ++j) {
    const double x = __shfl(v, j, OPT_LANES);
    s = j < nf ? fmax(s, fabs(x)) : s;
  }
  return s;
}

// 16 lanes per active problem: gradient, convergence test, BFGS update of H^-1, projected direction, K trial rows
extern "C" __global__ void __launch_bounds__(256)
opt_direction_kernel(cf_opt_params p, cf_opt_state st, const int32_t* __restrict__ act, int64_t n_act, const double* __restrict__ fs,
                     double* __restrict__ trials) {
#pragma clang fp contract(off)
  const int64_t a = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / OPT_LANES;
  const int i = (int)(threadIdx.x & (OPT_LANES - 1));
  if (a >= n_act) return;  // whole 16-lane groups leave together: the shuffles below stay inside a group
  const int64_t pb = act[a];
  const int nf = p.n_free, d = p.ndim, K = p.n_trials;
  const bool on = i < nf;
  const double f0 = st.f[pb], delta = p.delta;
  double ui = 0.0, g = 0.0;
  int bad = 0;
  if (on) {
    ui = st.u[pb * d + p.free_idx[i]];
    const int fm = st.form[pb * CF_OPT_MAX_NDIM + i];
    const double f1 = fs[(a * nf + i) * 2], f2 = fs[(a * nf + i) * 2 + 1], h2 = 2.0 * p.h;
    bad = !(isfinite(f1) && isfinite(f2));
    g = fm == 0 ? (f1 - f2) / h2 : fm > 0 ? ((4.0 * f1 - 3.0 * f0) - f2) / h2 : ((3.0 * f0 - 4.0 * f1) + f2) / h2;
  }
  const bool anybad = opt_sum((double)bad, nf) > 0.0;
  // a coordinate at a face whose gradient points out of the box is held
  const bool held = on && ((ui <= delta && g < 0.0) || (ui >= 1.0 - delta && g > 0.0));
  const double pg = on && !held ? g : 0.0;
  const double gnorm = opt_max_abs(pg, nf);
  const bool conv = !anybad && gnorm <= p.gtol + p.gtol_rel * fabs(f0);
  int flags = st.flags[pb];
  double di = 0.0;
  double hrow[OPT_LANES];
  const int64_t hb = pb * (CF_OPT_MAX_NDIM * CF_OPT_MAX_NDIM) + (int64_t)i * CF_OPT_MAX_NDIM;
#pragma unroll
  for (int j = 0; j < OPT_LANES; ++j) hrow[j] = on && j < nf ? st.hinv[hb + j] : 0.0;
  if (!anybad && !conv) {
    bool reset = (flags & CF_OPT_NEED_RESET) != 0;
    if (!reset && (flags & CF_OPT_HAS_PAIR)) {
      // BFGS on -f: s = the last step, y = grad(-f)_new - grad(-f)_old = g_prev - g on the coordinates that are not held
      // (a held coordinate's gradient change says nothing about the curvature of the subspace the search moves in)
      const double si = on ? st.s[pb * CF_OPT_MAX_NDIM + i] : 0.0;
      const double yi = on && !held ? st.g_prev[pb * CF_OPT_MAX_NDIM + i] - g : 0.0;
      const double sy = opt_sum(si * yi, nf), ss = opt_sum(si * si, nf), yy = opt_sum(yi * yi, nf);
      if (sy > 0.0 && sy * sy > (1e-20 * ss) * yy) {  // curvature condition, else the update is skipped
        double hy = 0.0;
#pragma unroll
        for (int j = 0; j < OPT_LANES; ++j) {
          const double yj = __shfl(yi, j, OPT_LANES);
          hy = j < nf ? hy + hrow[j] * yj : hy;
        }
        const double yhy = opt_sum(yi * hy, nf);
        const double rho = 1.0 / sy, b = (1.0 + rho * yhy) * rho;
#pragma unroll
        for (int j = 0; j < OPT_LANES; ++j) {
          const double sj = __shfl(si, j, OPT_LANES), hyj = __shfl(hy, j, OPT_LANES);
          const double t = hy * sj + si * hyj;
          hrow[j] = on && j < nf ? (hrow[j] - rho * t) + b * (si * sj) : 0.0;
        }
      }
    }
    if (!reset) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < OPT_LANES; ++j) {
        const double pgj = __shfl(pg, j, OPT_LANES);
        v = j < nf ? v + hrow[j] * pgj : v;
      }
      di = on && !held ? v : 0.0;
      reset = !(opt_sum(pg * di, nf) > 0.0);  // not an ascent direction
    }
    if (reset) {
      // scaled identity: the largest coordinate move is 10 % of the box at the start and 4 x the last accepted step's (at most
      // 10 %) once a step was taken; after a failed search no more than 4^-K x the failed direction's (the backtracking
      // continued).  Only the reset after a failed search is "fresh": a failure right after it stops the problem.
      const double dmax = opt_max_abs(on ? st.d[pb * CF_OPT_MAX_NDIM + i] : 0.0, nf);
      const double smax = opt_max_abs(on ? st.s[pb * CF_OPT_MAX_NDIM + i] : 0.0, nf);
      const bool after_fail = (flags & CF_OPT_NEED_RESET) && dmax > 0.0;
      const double m0 = (flags & CF_OPT_HAS_STEP) ? fmin(0.1, 4.0 * smax) : 0.1;
      const double m = after_fail ? fmin(m0, ldexp(dmax, -2 * K)) : m0;
      const double sigma = m / gnorm;
#pragma unroll
      for (int j = 0; j < OPT_LANES; ++j) hrow[j] = on && j == i ? sigma : 0.0;
      di = sigma * pg;
      flags = (flags & ~(CF_OPT_NEED_RESET | CF_OPT_FRESH)) | (after_fail ? CF_OPT_FRESH : 0);
    } else {
      flags &= ~CF_OPT_FRESH;
    }
#pragma unroll
    for (int j = 0; j < OPT_LANES; ++j)
      if (on && j < nf) st.hinv[hb + j] = hrow[j];
  }
  if (on) {
    st.g[pb * CF_OPT_MAX_NDIM + i] = g;
    st.d[pb * CF_OPT_MAX_NDIM + i] = di;
  }
  if (i == 0) {
    st.gnorm[pb] = gnorm;
    st.flags[pb] = flags;
    if (anybad) st.status[pb] = CF_OPT_NONFINITE_STENCIL;
    else if (conv) st.status[pb] = CF_OPT_CONVERGED;
  }
  // trial rows (a finished problem gets K copies of its iterate: d = 0); lane c writes coordinate c
  const int c = i;
  const int slot = c < d ? opt_slot(p, c) : -1;
  const double dc = __shfl(di, slot < 0 ? 0 : slot, OPT_LANES);
  if (c < d) {
    const double uc = st.u[pb * d + c];
    for (int k = 0; k < K; ++k) {
      const double v = slot >= 0 ? opt_trial(uc, dc, k, delta) : uc;
      trials[(a * K + k) * d + c] = p.lo[c] + v * p.width[c];
    }
  }
}

// one thread per active problem: Armijo on the K trials (largest step first), else the best improving trial, else a reset
// (or, after a fresh reset, the noise-floor stop); the step s, g_prev, u, f, the counters and the iteration cap
extern "C" __global__ void __launch_bounds__(256)
opt_accept_kernel(cf_opt_params p, cf_opt_state st, const int32_t* __restrict__ act, int64_t n_act, const double* __restrict__ ft) {
#pragma clang fp contract(off)
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (a >= n_act) return;
  const int64_t pb = act[a];
  if (st.status[pb] != CF_OPT_RUNNING) return;
  const int nf = p.n_free, d = p.ndim, K = p.n_trials;
  const double f0 = st.f[pb], delta = p.delta;
  const double* u = st.u + pb * d;
  const double* g = st.g + pb * CF_OPT_MAX_NDIM;
  const double* dd = st.d + pb * CF_OPT_MAX_NDIM;
  const double floor = f0 + ldexp(fabs(f0), -50);  // a trial must beat f by more than its rounding noise, 4 eps |f|
  int pick = -1;
  for (int k = 0; k < K && pick < 0; ++k) {
    const double fk = ft[a * K + k];
    double dec = 0.0;
    for (int j = 0; j < nf; ++j) {
      const double uj = u[p.free_idx[j]];
      dec = dec + g[j] * (opt_trial(uj, dd[j], k, delta) - uj);
    }
    if (isfinite(fk) && fk >= f0 + p.c1 * dec && fk > floor) pick = k;
  }
  if (pick < 0) {
    double best = floor;
    for (int k = 0; k < K; ++k) {
      const double fk = ft[a * K + k];
      if (isfinite(fk) && fk > best) {
        best = fk;
        pick = k;
      }
    }
  }
  int flags = st.flags[pb], status = CF_OPT_RUNNING;
  if (pick >= 0) {
    for (int j = 0; j < nf; ++j) {
      const int c = p.free_idx[j];
      const double uj = st.u[pb * d + c], un = opt_trial(uj, dd[j], pick, delta);
      st.s[pb * CF_OPT_MAX_NDIM + j] = un - uj;
      st.g_prev[pb * CF_OPT_MAX_NDIM + j] = g[j];
      st.u[pb * d + c] = un;
    }
    st.f[pb] = ft[a * K + pick];
    flags = (flags | CF_OPT_HAS_PAIR | CF_OPT_HAS_STEP) & ~(CF_OPT_NEED_RESET | CF_OPT_FRESH);
  } else if (flags & CF_OPT_FRESH) {
    status = CF_OPT_NOISE_FLOOR;  // no ascent even after a reset
  } else {
    flags = (flags | CF_OPT_NEED_RESET) & ~CF_OPT_HAS_PAIR;
  }
  const int it = st.n_iter[pb] + 1;
  if (status == CF_OPT_RUNNING && it >= p.max_iter) status = CF_OPT_ITER_CAP;
  st.n_iter[pb] = it;
  st.flags[pb] = flags;
  st.status[pb] = status;
}

// one workgroup of 1024 threads: the problems of act[0 .. n_act) still running, in order, into next; count[0] = how many
extern "C" __global__ void __launch_bounds__(1024)
opt_compact_kernel(const int32_t* __restrict__ act, int64_t n_act, const int32_t* __restrict__ status, int32_t* __restrict__ next,
                   int32_t* __restrict__ count) {
  __shared__ int wave_total[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int base = 0;
  for (int64_t c0 = 0; c0 < n_act; c0 += 1024) {
    const int64_t e = c0 + t;
    const int pb = e < n_act ? act[e] : 0;
    const bool keep = e < n_act && status[pb] == CF_OPT_RUNNING;
    const unsigned long long m = __ballot(keep);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[w] = __popcll(m);
    __syncthreads();
    int off = base, tot = 0;
    for (int k = 0; k < 16; ++k) {
      off += k < w ? wave_total[k] : 0;
      tot += wave_total[k];
    }
    if (keep) next[off + below] = pb;
    __syncthreads();
    base += tot;
  }
  if (t == 0) count[0] = base;
}

// ------------------------------------------------------------------------------------------------
static int opt_check_params(const cf_opt_params* p, const char* fn) {
  const std::string f(fn);
  if (!p) return cf_set_error(CF_ERR_INVALID, f + ": null params");
  if (p->ndim < 1 || p->ndim > CF_OPT_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, f + ": ndim must be in 1..16");
  if (p->n_free < 1 || p->n_free > p->ndim) return cf_set_error(CF_ERR_INVALID, f + ": n_free must be in 1..ndim");
  for (int j = 0; j < p->n_free; ++j)
    if (p->free_idx[j] < 0 || p->free_idx[j] >= p->ndim || (j > 0 && p->free_idx[j] <= p->free_idx[j - 1]))
      return cf_set_error(CF_ERR_INVALID, f + ": free_idx must be ascending indices below ndim");
  for (int c = 0; c < p->ndim; ++c)
    if (!std::isfinite(p->lo[c]) || !std::isfinite(p->width[c]) || !(p->width[c] > 0.0))
      return cf_set_error(CF_ERR_INVALID, f + ": coordinate " + std::to_string(c) + " needs a finite lo and width > 0");
  if (!(p->h > 0.0 && p->h <= 0.01)) return cf_set_error(CF_ERR_INVALID, f + ": h must be in (0, 0.01]");
  if (!(p->delta > 0.0 && p->delta <= 1e-3)) return cf_set_error(CF_ERR_INVALID, f + ": delta must be in (0, 1e-3]");
  if (!(p->c1 > 0.0 && p->c1 < 1.0)) return cf_set_error(CF_ERR_INVALID, f + ": c1 must be in (0, 1)");
  if (!(p->gtol >= 0.0 && p->gtol_rel >= 0.0 && std::isfinite(p->gtol) && std::isfinite(p->gtol_rel)))
    return cf_set_error(CF_ERR_INVALID, f + ": gtol and gtol_rel must be finite and >= 0");
  if (p->n_trials < 1 || p->n_trials > CF_OPT_MAX_TRIALS) return cf_set_error(CF_ERR_INVALID, f + ": n_trials must be in 1..8");
  if (p->max_iter < 1) return cf_set_error(CF_ERR_INVALID, f + ": max_iter must be >= 1");
  return CF_OK;
}

static int opt_check_state(const cf_opt_state* s, const char* fn) {
  if (!s || !s->u || !s->f || !s->g || !s->g_prev || !s->s || !s->hinv || !s->d || !s->gnorm || !s->form || !s->status ||
      !s->n_iter || !s->flags)
    return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": null state pointer");
  return CF_OK;
}

static unsigned opt_blocks(int64_t threads) { return (unsigned)((threads + 255) / 256); }

extern "C" int cf_opt_starts(const cf_opt_params* params, int64_t n, const double* d_x0, uint64_t key, int32_t random, double* d_u,
                             double* d_theta, void* hip_stream) {
  int rc = opt_check_params(params, "cf_opt_starts");
  if (rc) return rc;
  if (!d_x0 || !d_u || !d_theta || n < 0) return cf_set_error(CF_ERR_INVALID, "cf_opt_starts: null argument or n < 0");
  if (n == 0) return CF_OK;
  hipLaunchKernelGGL(opt_starts_kernel, dim3(opt_blocks(n * params->ndim)), dim3(256), 0, (hipStream_t)hip_stream, *params, n, d_x0, key,
                     (int)(random != 0), d_u, d_theta);
  return cf_launch_status("cf_opt_starts");
}

extern "C" int cf_opt_stencil(const cf_opt_params* params, const cf_opt_state* state, const int32_t* d_active, int64_t n_active,
                              double* d_rows, void* hip_stream) {
  int rc = opt_check_params(params, "cf_opt_stencil");
  if (!rc) rc = opt_check_state(state, "cf_opt_stencil");
  if (rc) return rc;
  if (!d_active || !d_rows || n_active < 0) return cf_set_error(CF_ERR_INVALID, "cf_opt_stencil: null argument or n_active < 0");
  if (n_active == 0) return CF_OK;
  hipLaunchKernelGGL(opt_stencil_kernel, dim3(opt_blocks(n_active * 2 * params->n_free * params->ndim)), dim3(256), 0,
                     (hipStream_t)hip_stream, *params, *state, d_active, n_active, d_rows);
  return cf_launch_status("cf_opt_stencil");
}

extern "C" int cf_opt_direction(const cf_opt_params* params, const cf_opt_state* state, const int32_t* d_active, int64_t n_active,
                                const double* d_fs, double* d_trials, void* hip_stream) {
  int rc = opt_check_params(params, "cf_opt_direction");
  if (!rc) rc = opt_check_state(state, "cf_opt_direction");
  if (rc) return rc;
  if (!d_active || !d_fs || !d_trials || n_active < 0)
    return cf_set_error(CF_ERR_INVALID, "cf_opt_direction: null argument or n_active < 0");
  if (n_active == 0) return CF_OK;
  hipLaunchKernelGGL(opt_direction_kernel, dim3(opt_blocks(n_active * OPT_LANES)), dim3(256), 0, (hipStream_t)hip_stream, *params, *state,
                     d_active, n_active, d_fs, d_trials);
  return cf_launch_status("cf_opt_direction");
}

extern "C" int cf_opt_accept(const cf_opt_params* params, const cf_opt_state* state, const int32_t* d_active, int64_t n_active,
                             const double* d_ft, void* hip_stream) {
  int rc = opt_check_params(params, "cf_opt_accept");
  if (!rc) rc = opt_check_state(state, "cf_opt_accept");
  if (rc) return rc;
  if (!d_active || !d_ft || n_active < 0) return cf_set_error(CF_ERR_INVALID, "cf_opt_accept: null argument or n_active < 0");
  if (n_active == 0) return CF_OK;
  hipLaunchKernelGGL(opt_accept_kernel, dim3(opt_blocks(n_active)), dim3(256), 0, (hipStream_t)hip_stream, *params, *state, d_active,
                     n_active, d_ft);
  return cf_launch_status("cf_opt_accept");
}

extern "C" int cf_opt_compact(const int32_t* d_active, int64_t n_active, const int32_t* d_status, int32_t* d_next, int32_t* d_count,
                              void* hip_stream) {
  if (!d_active || !d_status || !d_next || !d_count || n_active < 0 || n_active > INT32_MAX)
    return cf_set_error(CF_ERR_INVALID, "cf_opt_compact: null argument or n_active out of range");
  hipLaunchKernelGGL(opt_compact_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, d_active, n_active, d_status, d_next, d_count);
  return cf_launch_status("cf_opt_compact");
}
