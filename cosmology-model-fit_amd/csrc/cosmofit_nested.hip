// cosmofit_nested.hip — the per-step kernels of a device-resident nested sampler (nested.py is the driver).
//
// Classic nested sampling with batch deletion: every iteration kills the lowest-likelihood batch of the live set and
// replaces it by walkers that start at random survivors and take n_walk steps of a differential-evolution walk
// constrained to {log L > L*}.  One walk step is
//     propose (this file) -> log L of the proposals (the engine, or any torch callable) -> accept (this file),
// asynchronous on the caller's stream with no host round trip; L* is read from device memory.  The arithmetic is a few
// flops per walker and dimension, so these launches are short next to a likelihood call of thousands of walkers.
//
// Random numbers: the ensemble's counter-based generator (cosmofit_ensemble.hip: ens_mix / ens_uniform / ens_normal,
// restated here with the same bits), keyed on (seed, iteration, walk step) with a domain tag of its own (nested.py:
// ns_key).  Floating-point contraction is off in every expression that the tests restate in numpy, so a uniform-prior
// iteration has the restatement's bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"

__device__ __forceinline__ uint64_t ns_mix(uint64_t x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t ns_bits(uint64_t key0, int stream, int64_t id) {
  const uint64_t x = ns_mix((uint64_t)id * 0x9E3779B97F4A7C15ull + key0 + (uint64_t)stream);
  return ns_mix(x + 0x9E3779B97F4A7C15ull);
}
// uniform in [0, 1): ens_uniform
__device__ __forceinline__ double ns_uniform(uint64_t key0, int stream, int64_t id) {
  return (double)(ns_bits(key0, stream, id) >> 11) * (1.0 / 9007199254740992.0);
}
// uniform in (0, 1): the same 53 bits with the lowest one set, an odd multiple of 2^-53 (the prior draw: Phi^-1 stays finite)
__device__ __forceinline__ double ns_uniform_open(uint64_t key0, int stream, int64_t id) {
  return (double)((ns_bits(key0, stream, id) >> 11) | 1ull) * (1.0 / 9007199254740992.0);
}
// standard normal by Box-Muller from streams `stream`, `stream + 1`: ens_normal
__device__ __forceinline__ double ns_normal(uint64_t key0, int stream, int64_t id) {
#pragma clang fp contract(off)
  const double u1 = 1.0 - ns_uniform(key0, stream, id);
  const double u2 = ns_uniform(key0, stream + 1, id);
  return sqrt(-2.0 * log(u1)) * cos((2.0 * 3.14159265358979323846) * u2);
}

// theta = T(u): lo + u (hi - lo), or loc + scale * Phi^-1(u) (ocml's inverse normal CDF).  Not inlined: inlined into the
// propose kernel's loop, Phi^-1 takes that kernel from 88 to 256 VGPRs.
__device__ __attribute__((noinline)) double ns_transform(int kind, double a, double b, double u) {
#pragma clang fp contract(off)
  return kind == CF_NS_NORMAL ? a + b * normcdfinv(u) : a + u * (b - a);
}

// one thread per element (i, k): u from stream k at counter i, theta = T(u)
extern "C" __global__ void __launch_bounds__(256)
ns_prior_draw_kernel(cf_ns_prior p, int64_t n, uint64_t key, double* __restrict__ u, double* __restrict__ theta) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, d = p.ndim;
  if (e >= n * d) return;
  const int64_t i = e / d;
  const int k = (int)(e - i * d);
  const double v = ns_uniform_open(key, k, i);
  u[e] = v;
  theta[e] = ns_transform(p.kind[k], p.a[k], p.b[k], v);
}

extern "C" __global__ void __launch_bounds__(256)
ns_transform_kernel(cf_ns_prior p, const double* __restrict__ u, int64_t n, double* __restrict__ theta) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, d = p.ndim;
  if (e >= n * d) return;
  const int k = (int)(e % d);
  theta[e] = ns_transform(p.kind[k], p.a[k], p.b[k], u[e]);
}

// walker i starts at survivor floor(U * n_surv) of the frozen snapshot (the survivors in index order)
extern "C" __global__ void __launch_bounds__(256)
ns_walk_start_kernel(const double* __restrict__ su, const double* __restrict__ stheta, const double* __restrict__ slogl, int64_t n_surv,
                     int d, int64_t m, uint64_t key, double* __restrict__ wu, double* __restrict__ wtheta, double* __restrict__ wlogl) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  int64_t j = (int64_t)(ns_uniform(key, 0, i) * (double)n_surv);
  j = j > n_surv - 1 ? n_surv - 1 : j;
  for (int k = 0; k < d; ++k) {
    wu[i * d + k] = su[j * d + k];
    wtheta[i * d + k] = stheta[j * d + k];
  }
  wlogl[i] = slogl[j];
}

// u' = u + gamma (u_a - u_b) + sigma N: a uniform on the survivors, b uniform on the others.  The proposal is written first
// and read back for the transform, so that no per-dimension array is held in registers (ndim is a run-time value).
extern "C" __global__ void __launch_bounds__(256)
ns_propose_kernel(cf_ns_prior p, const double* __restrict__ su, int64_t n_surv, int64_t m, uint64_t key, double gamma, double sigma,
                  const double* __restrict__ wu, const double* __restrict__ wtheta, double* __restrict__ pu, double* __restrict__ ptheta,
                  int32_t* __restrict__ ok) {
#pragma clang fp contract(off)
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int d = p.ndim;
  int64_t a = (int64_t)(ns_uniform(key, 0, i) * (double)n_surv);
  a = a > n_surv - 1 ? n_surv - 1 : a;
  int64_t b = (int64_t)(ns_uniform(key, 1, i) * (double)(n_surv - 1));
  b = b > n_surv - 2 ? n_surv - 2 : b;
  b += b >= a ? 1 : 0;
  bool inside = true;
#pragma unroll 1
  for (int k = 0; k < d; ++k) {
    const double v = wu[i * d + k] + gamma * (su[a * d + k] - su[b * d + k]) + sigma * ns_normal(key, 2 + 2 * k, i);
    pu[i * d + k] = v;
    inside = inside && v > 0.0 && v < 1.0;
  }
#pragma unroll 1
  for (int k = 0; k < d; ++k)
    ptheta[i * d + k] = inside ? ns_transform(p.kind[k], p.a[k], p.b[k], pu[i * d + k]) : wtheta[i * d + k];
  ok[i] = inside ? 1 : 0;
}

// accept iff inside the cube and L* < log L < inf; counts[0..2] += accepted, out of the cube, non-finite (one integer atomic
// per wave and counter)
extern "C" __global__ void __launch_bounds__(256)
ns_accept_kernel(int64_t m, int d, const double* __restrict__ lstar, const double* __restrict__ pu, const double* __restrict__ ptheta,
                 const int32_t* __restrict__ ok, const double* __restrict__ plogl, double* __restrict__ wu, double* __restrict__ wtheta,
                 double* __restrict__ wlogl, unsigned long long* __restrict__ counts) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool acc = false, out = false, bad = false;
  if (i < m) {
    const double l = plogl[i];
    out = ok[i] == 0;
    bad = !out && !isfinite(l);
    acc = !out && !bad && l > lstar[0];
    if (acc) {
      for (int k = 0; k < d; ++k) {
        wu[i * d + k] = pu[i * d + k];
        wtheta[i * d + k] = ptheta[i * d + k];
      }
      wlogl[i] = l;
    }
  }
  const unsigned long long ma = __ballot(acc), mo = __ballot(out), mb = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    if (ma) atomicAdd(counts + 0, (unsigned long long)__popcll(ma));
    if (mo) atomicAdd(counts + 1, (unsigned long long)__popcll(mo));
    if (mb) atomicAdd(counts + 2, (unsigned long long)__popcll(mb));
  }
}

// ------------------------------------------------------------------------------------------------
static int ns_check_prior(const cf_ns_prior* p, const char* fn) {
  if (!p) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": null prior");
  if (p->ndim < 1 || p->ndim > CF_NS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": ndim must be in 1..16");
  for (int k = 0; k < p->ndim; ++k) {
    const bool uni = p->kind[k] == CF_NS_UNIFORM, nor = p->kind[k] == CF_NS_NORMAL;
    if ((!uni && !nor) || !std::isfinite(p->a[k]) || !std::isfinite(p->b[k]) || (uni && !(p->a[k] < p->b[k])) || (nor && !(p->b[k] > 0.0)))
      return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": dimension " + std::to_string(k) +
                                              " needs a uniform lo < hi or a normal with scale > 0");
  }
  return 0;
}

static unsigned ns_blocks(int64_t threads) { return (unsigned)((threads + 255) / 256); }

extern "C" int cf_ns_prior_draw(const cf_ns_prior* prior, int64_t n, uint64_t key, double* d_u, double* d_theta, void* hip_stream) {
  int rc = ns_check_prior(prior, "cf_ns_prior_draw");
  if (rc) return rc;
  if (!d_u || !d_theta || n < 0) return cf_set_error(CF_ERR_INVALID, "cf_ns_prior_draw: null argument or n < 0");
  if (n == 0) return CF_OK;
  hipLaunchKernelGGL(ns_prior_draw_kernel, dim3(ns_blocks(n * prior->ndim)), dim3(256), 0, (hipStream_t)hip_stream, *prior, n, key, d_u,
                     d_theta);
  return cf_launch_status("cf_ns_prior_draw");
}

extern "C" int cf_ns_transform(const cf_ns_prior* prior, const double* d_u, int64_t n, double* d_theta, void* hip_stream) {
  int rc = ns_check_prior(prior, "cf_ns_transform");
  if (rc) return rc;
  if (!d_u || !d_theta || n < 0) return cf_set_error(CF_ERR_INVALID, "cf_ns_transform: null argument or n < 0");
  if (n == 0) return CF_OK;
  hipLaunchKernelGGL(ns_transform_kernel, dim3(ns_blocks(n * prior->ndim)), dim3(256), 0, (hipStream_t)hip_stream, *prior, d_u, n, d_theta);
  return cf_launch_status("cf_ns_transform");
}

extern "C" int cf_ns_walk_start(const double* d_su, const double* d_stheta, const double* d_slogl, int64_t n_surv, int32_t ndim, int64_t m,
                                uint64_t key, double* d_wu, double* d_wtheta, double* d_wlogl, void* hip_stream) {
  if (ndim < 1 || ndim > CF_NS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, "cf_ns_walk_start: ndim must be in 1..16");
  if (n_surv < 1 || m < 0) return cf_set_error(CF_ERR_INVALID, "cf_ns_walk_start: needs n_surv >= 1 and m >= 0");
  if (!d_su || !d_stheta || !d_slogl || !d_wu || !d_wtheta || !d_wlogl) return cf_set_error(CF_ERR_INVALID, "cf_ns_walk_start: null argument");
  if (m == 0) return CF_OK;
  hipLaunchKernelGGL(ns_walk_start_kernel, dim3(ns_blocks(m)), dim3(256), 0, (hipStream_t)hip_stream, d_su, d_stheta, d_slogl, n_surv,
                     (int)ndim, m, key, d_wu, d_wtheta, d_wlogl);
  return cf_launch_status("cf_ns_walk_start");
}

extern "C" int cf_ns_propose(const cf_ns_prior* prior, const double* d_su, int64_t n_surv, int64_t m, uint64_t key, double gamma,
                             double sigma, const double* d_wu, const double* d_wtheta, double* d_pu, double* d_ptheta, int32_t* d_ok,
                             void* hip_stream) {
  int rc = ns_check_prior(prior, "cf_ns_propose");
  if (rc) return rc;
  if (n_surv < 2 || m < 0) return cf_set_error(CF_ERR_INVALID, "cf_ns_propose: needs n_surv >= 2 (two distinct partners) and m >= 0");
  if (!d_su || !d_wu || !d_wtheta || !d_pu || !d_ptheta || !d_ok) return cf_set_error(CF_ERR_INVALID, "cf_ns_propose: null argument");
  if (m == 0) return CF_OK;
  hipLaunchKernelGGL(ns_propose_kernel, dim3(ns_blocks(m)), dim3(256), 0, (hipStream_t)hip_stream, *prior, d_su, n_surv, m, key, gamma, sigma,
                     d_wu, d_wtheta, d_pu, d_ptheta, d_ok);
  return cf_launch_status("cf_ns_propose");
}

extern "C" int cf_ns_accept(int64_t m, int32_t ndim, const double* d_lstar, const double* d_pu, const double* d_ptheta, const int32_t* d_ok,
                            const double* d_plogl, double* d_wu, double* d_wtheta, double* d_wlogl, uint64_t* d_counts, void* hip_stream) {
  if (ndim < 1 || ndim > CF_NS_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, "cf_ns_accept: ndim must be in 1..16");
  if (m < 0) return cf_set_error(CF_ERR_INVALID, "cf_ns_accept: m < 0");
  if (!d_lstar || !d_pu || !d_ptheta || !d_ok || !d_plogl || !d_wu || !d_wtheta || !d_wlogl || !d_counts)
    return cf_set_error(CF_ERR_INVALID, "cf_ns_accept: null argument");
  if (m == 0) return CF_OK;
  hipLaunchKernelGGL(ns_accept_kernel, dim3(ns_blocks(m)), dim3(256), 0, (hipStream_t)hip_stream, m, (int)ndim, d_lstar, d_pu, d_ptheta, d_ok,
                     d_plogl, d_wu, d_wtheta, d_wlogl, (unsigned long long*)d_counts);
  return cf_launch_status("cf_ns_accept");
}
