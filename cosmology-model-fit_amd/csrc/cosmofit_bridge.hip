// cosmofit_bridge.hip — the device side of the bridge-sampling evidence (evidence.py): the box <-> unbounded transform with
// its Jacobian and the whitening by the proposal's Cholesky factor (cf_bridge_forward, cf_bridge_points), the proposal's
// counter-based normal draws (cf_bridge_draw) and the fixed point of Meng & Wong with the moments of its error estimate
// (cf_bridge_solve).
//
// TRANSFORM.  u = (theta - lo) / (hi - lo), phi = log u - log(1 - u) with 1 - u = (hi - theta) / (hi - lo),
// z = R^-1 (phi - mu) by forward substitution in index order.  Going back, theta = lo + (hi - lo) u below the middle of the
// box and hi - (hi - lo) (1 - u) above it, u or 1 - u being e^-|phi| / (1 + e^-|phi|): theta never leaves [lo, hi] and may
// equal a face.  One thread owns one row; the dimension is a template parameter (1 .. CF_BRIDGE_MAX_NDIM) so that phi and z live
// in registers (an array indexed by a run-time ndim would be placed in scratch).  lo, hi, mu and R travel in the kernel
// arguments (cf_bridge_geom, 2.6 kB); each workgroup copies them to LDS once and reads them from there as broadcasts.  A
// row's bits depend on that row and the geometry only.
//
// SOLVE.  r_{t+1} = mean_j A(x_2j) / mean_i B(x_1i) as one launch triple per iteration: bridge_partial_kernel over the
// slices of l2, the same over the slices of l1 (one thread per slice, the slices spread over the CUs), and the one-thread
// bridge_step_kernel that adds the partials, updates r in a small device state and sets its "done" flag when the step
// converged, r broke down or max_iter is reached.  The launches of later iterations read that flag first and return at once.
// The host enqueues CF_BRIDGE_BATCH iterations, reads the flag, and goes on or stops: no read per iteration, no workgroup
// ever waits on another (no grid barrier, no spin), every loop is bounded by max_iter or a row count.  The moments of
// f_1 = A and f_2 = r B at the final r follow as five more partial launches and two one-thread kernels; the last writes the
// record.  State and partials live in a stream-ordered workspace allocated and freed inside the call.  The first form was
// one 1024-thread workgroup iterating to the end in one launch: same order, same bits, but one CU -- 7.1 ms per iteration
// at 2 x 5.12 * 10^6 terms, more than the objective's time on a slowly converging pair (profiles/NOTES_bridge.md).
//
// ORDER OF SUMMATION (fixed; a function of n alone; the cf_kde_sum_device contract).  The terms of a sum are cut into slices
// of CF_BRIDGE_SLICE consecutive terms (the last one shorter).  A slice is added term by term in ascending index to a partial
// that starts at 0.0, by one thread.  The partials are added in ascending slice order to a total that starts at 0.0, by one
// thread.  So the bits of every sum depend on the inputs only: not on the launch geometry, the stream or repetition.  No
// float atomics.
//
// ARITHMETIC.  x = l - lstar; e = exp(-|x|) is the only exponential, never of a positive number, so log P near -700 and
// outliers of +-800 in x neither overflow nor lose the sum:
//   A(x) = 1 / (s1 + s2 r e)   (x >= 0)      e / (s1 e + s2 r)   (x < 0)
//   B(x) = e / (s1 + s2 r e)   (x >= 0)      1 / (s1 e + s2 r)   (x < 0)
// With p = e^x / r:  f_1 = p / (s1 p + s2) = A(x) and f_2 = 1 / (s1 p + s2) = r B(x), so the error moments reuse A and B.
// x_2 = -inf gives e = 0 and A = 0.  NaN or +inf in either vector, or -inf in l_1, is CF_BRIDGE_NONFINITE (nothing iterated).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"
#include "cf_rng.h"

#define CF_BRIDGE_ROW_THREADS 256
#define CF_BRIDGE_BATCH 16  // iterations enqueued between two host reads of the done flag

struct cf_bridge_geom {
  double lo[CF_BRIDGE_MAX_NDIM], hi[CF_BRIDGE_MAX_NDIM], width[CF_BRIDGE_MAX_NDIM], log_width[CF_BRIDGE_MAX_NDIM];
  double mean[CF_BRIDGE_MAX_NDIM];
  double chol[CF_BRIDGE_MAX_NDIM * CF_BRIDGE_MAX_NDIM];  // row-major, pitch CF_BRIDGE_MAX_NDIM, lower triangle
};

// The geometry goes from the kernel arguments to LDS once per workgroup and is read from there as broadcasts (every lane the
// same address): held in scalar registers, the 16-dimensional forms ran out of them and spilled.
#define CF_BRIDGE_GEOM_DOUBLES ((int)(sizeof(cf_bridge_geom) / sizeof(double)))
__device__ __forceinline__ void bridge_stage_geom(const cf_bridge_geom& arg, cf_bridge_geom* lds) {
  const double* src = reinterpret_cast<const double*>(&arg);
  double* dst = reinterpret_cast<double*>(lds);
  for (int i = threadIdx.x; i < CF_BRIDGE_GEOM_DOUBLES; i += CF_BRIDGE_ROW_THREADS) dst[i] = src[i];
  __syncthreads();
}

template <int D>
__global__ void __launch_bounds__(CF_BRIDGE_ROW_THREADS)
bridge_forward_kernel(const double* __restrict__ theta, int64_t n, const cf_bridge_geom arg, double* __restrict__ z_out,
                      double* __restrict__ log_jac) {
  __shared__ cf_bridge_geom g;
  bridge_stage_geom(arg, &g);
  const int64_t row = (int64_t)blockIdx.x * CF_BRIDGE_ROW_THREADS + threadIdx.x;
  if (row >= n) return;
  double z[D];
  double lj = 0.0;
  bool inside = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    // 1 - u is formed as (hi - theta) / (hi - lo), not from the rounded u: next to the upper face 1 - u would carry the
    // rounding of u divided by 1 - u, while both differences here are exact or good to an ulp
    const double t = theta[row * D + k], below = t - g.lo[k], above = g.hi[k] - t;
    inside = inside && below > 0.0 && above > 0.0;  // false for NaN
    const double lu = log(below / g.width[k]), l1u = log(above / g.width[k]);
    lj += g.log_width[k] + lu + l1u;
    double acc = (lu - l1u) - g.mean[k];
#pragma unroll
    for (int j = 0; j < k; ++j) acc -= g.chol[k * CF_BRIDGE_MAX_NDIM + j] * z[j];
    z[k] = acc / g.chol[k * CF_BRIDGE_MAX_NDIM + k];
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
  for (int k = 0; k < D; ++k) z_out[row * D + k] = inside ? z[k] : nan;
  log_jac[row] = inside ? lj : nan;
}

template <int D>
__global__ void __launch_bounds__(CF_BRIDGE_ROW_THREADS)
bridge_points_kernel(const double* __restrict__ z_in, int64_t n, const cf_bridge_geom arg, int mirror, double* __restrict__ theta,
                     double* __restrict__ log_jac) {
  __shared__ cf_bridge_geom g;
  bridge_stage_geom(arg, &g);
  const int64_t row = (int64_t)blockIdx.x * CF_BRIDGE_ROW_THREADS + threadIdx.x;
  if (row >= n) return;
  double z[D];
#pragma unroll
  for (int k = 0; k < D; ++k) z[k] = mirror ? -z_in[row * D + k] : z_in[row * D + k];  // mean - R z is mean + R (-z), bit for bit
  double lj = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double rz = 0.0;
#pragma unroll
    for (int j = 0; j <= k; ++j) rz += g.chol[k * CF_BRIDGE_MAX_NDIM + j] * z[j];
    const double phi = g.mean[k] + rz;
    const double a = fabs(phi), e = exp(-a);
    const double small = g.width[k] * (e / (1.0 + e));  // (hi - lo) times the smaller of u and 1 - u: no positive exponent
    theta[row * D + k] = phi >= 0.0 ? g.hi[k] - small : g.lo[k] + small;
    lj += (g.log_width[k] - a) - 2.0 * log1p(e);
  }
  log_jac[row] = lj;
}

extern "C" __global__ void __launch_bounds__(CF_BRIDGE_ROW_THREADS)
bridge_draw_kernel(uint64_t key, int64_t first, int64_t n, int ndim, double* __restrict__ z) {
  const int64_t e = (int64_t)blockIdx.x * CF_BRIDGE_ROW_THREADS + threadIdx.x;
  if (e >= n * ndim) return;
  const int64_t row = e / ndim;
  const int k = (int)(e - row * ndim);
  z[e] = ens_normal(key, 2 * k, first + row);
}

// ---- the fixed point ----------------------------------------------------------------------------------------------------
struct bridge_terms {
  double a, b;
};
__device__ __forceinline__ bridge_terms bridge_ab(double x, double r, double s1, double s2) {
  const double e = exp(-fabs(x));
  bridge_terms t;
  if (x >= 0.0) {
    const double d = s1 + s2 * r * e;
    t.a = 1.0 / d;
    t.b = e / d;
  } else {
    const double d = s1 * e + s2 * r;
    t.a = e / d;
    t.b = 1.0 / d;
  }
  return t;
}

// which term of a vector a sum takes
enum { BR_A = 0, BR_B = 1, BR_A_DEV2 = 2, BR_F2_DEV2 = 3, BR_F2_STORE = 4 };
// the solve's state in its workspace, followed there by the slice partials of l2 and of l1
enum { ST_R = 0, ST_DONE = 1, ST_ITER = 2, ST_STATUS = 3, ST_BAD = 4, ST_M1 = 5, ST_M2 = 6, ST_DOUBLES = 8 };

extern "C" __global__ void bridge_init_kernel(double* __restrict__ state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    state[ST_R] = 1.0;
    state[ST_DONE] = 0.0;
    state[ST_ITER] = 0.0;
    state[ST_STATUS] = (double)CF_BRIDGE_ITER_CAP;
    state[ST_BAD] = 0.0;
    state[ST_M1] = state[ST_M2] = 0.0;
  }
}

// a posterior sample has a finite l; a proposal draw may have -inf (outside the box) but neither NaN nor +inf.  Every
// thread that finds one stores the same two values: no atomics, and nothing here is read before the next launch.
extern "C" __global__ void __launch_bounds__(CF_BRIDGE_ROW_THREADS)
bridge_check_kernel(const double* __restrict__ l1, int64_t n1, const double* __restrict__ l2, int64_t n2, double* __restrict__ state) {
  const int64_t stride = (int64_t)gridDim.x * CF_BRIDGE_ROW_THREADS;
  int mine = 0;
  for (int64_t j = (int64_t)blockIdx.x * CF_BRIDGE_ROW_THREADS + threadIdx.x; j < n1; j += stride) mine |= !isfinite(l1[j]);
  for (int64_t j = (int64_t)blockIdx.x * CF_BRIDGE_ROW_THREADS + threadIdx.x; j < n2; j += stride) mine |= !(l2[j] < INFINITY);
  if (mine) {
    state[ST_BAD] = 1.0;
    state[ST_DONE] = 1.0;
    state[ST_STATUS] = (double)CF_BRIDGE_NONFINITE;
  }
}

// One thread per slice: part[s] = the slice's terms added in ascending index to a partial that starts at 0.0.  The launches
// of an iteration return at once when the state says done; the launches of the moments (final != 0) run whatever it says,
// and with a refused input write NaN.
template <int WHAT>
__global__ void __launch_bounds__(CF_BRIDGE_ROW_THREADS)
bridge_partial_kernel(const double* __restrict__ l, int64_t n, double lstar, double s1, double s2, const double* __restrict__ state,
                      int final, double* __restrict__ part, double* __restrict__ f2_out) {
  const int64_t n_slices = (n + CF_BRIDGE_SLICE - 1) / CF_BRIDGE_SLICE;
  const int64_t s = (int64_t)blockIdx.x * CF_BRIDGE_ROW_THREADS + threadIdx.x;
  if (s >= n_slices) return;
  if (!final && state[ST_DONE] != 0.0) return;
  const bool bad = state[ST_BAD] != 0.0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double r = state[ST_R];
  const double centre = WHAT == BR_A_DEV2 ? state[ST_M1] : WHAT == BR_F2_DEV2 ? state[ST_M2] : 0.0;
  const int64_t j0 = s * CF_BRIDGE_SLICE, j1 = j0 + CF_BRIDGE_SLICE < n ? j0 + CF_BRIDGE_SLICE : n;
  double acc = 0.0;
  for (int64_t j = j0; j < j1; ++j) {
    const bridge_terms t = bridge_ab(l[j] - lstar, r, s1, s2);
    double v;
    if (WHAT == BR_A) v = t.a;
    else if (WHAT == BR_B) v = t.b;
    else if (WHAT == BR_A_DEV2) v = (t.a - centre) * (t.a - centre);
    else if (WHAT == BR_F2_DEV2) v = (r * t.b - centre) * (r * t.b - centre);
    else {
      v = r * t.b;
      f2_out[j] = bad ? nan : v;
    }
    acc += v;
  }
  part[s] = acc;
}

// the partials of the slices added in ascending slice order to a total that starts at 0.0
__device__ __forceinline__ double bridge_total(const double* __restrict__ part, int64_t n_slices) {
  double tot = 0.0;
  for (int64_t k = 0; k < n_slices; ++k) tot += part[k];
  return tot;
}

// r_{t+1} from the partials of A over l2 and of B over l1; one thread
extern "C" __global__ void bridge_step_kernel(const double* __restrict__ part2, int64_t n_sl2, int64_t n2, const double* __restrict__ part1,
                                              int64_t n_sl1, int64_t n1, double tol, int max_iter, double* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || state[ST_DONE] != 0.0) return;
  const double r = state[ST_R];
  const double num = bridge_total(part2, n_sl2) / (double)n2, den = bridge_total(part1, n_sl1) / (double)n1;
  const double rn = num / den;
  const double it = state[ST_ITER] + 1.0;
  const bool conv = fabs(rn - r) <= tol * rn;
  state[ST_R] = rn;
  state[ST_ITER] = it;
  if (!(rn > 0.0) || !(rn < INFINITY)) {  // every draw outside the box (r = 0), or a breakdown
    state[ST_STATUS] = (double)CF_BRIDGE_NONFINITE;
    state[ST_DONE] = 1.0;
  } else if (conv) {
    state[ST_STATUS] = (double)CF_BRIDGE_CONVERGED;
    state[ST_DONE] = 1.0;
  } else if (it >= (double)max_iter) {
    state[ST_DONE] = 1.0;  // the status is still CF_BRIDGE_ITER_CAP
  }
}

extern "C" __global__ void bridge_means_kernel(const double* __restrict__ part2, int64_t n_sl2, int64_t n2, const double* __restrict__ part1,
                                               int64_t n_sl1, int64_t n1, double* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  state[ST_M1] = bridge_total(part2, n_sl2) / (double)n2;
  state[ST_M2] = bridge_total(part1, n_sl1) / (double)n1;
}

extern "C" __global__ void bridge_record_kernel(const double* __restrict__ part2, int64_t n_sl2, int64_t n2, const double* __restrict__ part1,
                                                int64_t n_sl1, int64_t n1, const double* __restrict__ state, double* __restrict__ result) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (state[ST_BAD] != 0.0) {
    for (int k = 0; k < CF_BRIDGE_RESULT_DOUBLES; ++k) result[k] = nan;
    result[CF_BR_N_ITER] = 0.0;
    result[CF_BR_STATUS] = (double)CF_BRIDGE_NONFINITE;
    return;
  }
  const double q1 = bridge_total(part2, n_sl2), q2 = bridge_total(part1, n_sl1), r = state[ST_R];
  result[CF_BR_LOG_R] = log(r);
  result[CF_BR_N_ITER] = state[ST_ITER];
  result[CF_BR_STATUS] = state[ST_STATUS];
  result[CF_BR_MEAN_F1] = state[ST_M1];
  result[CF_BR_VAR_F1] = n2 > 1 ? q1 / (double)(n2 - 1) : 0.0;
  result[CF_BR_MEAN_F2] = state[ST_M2];
  result[CF_BR_VAR_F2] = n1 > 1 ? q2 / (double)(n1 - 1) : 0.0;
  result[CF_BR_R] = r;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static int bridge_geom(const char* who, int64_t n, int32_t ndim, const double* lo, const double* hi, const double* mean,
                       const double* chol, const void* a, const void* b, const void* c, cf_bridge_geom* g) {
  const std::string w(who);
  if (ndim < 1 || ndim > CF_BRIDGE_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, w + ": need 1 <= ndim <= 16");
  if (n < 1) return cf_set_error(CF_ERR_INVALID, w + ": need n >= 1");
  if (n > ((int64_t)1 << 38)) return cf_set_error(CF_ERR_INVALID, w + ": need n <= 2^38");
  if (!lo || !hi || !mean || !chol || !a || !b || !c) return cf_set_error(CF_ERR_INVALID, w + ": null argument");
  for (int k = 0; k < CF_BRIDGE_MAX_NDIM; ++k) {
    g->lo[k] = 0.0, g->hi[k] = 1.0, g->width[k] = 1.0, g->log_width[k] = 0.0, g->mean[k] = 0.0;
    for (int j = 0; j < CF_BRIDGE_MAX_NDIM; ++j) g->chol[k * CF_BRIDGE_MAX_NDIM + j] = k == j ? 1.0 : 0.0;
  }
  for (int k = 0; k < ndim; ++k) {
    const double wd = hi[k] - lo[k];
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !(wd > 0.0) || !std::isfinite(wd))
      return cf_set_error(CF_ERR_INVALID, w + ": the box must be finite with lo < hi in every coordinate");
    if (!std::isfinite(mean[k])) return cf_set_error(CF_ERR_INVALID, w + ": the proposal's mean must be finite");
    g->lo[k] = lo[k], g->hi[k] = hi[k], g->width[k] = wd, g->log_width[k] = std::log(wd), g->mean[k] = mean[k];
    for (int j = 0; j <= k; ++j) {
      const double v = chol[k * ndim + j];
      if (!std::isfinite(v) || (j == k && !(v > 0.0)))
        return cf_set_error(CF_ERR_INVALID, w + ": the Cholesky factor must be finite with a positive diagonal");
      g->chol[k * CF_BRIDGE_MAX_NDIM + j] = v;
    }
  }
  return CF_OK;
}

#define CF_BRIDGE_DISPATCH(KERNEL, ...)                                                                                  \
  switch (ndim) {                                                                                                        \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 5: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 6: hipLaunchKernelGGL(KERNEL<6>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 7: hipLaunchKernelGGL(KERNEL<7>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 8: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 9: hipLaunchKernelGGL(KERNEL<9>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                  \
    case 10: hipLaunchKernelGGL(KERNEL<10>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                \
    case 11: hipLaunchKernelGGL(KERNEL<11>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                \
    case 12: hipLaunchKernelGGL(KERNEL<12>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                \
    case 13: hipLaunchKernelGGL(KERNEL<13>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                \
    case 14: hipLaunchKernelGGL(KERNEL<14>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                \
    case 15: hipLaunchKernelGGL(KERNEL<15>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                \
    default: hipLaunchKernelGGL(KERNEL<16>, grid, dim3(CF_BRIDGE_ROW_THREADS), 0, st, __VA_ARGS__); break;                \
  }

extern "C" int cf_bridge_forward(const double* d_theta, int64_t n, int32_t ndim, const double* lo, const double* hi,
                                 const double* mean, const double* chol, double* d_z, double* d_log_jac, void* hip_stream) {
  cf_bridge_geom g;
  const int rc = bridge_geom("cf_bridge_forward", n, ndim, lo, hi, mean, chol, d_theta, d_z, d_log_jac, &g);
  if (rc != CF_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)((n + CF_BRIDGE_ROW_THREADS - 1) / CF_BRIDGE_ROW_THREADS));
  CF_BRIDGE_DISPATCH(bridge_forward_kernel, d_theta, n, g, d_z, d_log_jac)
  return cf_launch_status("cf_bridge_forward");
}

extern "C" int cf_bridge_points(const double* d_z, int64_t n, int32_t ndim, const double* lo, const double* hi, const double* mean,
                                const double* chol, int32_t mirror, double* d_theta, double* d_log_jac, void* hip_stream) {
  cf_bridge_geom g;
  const int rc = bridge_geom("cf_bridge_points", n, ndim, lo, hi, mean, chol, d_z, d_theta, d_log_jac, &g);
  if (rc != CF_OK) return rc;
  if (mirror != 0 && mirror != 1) return cf_set_error(CF_ERR_INVALID, "cf_bridge_points: mirror must be 0 or 1");
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)((n + CF_BRIDGE_ROW_THREADS - 1) / CF_BRIDGE_ROW_THREADS));
  CF_BRIDGE_DISPATCH(bridge_points_kernel, d_z, n, g, (int)mirror, d_theta, d_log_jac)
  return cf_launch_status("cf_bridge_points");
}

extern "C" int cf_bridge_draw(uint64_t key, int64_t first, int64_t n, int32_t ndim, double* d_z, void* hip_stream) {
  if (ndim < 1 || ndim > CF_BRIDGE_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, "cf_bridge_draw: need 1 <= ndim <= 16");
  if (n < 1 || n > ((int64_t)1 << 38)) return cf_set_error(CF_ERR_INVALID, "cf_bridge_draw: need 1 <= n <= 2^38");
  if (first < 0 || first > ((int64_t)1 << 62)) return cf_set_error(CF_ERR_INVALID, "cf_bridge_draw: need 0 <= first <= 2^62");
  if (!d_z) return cf_set_error(CF_ERR_INVALID, "cf_bridge_draw: null argument");
  const int64_t blocks = (n * ndim + CF_BRIDGE_ROW_THREADS - 1) / CF_BRIDGE_ROW_THREADS;
  if (blocks > (int64_t)INT32_MAX) return cf_set_error(CF_ERR_INVALID, "cf_bridge_draw: too many draws for one call");
  hipLaunchKernelGGL(bridge_draw_kernel, dim3((unsigned)blocks), dim3(CF_BRIDGE_ROW_THREADS), 0, (hipStream_t)hip_stream, key, first,
                     n, (int)ndim, d_z);
  return cf_launch_status("cf_bridge_draw");
}

extern "C" int cf_bridge_solve(const double* d_l1, int64_t n1, const double* d_l2, int64_t n2, double lstar, double s1, double s2,
                               double tol, int32_t max_iter, double* d_result, double* d_f2, void* hip_stream) {
  if (!d_l1 || !d_l2 || !d_result || !d_f2) return cf_set_error(CF_ERR_INVALID, "cf_bridge_solve: null argument");
  if (n1 < 1 || n2 < 1 || n1 > ((int64_t)1 << 38) || n2 > ((int64_t)1 << 38))
    return cf_set_error(CF_ERR_INVALID, "cf_bridge_solve: need 1 <= n1, n2 <= 2^38");
  if (!std::isfinite(lstar)) return cf_set_error(CF_ERR_INVALID, "cf_bridge_solve: lstar must be finite");
  if (!(s1 > 0.0) || !(s2 > 0.0) || !std::isfinite(s1) || !std::isfinite(s2))
    return cf_set_error(CF_ERR_INVALID, "cf_bridge_solve: s1 and s2 must be finite and > 0");
  if (!(tol >= 0.0) || !std::isfinite(tol)) return cf_set_error(CF_ERR_INVALID, "cf_bridge_solve: tol must be finite and >= 0");
  if (max_iter < 1) return cf_set_error(CF_ERR_INVALID, "cf_bridge_solve: need max_iter >= 1");
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t n_sl1 = (n1 + CF_BRIDGE_SLICE - 1) / CF_BRIDGE_SLICE, n_sl2 = (n2 + CF_BRIDGE_SLICE - 1) / CF_BRIDGE_SLICE;
  double* work = nullptr;  // state, then the partials of l2, then those of l1; stream-ordered, freed inside the call
  if (hipMallocAsync(reinterpret_cast<void**>(&work), (size_t)(ST_DOUBLES + n_sl1 + n_sl2) * sizeof(double), st) != hipSuccess) {
    (void)hipGetLastError();
    return cf_set_error(CF_ERR_HIP, "cf_bridge_solve: no workspace for the slice partials");
  }
  double *state = work, *part2 = work + ST_DOUBLES, *part1 = part2 + n_sl2;
  const dim3 one(1), lane(64), row(CF_BRIDGE_ROW_THREADS);
  const dim3 g1((unsigned)((n_sl1 + CF_BRIDGE_ROW_THREADS - 1) / CF_BRIDGE_ROW_THREADS));
  const dim3 g2((unsigned)((n_sl2 + CF_BRIDGE_ROW_THREADS - 1) / CF_BRIDGE_ROW_THREADS));
  const int64_t check_blocks = ((n1 > n2 ? n1 : n2) + CF_BRIDGE_ROW_THREADS - 1) / CF_BRIDGE_ROW_THREADS;
  hipLaunchKernelGGL(bridge_init_kernel, one, lane, 0, st, state);
  hipLaunchKernelGGL(bridge_check_kernel, dim3((unsigned)(check_blocks < 1024 ? check_blocks : 1024)), row, 0, st, d_l1, n1, d_l2, n2, state);
  hipError_t err = hipGetLastError();
  // batches of CF_BRIDGE_BATCH iterations, three launches each, between host reads of the done flag; once it is set the
  // remaining launches of a batch return at once
  for (int64_t launched = 0; err == hipSuccess && launched < (int64_t)max_iter; launched += CF_BRIDGE_BATCH) {
    for (int k = 0; k < CF_BRIDGE_BATCH; ++k) {
      hipLaunchKernelGGL(bridge_partial_kernel<BR_A>, g2, row, 0, st, d_l2, n2, lstar, s1, s2, (const double*)state, 0, part2, (double*)nullptr);
      hipLaunchKernelGGL(bridge_partial_kernel<BR_B>, g1, row, 0, st, d_l1, n1, lstar, s1, s2, (const double*)state, 0, part1, (double*)nullptr);
      hipLaunchKernelGGL(bridge_step_kernel, one, lane, 0, st, (const double*)part2, n_sl2, n2, (const double*)part1, n_sl1, n1, tol,
                         (int)max_iter, state);
    }
    double done = 0.0;
    err = hipMemcpyAsync(&done, state + ST_DONE, sizeof(double), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (done != 0.0) break;
  }
  if (err == hipSuccess) {
    // the moments of f_1 = A(x_2) and f_2 = r B(x_1) at the final r: the means, then the sums of squared deviations
    hipLaunchKernelGGL(bridge_partial_kernel<BR_A>, g2, row, 0, st, d_l2, n2, lstar, s1, s2, (const double*)state, 1, part2, (double*)nullptr);
    hipLaunchKernelGGL(bridge_partial_kernel<BR_F2_STORE>, g1, row, 0, st, d_l1, n1, lstar, s1, s2, (const double*)state, 1, part1, d_f2);
    hipLaunchKernelGGL(bridge_means_kernel, one, lane, 0, st, (const double*)part2, n_sl2, n2, (const double*)part1, n_sl1, n1, state);
    hipLaunchKernelGGL(bridge_partial_kernel<BR_A_DEV2>, g2, row, 0, st, d_l2, n2, lstar, s1, s2, (const double*)state, 1, part2,
                       (double*)nullptr);
    hipLaunchKernelGGL(bridge_partial_kernel<BR_F2_DEV2>, g1, row, 0, st, d_l1, n1, lstar, s1, s2, (const double*)state, 1, part1,
                       (double*)nullptr);
    hipLaunchKernelGGL(bridge_record_kernel, one, lane, 0, st, (const double*)part2, n_sl2, n2, (const double*)part1, n_sl1, n1,
                       (const double*)state, d_result);
    err = hipGetLastError();
  }
  const hipError_t freed = hipFreeAsync(work, st);  // stream-ordered: after the record kernel
  if (err == hipSuccess) err = freed;
  return err == hipSuccess ? CF_OK : cf_set_error(CF_ERR_HIP, "cf_bridge_solve: launch failed");
}
