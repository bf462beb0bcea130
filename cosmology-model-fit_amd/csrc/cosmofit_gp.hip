// cosmofit_gp.hip — exact Gaussian-process regression of H(z) with theta-dependent covariance (include/cosmofit.h: cf_gp_*; the
// driver is cosmology-model-fit_amd/gp.py).
//
// What ohd/cc_gp.py + ohd/gp_lib.py fit: a constant mean m, a scaled RBF kernel (output scale s_f^2, length scale l) and the
// full data covariance C as fixed noise times one learned noise scale s (cc_gp.py:14-41, gp_lib.py:55-68).  Here the log
// marginal likelihood is a batched theta[W, 4] -> [W] function, so that the type-II maximum, the hyperparameter posterior and
// the evidence come from the library's optimizer and samplers, and the predictive moments of H(z) and H'(z) are evaluated for
// every row of a device chain.
//
// Unlike every likelihood kernel of the library, the matrix to factor depends on theta: nothing is prepared on the host.
//
// gp_mll_kernel: ONE WAVE PER ROW, lane i owns matrix row i (n <= 64).
//   * K = s_f^2 exp(-(z_i - z_j)^2 / 2 l^2) + s C_ij is built straight into LDS, lower triangle only.  Rows i and n - 1 - i are
//     paired so that the n (n + 1) / 2 exponentials spread evenly over the lanes.
//   * Storage is column-major with an odd leading dimension: the lanes' read of one column is contiguous (conflict-free), and
//     the read of one element of the pivot column is the same address in every lane (a broadcast).
//   * Right-looking Cholesky in place, pivots in index order.  The forward solve of r = y - m is carried along as one more
//     column held in registers (r_i in lane i), so w = L^-1 r and r^T K^-1 r = sum_k w_k^2 (k ascending) need no second pass.
//     log|K| = sum_k log(pivot_k), k ascending, one log per lane.
//   * LDS: (n | 1) n + 64 doubles = 33 792 B at n = 64, 12 368 B at n = 38.
//
// gp_predict_kernel: ONE 256-THREAD WORKGROUP PER ROW.  All four waves build K, the first wave factors it (same code), then
// every wave takes test points round-robin.  For a test point lane i holds k*_i and dk*_i / dz*; both forward substitutions run
// together against the columns of L (contiguous reads), the solved component of step k is handed to all lanes with two
// v_readlane, and the five dot products accumulate in step order in every lane: no reduction tree and no per-lane scratch.
// The predictive mean is m + (L^-1 k*) . (L^-1 r), the same number as m + k*^T alpha with alpha = K^-1 r, without the
// backward substitution.
//
// Every sum runs in an order fixed by the row (and the test point) alone: a row's bits depend neither on W / S, nor on its
// position, nor on the launch geometry.  The only atomic is the integer count of failed factorisations.  No index depends on a
// value computed from theta: a failed pivot lets NaN run through the remaining arithmetic and is reported at the end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cosmofit.h"
#include "cf_host.h"

#define GP_WAVE 64
#define GP_PRED_TPB 256
#define GP_HOST_CHUNK 16384
#define GP_MAX_ROWS (((int64_t)1 << 31) - 1)
#define GP_LAUNCH_ROWS ((int64_t)1 << 22)  // rows (workgroups) per grid: 2^30 threads at 256 per workgroup

struct GpDev {
  const double* z;  // [n]
  const double* y;  // [n]
  const double* C;  // [n * n] row-major; the lower triangle is read
  unsigned long long* fail_count;
  int n, ld;
  double lo[CF_GP_NDIM], hi[CF_GP_NDIM];
};

struct cf_gp {
  int device = 0;
  GpDev d{};
  DevBuf buf;  // z, y, C, then the counter
  hipStream_t stream = nullptr;
  std::mutex mu;
};

__device__ __host__ inline int gp_ld(int n) { return n | 1; }
__device__ __host__ inline size_t gp_lds_doubles(int n) { return (size_t)gp_ld(n) * n + GP_WAVE; }

// lane k's v in every lane; k is the same in all lanes
__device__ __forceinline__ double gp_bcast(double v, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

struct GpHyper {
  double m, sf2, ell, s;
  bool inbox;  // every entry strictly inside the box (false for NaN and +-inf)
};

__device__ __forceinline__ GpHyper gp_hyper(const GpDev& g, const double* __restrict__ th) {
  GpHyper h;
  h.m = th[0]; h.sf2 = th[1]; h.ell = th[2]; h.s = th[3];
  bool in = true;
#pragma unroll
  for (int k = 0; k < CF_GP_NDIM; ++k) in = in & (g.lo[k] < th[k]) & (th[k] < g.hi[k]);
  h.inbox = in;
  return h;
}

// What the factoring wave keeps, lane k: w_k = (L^-1 r)_k, 1 / L_kk, pivot_k = L_kk^2; in every lane: q = sum w_k^2, ok.
struct GpFactor {
  double w, rinv, piv, q;
  bool ok;
};

// Called by every thread of the workgroup (the barriers are the workgroup's); all threads build, wave 0 factors.
__device__ __forceinline__ GpFactor gp_build_factor(const GpDev& g, const GpHyper& h, double* __restrict__ A, double* __restrict__ zs) {
  const int n = g.n, ld = g.ld, tid = threadIdx.x, lane = tid & (GP_WAVE - 1);
  const bool active = tid < GP_WAVE;
  if (tid < n) zs[tid] = g.z[tid];
  __syncthreads();
  // rows p and n - 1 - p together hold n + 1 entries of the lower triangle
  const int half = (n + 1) >> 1, cols = n + 1, total = half * cols;
  const double c2 = -0.5 / (h.ell * h.ell);
  for (int idx = tid; idx < total; idx += blockDim.x) {
    const int p = idx / cols, q = idx - p * cols;
    int i = p, j = q;
    if (q > p) {
      i = n - 1 - p;
      j = q - p - 1;
      if (i == p) continue;  // the middle row of an odd n is its own partner
    }
    const double dz = zs[i] - zs[j];
    A[j * ld + i] = fma(h.s, g.C[i * n + j], h.sf2 * exp(c2 * (dz * dz)));
    if (i != j) A[i * ld + j] = 0.0;  // the mirror slot of the upper triangle: never read as data, but never garbage either
  }
  __syncthreads();
  GpFactor f;
  f.w = 0.0; f.rinv = 0.0; f.piv = 1.0; f.q = 0.0; f.ok = true;
  const bool row = active && lane < n;
  double r = row ? g.y[lane] - h.m : 0.0;
  for (int k = 0; k < n; ++k) {
    double lik = 0.0;
    const bool below = row && lane > k;
    if (active) {
      const double akk = A[k * ld + k];
      f.ok = f.ok && (akk > 0.0) && (akk < std::numeric_limits<double>::infinity());
      const double rd = 1.0 / sqrt(akk);
      if (below) {
        lik = A[k * ld + lane] * rd;
        A[k * ld + lane] = lik;
      }
      const double wk = gp_bcast(r, k) * rd;
      f.q = fma(wk, wk, f.q);
      if (lane == k) {
        f.w = wk; f.rinv = rd; f.piv = akk;
      }
      if (below) r = fma(-lik, wk, r);
    }
    __syncthreads();
    // Trailing update.  Lanes above the diagonal (lane < j) update slots of the unused upper triangle (zeroed by the build)
    // rather than branch per column: no lower-triangle slot is touched by a lane that does not own it, and no result is ever
    // computed from an upper-triangle slot (gp_predict_kernel drops them with a select).
    // Four columns per trip, loads first: the eight LDS reads are in flight together (a column belongs to one j only).
    if (row) {
      const double* __restrict__ pk = A + k * ld;
      int j = k + 1;
      for (; j + 3 < n; j += 4) {
        double* c0 = A + j * ld + lane;
        const double l0 = pk[j], l1 = pk[j + 1], l2 = pk[j + 2], l3 = pk[j + 3];
        const double a0 = c0[0], a1 = c0[ld], a2 = c0[2 * ld], a3 = c0[3 * ld];
        c0[0] = fma(-lik, l0, a0);
        c0[ld] = fma(-lik, l1, a1);
        c0[2 * ld] = fma(-lik, l2, a2);
        c0[3 * ld] = fma(-lik, l3, a3);
      }
      for (; j < n; ++j) A[j * ld + lane] = fma(-lik, pk[j], A[j * ld + lane]);
    }
    __syncthreads();
  }
  return f;
}

__global__ void __launch_bounds__(GP_WAVE)
gp_mll_kernel(GpDev g, const double* __restrict__ theta, int64_t W, double* __restrict__ out, double* __restrict__ parts) {
  extern __shared__ __attribute__((aligned(16))) double gp_smem[];
  const int64_t row = blockIdx.x;
  if (row >= W) return;
  const GpHyper h = gp_hyper(g, theta + row * CF_GP_NDIM);
  const int lane = threadIdx.x;
  if (!h.inbox) {  // not evaluated
    if (lane == 0) {
      out[row] = -std::numeric_limits<double>::infinity();
      if (parts) parts[2 * row] = parts[2 * row + 1] = __builtin_nan("");
    }
    return;
  }
  double* A = gp_smem;
  double* zs = gp_smem + (size_t)g.ld * g.n;
  const GpFactor f = gp_build_factor(g, h, A, zs);
  const double lg = lane < g.n ? log(f.piv) : 0.0;
  double logdet = 0.0;
  for (int k = 0; k < g.n; ++k) logdet += gp_bcast(lg, k);
  if (lane == 0) {
    double v = -0.5 * f.q - 0.5 * logdet - 0.5 * (double)g.n * 1.8378770664093454835606594728112;  // log(2 pi)
    if (!f.ok || !(v == v)) v = -std::numeric_limits<double>::infinity();
    out[row] = v;
    if (parts) {
      parts[2 * row] = f.ok ? f.q : __builtin_nan("");
      parts[2 * row + 1] = f.ok ? logdet : __builtin_nan("");
    }
    if (!f.ok) atomicAdd(g.fail_count, 1ull);
  }
}

__global__ void __launch_bounds__(GP_PRED_TPB)
gp_predict_kernel(GpDev g, const double* __restrict__ theta, int64_t S, const double* __restrict__ zstar, int nz, double noise,
                  double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double gp_smem[];
  __shared__ double ws[GP_WAVE], rinvs[GP_WAVE];
  __shared__ int ok_s;
  const int64_t row = blockIdx.x;
  if (row >= S) return;
  const GpHyper h = gp_hyper(g, theta + row * CF_GP_NDIM);
  const int tid = threadIdx.x, lane = tid & (GP_WAVE - 1), wave = tid >> 6, n = g.n, ld = g.ld;
  double* o = out + row * (int64_t)nz * 5;
  const int64_t n_out = (int64_t)nz * 5;
  if (!h.inbox) {
    for (int64_t k = tid; k < n_out; k += GP_PRED_TPB) o[k] = __builtin_nan("");
    return;
  }
  double* A = gp_smem;
  double* zs = gp_smem + (size_t)ld * n;
  const GpFactor f = gp_build_factor(g, h, A, zs);
  if (tid < GP_WAVE) {
    ws[lane] = f.w;
    rinvs[lane] = f.rinv;
    if (lane == 0) ok_s = f.ok ? 1 : 0;
  }
  __syncthreads();
  if (!ok_s) {
    for (int64_t k = tid; k < n_out; k += GP_PRED_TPB) o[k] = __builtin_nan("");
    return;
  }
  const bool rowl = lane < n;
  const double w = rowl ? ws[lane] : 0.0, rinv = rowl ? rinvs[lane] : 0.0;
  const double zi = rowl ? zs[lane] : 0.0;
  const double inv_l2 = 1.0 / (h.ell * h.ell), c2 = -0.5 * inv_l2;
  for (int t = wave; t < nz; t += GP_PRED_TPB / GP_WAVE) {
    const double zt = zstar[t];
    double* ot = o + (int64_t)t * 5;
    if (!(fabs(zt) < std::numeric_limits<double>::infinity())) {
      if (lane < 5) ot[lane] = __builtin_nan("");
      continue;
    }
    const double dz = zi - zt;
    double bv = rowl ? h.sf2 * exp(c2 * (dz * dz)) : 0.0;  // k*_i
    double bu = bv * dz * inv_l2;                          // d k*_i / d z*
    double vv = 0.0, uu = 0.0, vu = 0.0, vw = 0.0, uw = 0.0;
    for (int k = 0; k < n; ++k) {
      // in bounds for every lane: (n - 1) ld + 63 < ld n + 64.  Lanes <= k read an upper-triangle slot (or, beyond n, the
      // next column / the z block): such a value must only ever be dropped by the select below, never multiplied in.
      const double a = A[k * ld + lane];
      const double col = (rowl && lane > k) ? a : 0.0;
      const double vk = gp_bcast(bv * rinv, k), uk = gp_bcast(bu * rinv, k), wk = gp_bcast(w, k);
      vv = fma(vk, vk, vv);
      uu = fma(uk, uk, uu);
      vu = fma(vk, uk, vu);
      vw = fma(vk, wk, vw);
      uw = fma(uk, wk, uw);
      bv = fma(-col, vk, bv);
      bu = fma(-col, uk, bu);
    }
    if (lane == 0) {
      ot[0] = h.m + vw;
      ot[1] = fma(h.s, noise, h.sf2 - vv);
      ot[2] = uw;
      ot[3] = h.sf2 * inv_l2 - uu;
      ot[4] = -vu;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------
static int gp_launch_mll(cf_gp* gp, const double* d_theta, int64_t W, double* d_out, double* d_parts, hipStream_t st) {
  const size_t lds = gp_lds_doubles(gp->d.n) * sizeof(double);
  // one workgroup per row: at most GP_LAUNCH_ROWS rows per grid, so that no grid nears the 2^32 threads a launch may hold
  for (int64_t r0 = 0; r0 < W; r0 += GP_LAUNCH_ROWS) {
    const int64_t m = std::min<int64_t>(GP_LAUNCH_ROWS, W - r0);
    hipLaunchKernelGGL(gp_mll_kernel, dim3((unsigned)m), dim3(GP_WAVE), lds, st, gp->d, d_theta + r0 * CF_GP_NDIM, m, d_out + r0,
                       d_parts ? d_parts + 2 * r0 : nullptr);
    if (int rc = cf_launch_status("cf_gp_mll_device")) return rc;
  }
  return CF_OK;
}

static int gp_launch_predict(cf_gp* gp, const double* d_theta, int64_t S, const double* d_z, int nz, double noise, double* d_out,
                             hipStream_t st) {
  const size_t lds = gp_lds_doubles(gp->d.n) * sizeof(double);
  for (int64_t r0 = 0; r0 < S; r0 += GP_LAUNCH_ROWS) {
    const int64_t m = std::min<int64_t>(GP_LAUNCH_ROWS, S - r0);
    hipLaunchKernelGGL(gp_predict_kernel, dim3((unsigned)m), dim3(GP_PRED_TPB), lds, st, gp->d, d_theta + r0 * CF_GP_NDIM, m, d_z, nz,
                       noise, d_out + r0 * (int64_t)nz * 5);
    if (int rc = cf_launch_status("cf_gp_predict_device")) return rc;
  }
  return CF_OK;
}

static bool gp_all_finite(const double* a, int64_t n) {
  for (int64_t k = 0; k < n; ++k)
    if (!std::isfinite(a[k])) return false;
  return true;
}

extern "C" int cf_gp_create(const cf_gp_desc* c, cf_gp** out) {
  // every argument check comes before the first HIP call: a machine without a GPU reports them the same
  if (!c || !out) return cf_set_error(CF_ERR_INVALID, "cf_gp_create: null argument");
  *out = nullptr;
  if (c->struct_size != (int32_t)sizeof(cf_gp_desc))
    return cf_set_error(CF_ERR_INVALID, "cf_gp_create: struct_size does not match sizeof(cf_gp_desc)");
  if (c->n < 1 || c->n > CF_GP_MAX_N)
    return cf_set_error(CF_ERR_INVALID, "cf_gp_create: n = " + std::to_string(c->n) + " is outside 1.." + std::to_string(CF_GP_MAX_N));
  if (!c->z || !c->y || !c->cov || !c->bounds) return cf_set_error(CF_ERR_INVALID, "cf_gp_create: null data pointer (z, y, cov, bounds)");
  const int n = c->n;
  if (!gp_all_finite(c->z, n)) return cf_set_error(CF_ERR_INVALID, "cf_gp_create: z has a non-finite entry");
  if (!gp_all_finite(c->y, n)) return cf_set_error(CF_ERR_INVALID, "cf_gp_create: y has a non-finite entry");
  if (!gp_all_finite(c->cov, (int64_t)n * n)) return cf_set_error(CF_ERR_INVALID, "cf_gp_create: cov has a non-finite entry");
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j) {
      const double a = c->cov[i * n + j], b = c->cov[j * n + i];
      if (std::fabs(a - b) > 1e-12 * std::max(std::fabs(a), std::fabs(b)))
        return cf_set_error(CF_ERR_INVALID, "cf_gp_create: cov is not symmetric at (" + std::to_string(i) + ", " + std::to_string(j) +
                                                ") to 1e-12 relative");
    }
  for (int k = 0; k < CF_GP_NDIM; ++k) {
    const double lo = c->bounds[2 * k], hi = c->bounds[2 * k + 1];
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi))
      return cf_set_error(CF_ERR_INVALID, "cf_gp_create: bounds[" + std::to_string(k) + "] must be finite with lo < hi");
  }
  // s_f^2, l and s divide or scale the kernel: their boxes must keep them positive
  for (int k = 1; k < CF_GP_NDIM; ++k)
    if (!(c->bounds[2 * k] >= 0.0))
      return cf_set_error(CF_ERR_INVALID, "cf_gp_create: bounds[" + std::to_string(k) + "] must have lo >= 0 (output scale, length scale, noise scale)");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
    return cf_set_error(CF_ERR_NO_DEVICE, "cf_gp_create: no HIP device visible (there is no CPU implementation to fall back to)");
  if (c->device < 0 || c->device >= count)
    return cf_set_error(CF_ERR_INVALID, "cf_gp_create: device " + std::to_string(c->device) + " of " + std::to_string(count));
  cf_gp* gp = new cf_gp();
  gp->device = c->device;
  auto bail = [&](int code) { cf_gp_destroy(gp); return code; };
  DeviceScope on_device(gp->device);
  if (on_device.err != hipSuccess) return bail(cf_set_error(CF_ERR_HIP, "cf_gp_create: hipSetDevice failed"));
  const size_t nd = (size_t)2 * n + (size_t)n * n;
  if (gp->buf.ensure((nd + 1) * 8)) return bail(cf_set_error(CF_ERR_HIP, "cf_gp_create: hipMalloc failed"));
  std::vector<double> host(nd + 1, 0.0);
  std::copy(c->z, c->z + n, host.begin());
  std::copy(c->y, c->y + n, host.begin() + n);
  std::copy(c->cov, c->cov + (size_t)n * n, host.begin() + 2 * n);
  if (hipMemcpy(gp->buf.p, host.data(), (nd + 1) * 8, hipMemcpyHostToDevice) != hipSuccess)
    return bail(cf_set_error(CF_ERR_HIP, "cf_gp_create: hipMemcpy failed"));
  if (hipStreamCreateWithFlags(&gp->stream, hipStreamNonBlocking) != hipSuccess)
    return bail(cf_set_error(CF_ERR_HIP, "cf_gp_create: hipStreamCreate failed"));
  double* base = gp->buf.as<double>();
  gp->d.z = base;
  gp->d.y = base + n;
  gp->d.C = base + 2 * n;
  gp->d.fail_count = (unsigned long long*)(base + nd);
  gp->d.n = n;
  gp->d.ld = gp_ld(n);
  for (int k = 0; k < CF_GP_NDIM; ++k) {
    gp->d.lo[k] = c->bounds[2 * k];
    gp->d.hi[k] = c->bounds[2 * k + 1];
  }
  *out = gp;
  return CF_OK;
}

extern "C" void cf_gp_destroy(cf_gp* gp) {
  if (!gp) return;
  DeviceScope on_device(gp->device);
  if (gp->stream) {
    (void)hipStreamSynchronize(gp->stream);
    (void)hipStreamDestroy(gp->stream);
  }
  delete gp;  // frees buf
}

extern "C" int cf_gp_get_info(cf_gp* gp, cf_gp_info* info) {
  if (!gp || !info) return cf_set_error(CF_ERR_INVALID, "cf_gp_get_info: null argument");
  std::lock_guard<std::mutex> lk(gp->mu);
  DeviceScope on_device(gp->device);
  HIP_TRY(on_device.err);
  unsigned long long cnt = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&cnt, gp->d.fail_count, 8, hipMemcpyDeviceToHost));
  info->n = gp->d.n;
  info->device = gp->device;
  info->ld = gp->d.ld;
  info->lds_bytes = (int32_t)(gp_lds_doubles(gp->d.n) * sizeof(double));
  info->failed_factorizations = (int64_t)cnt;
  return CF_OK;
}

static int gp_check_rows(const cf_gp* gp, int64_t rows, const char* fn) {
  if (!gp) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": null argument");
  if (rows < 0 || rows > GP_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": row count out of range");
  return CF_OK;
}

static int gp_check_predict(int32_t nz, double noise, const char* fn) {
  if (nz < 1 || nz > CF_GP_MAX_NZ)
    return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": nz must be in 1.." + std::to_string(CF_GP_MAX_NZ));
  if (!std::isfinite(noise) || noise < 0.0) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": noise must be finite and >= 0");
  return CF_OK;
}

extern "C" int cf_gp_mll_device(cf_gp* gp, const double* d_theta, int64_t W, double* d_out, double* d_parts, void* hip_stream) {
  int rc = gp_check_rows(gp, W, "cf_gp_mll_device");
  if (rc) return rc;
  if (W == 0) return CF_OK;
  if (!d_theta || !d_out) return cf_set_error(CF_ERR_INVALID, "cf_gp_mll_device: null argument");
  DeviceScope on_device(gp->device);
  HIP_TRY(on_device.err);
  return gp_launch_mll(gp, d_theta, W, d_out, d_parts, (hipStream_t)hip_stream);
}

extern "C" int cf_gp_predict_device(cf_gp* gp, const double* d_theta, int64_t S, const double* d_zstar, int32_t nz, double noise,
                                    double* d_out, void* hip_stream) {
  int rc = gp_check_rows(gp, S, "cf_gp_predict_device");
  if (rc) return rc;
  if ((rc = gp_check_predict(nz, noise, "cf_gp_predict_device"))) return rc;
  if (S == 0) return CF_OK;
  if (!d_theta || !d_zstar || !d_out) return cf_set_error(CF_ERR_INVALID, "cf_gp_predict_device: null argument");
  DeviceScope on_device(gp->device);
  HIP_TRY(on_device.err);
  return gp_launch_predict(gp, d_theta, S, d_zstar, nz, noise, d_out, (hipStream_t)hip_stream);
}

// Host-buffer twins: rows in chunks through temporary device buffers on the handle's own stream.
extern "C" int cf_gp_mll(cf_gp* gp, const double* theta, int64_t W, double* out, double* parts) {
  int rc = gp_check_rows(gp, W, "cf_gp_mll");
  if (rc) return rc;
  if (W == 0) return CF_OK;
  if (!theta || !out) return cf_set_error(CF_ERR_INVALID, "cf_gp_mll: null argument");
  std::lock_guard<std::mutex> lk(gp->mu);
  DeviceScope on_device(gp->device);
  HIP_TRY(on_device.err);
  RowStage rows(gp->stream, std::min<int64_t>(W, GP_HOST_CHUNK));
  const double* dth = rows.in(theta, CF_GP_NDIM * 8);
  double* dout = rows.out(out, 8);
  double* dparts = rows.out(parts, 16);
  return rows.run(W, [&](int64_t, int64_t m) { return gp_launch_mll(gp, dth, m, dout, dparts, gp->stream); });
}

extern "C" int cf_gp_predict(cf_gp* gp, const double* theta, int64_t S, const double* zstar, int32_t nz, double noise, double* out) {
  int rc = gp_check_rows(gp, S, "cf_gp_predict");
  if (rc) return rc;
  if ((rc = gp_check_predict(nz, noise, "cf_gp_predict"))) return rc;
  if (S == 0) return CF_OK;
  if (!theta || !zstar || !out) return cf_set_error(CF_ERR_INVALID, "cf_gp_predict: null argument");
  std::lock_guard<std::mutex> lk(gp->mu);
  DeviceScope on_device(gp->device);
  HIP_TRY(on_device.err);
  const int64_t per_row = (int64_t)nz * 5;
  RowStage rows(gp->stream, std::min<int64_t>(S, std::max<int64_t>(1, ((int64_t)GP_HOST_CHUNK * 256) / per_row)));
  const double* dth = rows.in(theta, CF_GP_NDIM * 8);
  double* dout = rows.out(out, (size_t)per_row * 8);
  DevBuf dz;
  if (dz.ensure((size_t)nz * 8)) return CF_ERR_HIP;
  HIP_TRY(hipMemcpyAsync(dz.p, zstar, (size_t)nz * 8, hipMemcpyHostToDevice, gp->stream));
  return rows.run(S, [&](int64_t, int64_t m) {
    return gp_launch_predict(gp, dth, m, dz.as<const double>(), nz, noise, dout, gp->stream);
  });
}
