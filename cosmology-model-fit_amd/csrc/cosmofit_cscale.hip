// cosmofit_cscale.hip — a free amplitude on the SN covariance, C(s) = C0 + s C1, without refactorising (include/cosmofit.h:
// cf_cscale_apply_device, cf_cscale_eval_device; the kernels, then the host side; the driver is
// cosmology-model-fit_amd/covscale.py).
//
// With C0 = L0 L0^T the factor the engine holds, A = L0^-1 C1 L0^-T = Q diag(lambda) Q^T and T = Q^T L0^-1 (both formed once on
// the host), a residual row r gives y = T r and
//   quad(s)   = r^T C(s)^-1 r      = sum_k y_k^2 / (1 + s lambda_k)
//   logdet(s) = ln|C(s)| - ln|C0|  = sum_k log1p(s lambda_k)
// valid while 1 + s lambda_k > 0 for every k.
//
// cscale_gemm_kernel: Y[S, n] = R[S, n] M[n, n], M = T^T, on FP64 matrix cores: the tiling, the LDS staging and the operand maps
// of prec_gemm_kernel (cosmofit_infl.hip: lane l holds A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15], result register r of the
// lane is D[(l>>4) + 4 r][l&15]; a workgroup of four waves owns a 64 x 64 block, wave (wr, wc) its 32 x 32 quarter as 2 x 2
// tiles).  ONE accumulator per output and an ascending k loop over ceil(n / 32) * 32 columns whatever S is, so an element of Y
// depends on its row of R and on M only.  Rows >= S and columns >= n of R are never read (a select, not a product with zero).
// Y is NOT written unless the caller asks for it: the epilogue forms, per row, per SLAB (the 32 columns of a wave) and per
// amplitude j, sum_k y_k^2 / (1 + s_j lambda_k) in a fixed order -- the lane's two tiles (u = 0, then u = 1), then the xor
// butterfly (8, 4, 2, 1) over the 16 lanes that hold the row -- and stores that one partial at part[(row * n_slab + slab) * n_s + j].
//
// cscale_row_kernel: ONE WAVE PER ROW, four rows per 256-thread workgroup (the form of infl_row_kernel).  Per amplitude j the
// wave forms sum_k log1p(s_j lambda_k) as lane-strided partials (lane l takes k = l, l + 64, ...) combined by the fixed xor
// butterfly (32, 16, .., 1) and notes whether any 1 + s_j lambda_k failed to be > 0; lane j then sums the row's slab partials
// in ascending slab order, applies the domain rule and combines with the engine's values.  No atomics, no LDS, and nothing
// depends on the launch geometry: the outputs of (row, s_j) depend on the row's residuals, s_j, T and lambda only.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950): see profiles/NOTES_cscale.md; scratch is 0 in both kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_handle.h"
#include "cf_wave.h"
#include "cosmofit_resid.h"

typedef double d4 __attribute__((ext_vector_type(4)));

#define CG_TPB 256
#define CG_BM 64
#define CG_BN 64
#define CG_BK 32
#define CG_SLAB 32          // columns per quad partial: a wave's share of the block
#define CG_RP (CG_BK + 2)   // LDS pitch of a staged R row
#define CG_MP (CG_BN + 16)  // LDS pitch of a staged M row
#define CSCALE_MAX_N 32768

// ---- the arithmetic both sides share: the device kernels and cf_selftest_cscale_host run these same functions -----------------
// one term of quad: y^2 / (1 + s lambda), the denominator one fused multiply-add
__host__ __device__ static inline double cscale_quad_term(double y, double s, double lam) { return (y * y) / fma(s, lam, 1.0); }

// one term of logdet, and whether the amplitude leaves the domain at this eigenvalue
__host__ __device__ static inline double cscale_log_term(double s, double lam, bool* bad) {
  *bad = *bad || !(fma(s, lam, 1.0) > 0.0);
  return log1p(s * lam);
}

// the domain rule on (quad, logdet): a non-finite amplitude or one outside the domain gives NaN in both
__host__ __device__ static inline void cscale_domain(double s, bool bad, double* quad, double* logdet) {
  if (bad || !(fabs(s) <= 1.79769313486231570815e308)) *quad = *logdet = NAN;
}

// The value of kind `out_kind` from the engine's own value `e` of that kind, the SN chi^2 `c0` the engine computed with C0, and
// (quad, logdet) after the domain rule.  theta_ok: every entry of the row's theta is finite.
__host__ __device__ static inline double cscale_combine(int out_kind, double e, double c0, double quad, double logdet, double s,
                                                        bool bad, bool theta_ok) {
  if (!theta_ok || !(fabs(s) <= 1.79769313486231570815e308)) return NAN;
  if (out_kind == CF_OUT_CHI2) return bad ? NAN : (e - c0) + quad;
  if (bad || e == -INFINITY) return -INFINITY;  // outside the domain, or where the engine itself says -inf (the prior box, a NaN chi^2)
  return e + 0.5 * c0 - 0.5 * (quad + logdet);
}

__global__ void __launch_bounds__(CG_TPB)
cscale_gemm_kernel(const double* __restrict__ R, int64_t pitch, int n, int64_t S, const double* __restrict__ M, int64_t kp,
                   const double* __restrict__ lam, const double* __restrict__ amp, int n_s, int n_slab, double* __restrict__ part,
                   double* __restrict__ Y) {
  __shared__ double Rs[CG_BM * CG_RP];
  __shared__ double Ms[CG_BK * CG_MP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * CG_BM;
  const int col0 = blockIdx.y * CG_BN;
  // staging: thread t fetches R[row0 + (t>>5) + 8 j][k0 + (t&31)] and M[k0 + (t>>6) + 4 j][col0 + (t&63)], j < 8
  const int rk = tid & 31, rr = tid >> 5;
  const int kc = tid & 63, kr = tid >> 6;
  double rreg[8], mreg[8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t row = row0 + rr + 8 * j;
      const int k = k0 + rk;
      rreg[j] = (row < S && k < n) ? R[row * pitch + k] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + kr + 4 * j, c = col0 + kc;
      mreg[j] = (k < kp && c < kp) ? M[(int64_t)k * kp + c] : 0.0;
    }
  };
  const int wr = wave >> 1, wc = wave & 1;
  const double* a_lds = Rs + (32 * wr + (lane & 15)) * CG_RP + (lane >> 4);
  const double* b_lds = Ms + (lane >> 4) * CG_MP + 32 * wc + (lane & 15);
  d4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
  const int n_tiles = (n + CG_BK - 1) / CG_BK;
  fetch(0);
  for (int tile = 0; tile < n_tiles; ++tile) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Rs[(rr + 8 * j) * CG_RP + rk] = rreg[j];
      Ms[(kr + 4 * j) * CG_MP + kc] = mreg[j];
    }
    __syncthreads();
    if (tile + 1 < n_tiles) fetch((tile + 1) * CG_BK);
#pragma unroll
    for (int kk = 0; kk < CG_BK; kk += 4) {
      const double a0 = a_lds[kk], a1 = a_lds[16 * CG_RP + kk];
      const double b0 = b_lds[kk * CG_MP], b1 = b_lds[kk * CG_MP + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // ---- epilogue: y on request, and the slab's share of quad for every amplitude of the row ----
  const int c0 = col0 + 32 * wc + (lane & 15), c1 = c0 + 16;
  const bool live0 = c0 < n, live1 = c1 < n;
  if (Y) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 32 * wr + 16 * t + (lane >> 4) + 4 * r;
        if (row < S && live0) Y[row * n + c0] = acc[t][0][r];
        if (row < S && live1) Y[row * n + c1] = acc[t][1][r];
      }
  }
  if (!part || col0 + 32 * wc >= n) return;  // wave-uniform: a slab wholly beyond n has no partial
  const double lam0 = live0 ? lam[c0] : 0.0, lam1 = live1 ? lam[c1] : 0.0;
  const int slab = 2 * (int)blockIdx.y + wc;
  for (int j = 0; j < n_s; ++j) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 32 * wr + 16 * t + (lane >> 4) + 4 * r;
        const bool in = row < S;
        const double s = in ? amp[row * n_s + j] : 0.0;
        double q = live0 ? cscale_quad_term(acc[t][0][r], s, lam0) : 0.0;
        q += live1 ? cscale_quad_term(acc[t][1][r], s, lam1) : 0.0;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) q += __shfl_xor(q, m);
        if (in && (lane & 15) == 0) part[(row * n_slab + slab) * n_s + j] = q;
      }
  }
}

#define CR_TPB 256
#define CR_ROWS_PER_WG (CR_TPB / 64)

struct cf_cscale_row_args {
  const double* part;   // [rows][n_slab][n_s]
  const double* lam;    // [n]
  const double* amp;    // [rows][n_s]
  const double* theta;  // [rows][ndim], or null (cf_cscale_apply_device: no engine values)
  const double* eng;    // [rows] the engine's value of kind out_kind
  const double* c0;     // [rows] the engine's SN chi^2
  double* out;          // [rows][n_s] or null
  double* quad;         // [rows][n_s] or null
  double* logdet;       // [rows][n_s] or null
  double* parts;        // [rows][n_s][2] or null
  int32_t n, n_s, n_slab, ndim, out_kind;
};

__global__ void __launch_bounds__(CR_TPB) cscale_row_kernel(int64_t rows, cf_cscale_row_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * CR_ROWS_PER_WG + (threadIdx.x >> 6);
  if (row >= rows) return;  // whole waves leave: no cross-lane step below has a missing partner
  const double* __restrict__ amp = a.amp + row * a.n_s;
  double my_s = 0.0, my_logdet = 0.0;
  bool my_bad = false;
  for (int j = 0; j < a.n_s; ++j) {
    const double s = amp[j];
    double ld = 0.0;
    bool bad = false;
    for (int k = lane; k < a.n; k += 64) ld += cscale_log_term(s, a.lam[k], &bad);
    ld = wave_sum(ld);
    bad = __any(bad);
    if (lane == j) { my_s = s; my_logdet = ld; my_bad = bad; }
  }
  bool theta_ok = true;
  if (a.theta) {
    const double t = lane < a.ndim ? a.theta[row * a.ndim + lane] : 0.0;
    theta_ok = !__any(!(fabs(t) <= 1.79769313486231570815e308));
  }
  if (lane >= a.n_s) return;
  const double* __restrict__ p = a.part + row * a.n_slab * (int64_t)a.n_s + lane;
  double quad = 0.0;
  for (int b = 0; b < a.n_slab; ++b) quad += p[(int64_t)b * a.n_s];
  cscale_domain(my_s, my_bad, &quad, &my_logdet);
  const int64_t o = row * a.n_s + lane;
  if (a.quad) a.quad[o] = quad;
  if (a.logdet) a.logdet[o] = my_logdet;
  if (a.parts) { a.parts[2 * o] = quad; a.parts[2 * o + 1] = my_logdet; }
  if (a.out) a.out[o] = cscale_combine(a.out_kind, a.eng[row], a.c0[row], quad, my_logdet, my_s, my_bad, theta_ok);
}

// ------------------------------------------------------------------------------------------------
// Host side.
// ------------------------------------------------------------------------------------------------
struct cf_cscale {
  int64_t n = 0, kp = 0;  // kp: row pitch of M on the device, n rounded up to 16 (zero in the padding)
  int device = 0;
  DevBuf M, lam;
  // the ONE scratch of the slab partials is shared by every call on this object: a call on another stream than the previous one
  // first waits, on the host, for the device (as a handle's workspace: the caller's stream is compared, never passed back to HIP)
  DevBuf part;
  std::mutex mu;
  hipStream_t last_stream = nullptr;
  bool has_last = false;
};

static inline int cscale_slabs(int64_t n) { return (int)((n + CG_SLAB - 1) / CG_SLAB); }

extern "C" int cf_selftest_cscale_host(const double* y, const double* lambda, int64_t n, const double* s, int32_t n_s, double* quad,
                                       double* logdet) {
  const std::string F = "cf_selftest_cscale_host: ";
  if (!y || !lambda || !s) return cf_set_error(CF_ERR_INVALID, F + "null argument");
  if (n < 1 || n > CSCALE_MAX_N) return cf_set_error(CF_ERR_INVALID, F + "n must be in 1..32768");
  if (n_s < 1 || n_s > CF_CSCALE_MAX_S) return cf_set_error(CF_ERR_INVALID, F + "n_s must be in 1..16");
  const int n_slab = cscale_slabs(n);
  for (int j = 0; j < n_s; ++j) {
    // quad: per slab the 16 lanes of a row, each its two tiles, then the butterfly (8, 4, 2, 1); the slabs in ascending order
    double q = 0.0;
    for (int b = 0; b < n_slab; ++b) {
      double v[16];
      for (int l = 0; l < 16; ++l) {
        const int64_t c0 = (int64_t)b * CG_SLAB + l, c1 = c0 + 16;
        v[l] = c0 < n ? cscale_quad_term(y[c0], s[j], lambda[c0]) : 0.0;
        v[l] += c1 < n ? cscale_quad_term(y[c1], s[j], lambda[c1]) : 0.0;
      }
      for (int m = 8; m >= 1; m >>= 1) {
        double w[16];
        for (int l = 0; l < 16; ++l) w[l] = v[l] + v[l ^ m];
        memcpy(v, w, sizeof v);
      }
      q += v[0];
    }
    // logdet: 64 lane-strided partials, then the butterfly (32, .., 1) of wave_sum (cf_wave.h), written out on the host
    double v[64];
    bool bad = false;
    for (int l = 0; l < 64; ++l) {
      v[l] = 0.0;
      for (int64_t k = l; k < n; k += 64) v[l] += cscale_log_term(s[j], lambda[k], &bad);
    }
    for (int m = 32; m >= 1; m >>= 1) {
      double w[64];
      for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ m];
      memcpy(v, w, sizeof v);
    }
    double ld = v[0];
    cscale_domain(s[j], bad, &q, &ld);
    if (quad) quad[j] = q;
    if (logdet) logdet[j] = ld;
  }
  return CF_OK;
}

extern "C" int cf_cscale_create(const double* T, int64_t n, int64_t ld, const double* lambda, int32_t device, cf_cscale** out) {
  const std::string F = "cf_cscale_create: ";
  if (!out) return cf_set_error(CF_ERR_INVALID, F + "null argument");
  *out = nullptr;
  if (!T || !lambda) return cf_set_error(CF_ERR_INVALID, F + "null argument");
  if (n < 1 || n > CSCALE_MAX_N) return cf_set_error(CF_ERR_INVALID, F + "n must be in 1..32768");
  if (ld < n) return cf_set_error(CF_ERR_INVALID, F + "ld < n");
  const int64_t kp = (n + 15) / 16 * 16;
  std::vector<double> Mp((size_t)kp * kp, 0.0);
  for (int64_t k = 0; k < n; ++k) {
    if (!std::isfinite(lambda[k])) return cf_set_error(CF_ERR_INVALID, F + "a non-finite eigenvalue");
    for (int64_t i = 0; i < n; ++i) {
      const double v = T[k * ld + i];
      if (!std::isfinite(v)) return cf_set_error(CF_ERR_INVALID, F + "a non-finite entry of T");
      Mp[(size_t)i * kp + k] = v;  // M = T^T
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return cf_set_error(CF_ERR_NO_DEVICE, F + "no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return cf_set_error(CF_ERR_INVALID, F + "device ordinal out of range");
  std::unique_ptr<cf_cscale> p(new cf_cscale());
  p->n = n;
  p->kp = kp;
  p->device = device;
  DeviceScope on_device(device);
  HIP_TRY(on_device.err);
  int rc;
  if ((rc = upload(p->M, Mp.data(), (int64_t)Mp.size()))) return rc;
  if ((rc = upload(p->lam, lambda, n))) return rc;
  *out = p.release();
  return CF_OK;
}

extern "C" void cf_cscale_destroy(cf_cscale* p) {
  if (!p) return;
  DeviceScope on_device(p->device);
  delete p;
}

extern "C" int cf_cscale_look(const cf_cscale* p, int64_t* n, int32_t* device) {
  if (!p) return cf_set_error(CF_ERR_INVALID, "cf_cscale_look: null cf_cscale");
  if (n) *n = p->n;
  if (device) *device = p->device;
  return CF_OK;
}

// The scratch for chunks of `rows` rows, and the order behind the previous call.  p->mu held, p's device current.
static int cscale_prepare(cf_cscale* p, int64_t rows, int32_t n_s, hipStream_t st) {
  const size_t need = (size_t)rows * (size_t)cscale_slabs(p->n) * (size_t)n_s * 8;
  const bool grow = need > p->part.bytes;
  if (grow || (p->has_last && p->last_stream != st)) HIP_TRY(hipDeviceSynchronize());
  if (grow && p->part.ensure(need)) return CF_ERR_HIP;
  p->last_stream = st;
  p->has_last = true;
  return 0;
}

// One chunk: m rows at d_rows (row pitch `pitch`), their amplitudes, and the row kernel's arguments already offset to the chunk.
static int cscale_chunk(cf_cscale* p, const double* d_rows, int64_t pitch, int64_t m, int32_t n_s, double* d_y,
                        cf_cscale_row_args a, hipStream_t st, const char* fn) {
  const int n = (int)p->n, n_slab = cscale_slabs(p->n);
  const bool need_row = a.out || a.quad || a.logdet || a.parts;
  const dim3 grid((unsigned)((m + CG_BM - 1) / CG_BM), (unsigned)((n + CG_BN - 1) / CG_BN));
  hipLaunchKernelGGL(cscale_gemm_kernel, grid, dim3(CG_TPB), 0, st, d_rows, pitch, n, m, p->M.as<const double>(), p->kp,
                     p->lam.as<const double>(), a.amp, (int)n_s, n_slab, need_row ? p->part.as<double>() : nullptr, d_y);
  if (int rc = cf_launch_status(fn)) return rc;
  if (!need_row) return CF_OK;
  a.part = p->part.as<const double>();
  a.lam = p->lam.as<const double>();
  a.n = n;
  a.n_s = n_s;
  a.n_slab = n_slab;
  hipLaunchKernelGGL(cscale_row_kernel, dim3((unsigned)((m + CR_ROWS_PER_WG - 1) / CR_ROWS_PER_WG)), dim3(CR_TPB), 0, st, m, a);
  return cf_launch_status(fn);
}

extern "C" int cf_cscale_apply_device(cf_cscale* p, const double* d_rows, int64_t pitch, int64_t S, const double* d_s, int32_t n_s,
                                      double* d_quad, double* d_logdet, double* d_y, void* hip_stream) {
  const std::string F = "cf_cscale_apply_device: ";
  if (!p) return cf_set_error(CF_ERR_INVALID, F + "null cf_cscale");
  if (S < 0 || S > CF_RESID_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, F + "S out of range");
  if (n_s < 1 || n_s > CF_CSCALE_MAX_S) return cf_set_error(CF_ERR_INVALID, F + "n_s must be in 1..16");
  if (pitch < p->n) return cf_set_error(CF_ERR_INVALID, F + "a pitch below n");
  if (!d_quad && !d_logdet && !d_y) return cf_set_error(CF_ERR_INVALID, F + "no output requested");
  if (S == 0) return CF_OK;
  if (!d_rows || !d_s) return cf_set_error(CF_ERR_INVALID, F + "null rows or amplitudes");
  std::lock_guard<std::mutex> lock(p->mu);
  DeviceScope on_device(p->device);
  HIP_TRY(on_device.err);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t chunk = std::min<int64_t>(S, CF_CSCALE_CHUNK);
  int rc;
  if ((rc = cscale_prepare(p, chunk, n_s, st))) return rc;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t m = std::min(chunk, S - s0);
    cf_cscale_row_args a{};
    a.amp = d_s + s0 * n_s;
    a.quad = d_quad ? d_quad + s0 * n_s : nullptr;
    a.logdet = d_logdet ? d_logdet + s0 * n_s : nullptr;
    if ((rc = cscale_chunk(p, d_rows + s0 * pitch, pitch, m, n_s, d_y ? d_y + s0 * p->n : nullptr, a, st, "cf_cscale_apply_device")))
      return rc;
  }
  return CF_OK;
}

extern "C" int cf_cscale_check_args(int64_t n_sn, int32_t is_quasar, int32_t n_devices, int32_t handle_device, int32_t has_cscale,
                                    int64_t cscale_n, int32_t cscale_device, const void* theta, const void* s, int32_t n_s, int64_t S,
                                    int32_t out_kind, const void* out, const void* parts) {
  const std::string F = "cf_cscale: ";
  if (is_quasar) return cf_set_error(CF_ERR_INVALID, F + "a quasar handle has no accessor path to take the residuals from");
  if (n_devices > 1) return cf_set_error(CF_ERR_INVALID, F + "this handle spans several devices; use one handle per device");
  if (n_sn < 1) return cf_set_error(CF_ERR_INVALID, F + "this handle has no SN block");
  if (!has_cscale) return cf_set_error(CF_ERR_INVALID, F + "null cf_cscale");
  if (cscale_n != n_sn) return cf_set_error(CF_ERR_INVALID, F + "cf_cscale.n is not the number of SNe of the handle");
  if (cscale_device != handle_device) return cf_set_error(CF_ERR_INVALID, F + "the cf_cscale lives on another device than the handle");
  if (S < 0 || S > CF_RESID_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, F + "S out of range");
  if (n_s < 1 || n_s > CF_CSCALE_MAX_S) return cf_set_error(CF_ERR_INVALID, F + "n_s must be in 1..16");
  if (out_kind != CF_OUT_CHI2 && out_kind != CF_OUT_LOGL && out_kind != CF_OUT_LOGP)
    return cf_set_error(CF_ERR_INVALID, F + "out_kind must be CF_OUT_CHI2, CF_OUT_LOGL or CF_OUT_LOGP");
  if (!out && !parts) return cf_set_error(CF_ERR_INVALID, F + "no output requested");
  if (S > 0 && !theta) return cf_set_error(CF_ERR_INVALID, F + "null theta");
  if (S > 0 && !s) return cf_set_error(CF_ERR_INVALID, F + "null amplitudes");
  return CF_OK;
}

static int cscale_check(cf_handle* h, cf_cscale* p, const void* theta, const void* s, int32_t n_s, int64_t S, int32_t out_kind,
                        const void* out, const void* parts) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_cscale: null handle");
  return cf_cscale_check_args(h->d.n_sn, h->qsr ? 1 : 0, 1 + (int32_t)h->peers.size(), h->device, p ? 1 : 0, p ? p->n : 0,
                              p ? p->device : 0, theta, s, n_s, S, out_kind, out, parts);
}

extern "C" int cf_cscale_set_chunk(cf_handle* h, int64_t rows) {
  return set_chunk(h, &cf_handle::cscale_chunk, rows, "cf_cscale_set_chunk");
}

// Arguments checked.  Device pointers throughout.  The residual rows come from the accessor path one chunk at a time exactly as
// infl_run gets them (rows at h->delta, pitch n_ld); the engine's value of the asked kind lands in h->out and its SN chi^2 in
// the fit report's r_snb, and the two kernels follow on the same stream.
static int cscale_run(const HandleScope& hs, cf_cscale* p, const double* d_theta, const double* d_s, int32_t n_s, int64_t S,
                      int32_t out_kind, double* d_out, double* d_parts, hipStream_t st) {
  cf_handle* const h = hs.h;
  int rc;
  const int64_t chunk = std::min<int64_t>(S, h->cscale_chunk > 0 ? h->cscale_chunk : CF_CSCALE_CHUNK);
  if ((rc = ensure_workspace(h, chunk))) return rc;
  if ((rc = resid_prepare(hs, chunk))) return rc;
  std::lock_guard<std::mutex> lock(p->mu);
  if ((rc = cscale_prepare(p, chunk, n_s, st))) return rc;
  const cf_dev_desc& d = h->d;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t m = std::min(chunk, S - s0);
    // a mu_corr buffer selects the accessor form of the per-walker kernel (residual rows in row layout), as in resid_run
    if ((rc = launch_path(h, d_theta + s0 * d.ndim, m, h->out.as<double>(), out_kind, st, nullptr, h->r_mc.as<double>(), nullptr,
                          d.n_bao > 0 ? h->r_bt.as<double>() : nullptr, h->r_snb.as<double>())))
      return rc;
    cf_cscale_row_args a{};
    a.amp = d_s + s0 * n_s;
    a.theta = d_theta + s0 * d.ndim;
    a.ndim = d.ndim;
    a.eng = h->out.as<const double>();
    a.c0 = h->r_snb.as<const double>();
    a.out_kind = out_kind;
    a.out = d_out ? d_out + s0 * n_s : nullptr;
    a.parts = d_parts ? d_parts + 2 * s0 * n_s : nullptr;
    if ((rc = cscale_chunk(p, h->delta.as<const double>(), (int64_t)d.n_ld, m, n_s, nullptr, a, st, "cf_cscale_eval_device"))) return rc;
  }
  return CF_OK;
}

extern "C" int cf_cscale_eval_device(cf_handle* h, cf_cscale* p, const double* d_theta, const double* d_s, int32_t n_s, int64_t S,
                                     int32_t out_kind, double* d_out, double* d_parts, void* hip_stream) {
  int rc = cscale_check(h, p, d_theta, d_s, n_s, S, out_kind, d_out, d_parts);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  return cscale_run(hs, p, d_theta, d_s, n_s, S, out_kind, d_out, d_parts, (hipStream_t)hip_stream);
}

// Host-buffer twin: rows in pieces through temporary device buffers on the handle's own stream.
#define CF_CSCALE_HOST_PIECE 4096

extern "C" int cf_cscale_eval(cf_handle* h, cf_cscale* p, const double* theta, const double* s, int32_t n_s, int64_t S,
                              int32_t out_kind, double* out, double* parts) {
  int rc = cscale_check(h, p, theta, s, n_s, S, out_kind, out, parts);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  RowStage rows(h->stream, std::min<int64_t>(S, CF_CSCALE_HOST_PIECE));
  const double* dth = rows.in(theta, (size_t)h->d.ndim * 8);
  const double* ds = rows.in(s, (size_t)n_s * 8);
  double* dout = rows.out(out, (size_t)n_s * 8);
  double* dparts = rows.out(parts, (size_t)n_s * 16);
  return rows.run(S, [&](int64_t, int64_t m) { return cscale_run(hs, p, dth, ds, n_s, m, out_kind, dout, dparts, h->stream); });
}
