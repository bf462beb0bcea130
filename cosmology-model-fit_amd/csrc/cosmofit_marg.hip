// cosmofit_marg.hip — linear SN nuisance parameters marginalised or profiled in closed form (include/cosmofit.h:
// cf_marg_apply_device, cf_marg_eval_device; the kernels, then the host side; the driver is
// cosmology-model-fit_amd/nuisance.py).
//
// The SN residual is r(theta, alpha) = r0(theta) - A alpha with constant templates A [n, m] (a column of ones: the absolute
// magnitude; a 0/1 mask: a per-survey offset; sn_lin_coef: the bulk-flow amplitude) and a prior N(mu_j, sigma_j) or flat on each
// alpha_j.  With P = diag(1 / sigma_j^2), K = C^-1 A, F = A^T K + P = L_F L_F^T, Wt = K L_F^-T, ct = L_F^-1 P mu, U = L_F^T and
// pmu = mu^T P mu (all formed once on the host, nuisance.project), a residual row r0 gives
//   t = Wt^T r0 + ct,  q = sum_j t_j^2,  alpha_hat = U^-1 t,  alpha_draw = U^-1 (t + xi)
//   chi2_prof = chi2_engine + pmu - q,   ln L_marg = ln L_engine + 0.5 q - 0.5 pmu + log_norm.
//
// marg_proj_kernel: T[S, 16] = R[S, n] Wt[n, 16] on FP64 matrix cores with the operand maps of prec_gemm_kernel /
// cscale_gemm_kernel (lane l holds A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15], result register r of the lane is
// D[(l>>4) + 4 r][l&15]).  The product is 0.2 GFLOP behind 56 MB of residual rows per 4096-row chunk at n = 1701, so the form is
// the one that streams the rows: a wave owns 16 rows and ONE k slice of MP_SLICE columns, reads its rows 64 consecutive doubles
// per load (lane = column), each element once, and stages them through LDS for the operand map; the four waves of a workgroup
// share the slice, so the 64 x 16 tile of Wt is staged once for the four.  The slice length is a compile-time constant: the grid
// is ceil(S / 64) x ceil(n / MP_SLICE) workgroups, 1792 waves at S = 4096, n = 1701.  A wave keeps ONE accumulator and an
// ascending k loop and stores its 16 x 16 partial at part[(row * n_slice + slice) * 16 + j]; rows >= S and columns >= n are
// never read (a select, not a product with zero), and Wt is zero-padded to 16 columns and to a multiple of 64 rows at creation.
//
// marg_row_kernel: SIXTEEN LANES PER ROW (lane j = component j), sixteen rows per 256-thread workgroup.  Lane j sums the row's
// slice partials in ascending slice order and adds ct_j; q is summed in ascending j by one lane-to-lane read per component; the
// back-substitution against U walks j = m - 1 .. 0; then the combination rule.  No atomics, no LDS, and nothing depends on the
// launch geometry: a row's outputs depend on its residuals (and its xi) and on the object only.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950): see profiles/NOTES_marg.md; scratch is 0 in both kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_handle.h"
#include "cosmofit_resid.h"

typedef double d4 __attribute__((ext_vector_type(4)));

#define MP_TPB 256
#define MP_WAVES (MP_TPB / 64)
#define MP_TILE 16                  // rows of a wave, and the padded number of components
#define MP_BK 64                    // columns per staged tile: one load of a wave along a row
#define MP_SLICE CF_MARG_SLICE      // columns per k slice
#define MP_RP (MP_BK + 2)           // LDS pitch of a staged residual row
#define MARG_MAX_N 32768

// ---- the arithmetic both sides share: marg_row_kernel and cf_selftest_marg_host run these same functions ----------------------
// q, one component at a time in ascending j
__host__ __device__ static inline double marg_q_step(double q, double t) { return fma(t, t, q); }

// one elimination of the back-substitution: v_i - U_ij alpha_j
__host__ __device__ static inline double marg_back_step(double v, double u, double a) { return fma(-u, a, v); }

// a row whose projection is not finite (a NaN or an inf among its residuals) has no t, q or alpha
__host__ __device__ static inline bool marg_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }

// whether the engine's value leaves the row without a conditional posterior: rejected (-inf) or NaN
__host__ __device__ static inline bool marg_dead(double e) { return e == -INFINITY || e != e; }

// The value of kind `out_kind` from the engine's own value `e` of that kind and the row's q.  mode 0: profiled, 1: marginalised.
// bad: the row's projection is not finite.
__host__ __device__ static inline double marg_combine(int out_kind, int mode, double e, double q, double pmu, double log_norm,
                                                      bool bad) {
  if (e != e) return NAN;
  if (out_kind == CF_OUT_CHI2) return bad ? NAN : (e + pmu) - q;
  if (e == -INFINITY) return e;  // outside the prior box, or a chi^2 the engine itself rejects: whatever the residuals hold
  if (bad) return NAN;
  const double v = (e + 0.5 * q) - 0.5 * pmu;
  return mode == CF_MARG_MARGINAL ? v + log_norm : v;
}

__global__ void __launch_bounds__(MP_TPB)
marg_proj_kernel(const double* __restrict__ R, int64_t pitch, int n, int64_t S, const double* __restrict__ Wt, int n_slice,
                 double* __restrict__ part) {
  __shared__ double Rs[MP_WAVES * MP_TILE * MP_RP];
  __shared__ double Ws[MP_BK * MP_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = ((int64_t)blockIdx.x * MP_WAVES + wave) * MP_TILE;
  const int slice = blockIdx.y;
  const int k_beg = slice * MP_SLICE;
  const int k_end = min(n, k_beg + MP_SLICE);  // workgroup-uniform: every wave makes the same trips to the barriers
  double rreg[MP_TILE], wreg[MP_TILE * MP_BK / MP_TPB];
  auto fetch = [&](int k0) {
    const int k = k0 + lane;
#pragma unroll
    for (int j = 0; j < MP_TILE; ++j) {
      const int64_t row = row0 + j;
      rreg[j] = (row < S && k < n) ? R[row * pitch + k] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < MP_TILE * MP_BK / MP_TPB; ++j) wreg[j] = Wt[(int64_t)k0 * MP_TILE + j * MP_TPB + tid];  // rows < n_pad
  };
  double* r_st = Rs + wave * (MP_TILE * MP_RP) + lane;
  const double* a_lds = Rs + wave * (MP_TILE * MP_RP) + (lane & 15) * MP_RP + (lane >> 4);
  const double* b_lds = Ws + (lane >> 4) * MP_TILE + (lane & 15);
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
  fetch(k_beg);
  for (int k0 = k_beg; k0 < k_end; k0 += MP_BK) {
#pragma unroll
    for (int j = 0; j < MP_TILE; ++j) r_st[j * MP_RP] = rreg[j];
#pragma unroll
    for (int j = 0; j < MP_TILE * MP_BK / MP_TPB; ++j) Ws[j * MP_TPB + tid] = wreg[j];
    __syncthreads();
    if (k0 + MP_BK < k_end) fetch(k0 + MP_BK);
#pragma unroll
    for (int kk = 0; kk < MP_BK; kk += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_lds[kk], b_lds[kk * MP_TILE], acc, 0, 0, 0);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + (lane >> 4) + 4 * r;
    if (row < S) part[(row * n_slice + slice) * MP_TILE + (lane & 15)] = acc[r];
  }
}

struct cf_marg_row_args {
  const double* part;  // [rows][n_slice][16]
  const double* ct;    // [16], zero beyond m
  const double* U;     // [m][m], the upper triangle read
  const double* xi;    // [rows][m] or null
  const double* eng;   // [rows] the engine's value of kind out_kind, or null (cf_marg_apply_device: no engine values)
  double* t;           // [rows][m] or null
  double* q;           // [rows] or null
  double* alpha;       // [rows][m] or null
  double* out;         // [rows] or null
  double pmu, log_norm;
  int32_t m, n_slice, out_kind, mode;
};

#define MR_TPB 256
#define MR_ROWS_PER_WG (MR_TPB / MP_TILE)

__global__ void __launch_bounds__(MR_TPB) marg_row_kernel(int64_t rows, cf_marg_row_args a) {
  const int j = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * MR_ROWS_PER_WG + (threadIdx.x >> 4);
  const bool in = row < rows;   // every lane stays to the end: the lane-to-lane reads below never miss a partner
  const bool live = in && j < a.m;
  const int m = a.m;
  double t = 0.0;
  if (live) {
    const double* __restrict__ p = a.part + row * a.n_slice * (int64_t)MP_TILE + j;
    for (int b = 0; b < a.n_slice; ++b) t += p[(int64_t)b * MP_TILE];
    t += a.ct[j];
  }
  double q = 0.0;
  bool bad = false;
  for (int c = 0; c < m; ++c) {
    const double tc = __shfl(t, c, MP_TILE);
    q = marg_q_step(q, tc);
    bad = bad || !marg_finite(tc);
  }
  const double e = (in && a.eng) ? a.eng[row] : 0.0;
  const bool dead = bad || marg_dead(e);
  double v = t;
  if (live && a.xi) v += a.xi[row * m + j];
  double alpha = 0.0;
  for (int c = m - 1; c >= 0; --c) {
    const double ucc = a.U[c * m + c];
    const double ac = __shfl(v, c, MP_TILE) / ucc;
    if (j == c) alpha = ac;
    if (j < c) v = marg_back_step(v, a.U[j * m + c], ac);
  }
  if (live) {
    if (a.t) a.t[row * m + j] = bad ? NAN : t;
    if (a.alpha) a.alpha[row * m + j] = dead ? NAN : alpha;
  }
  if (in && j == 0) {
    if (a.q) a.q[row] = bad ? NAN : q;
    if (a.out) a.out[row] = marg_combine(a.out_kind, a.mode, e, q, a.pmu, a.log_norm, bad);
  }
}

// ------------------------------------------------------------------------------------------------
// Host side.
// ------------------------------------------------------------------------------------------------
struct cf_marg {
  int64_t n = 0, n_pad = 0;  // n_pad: rows of Wt on the device, n rounded up to MP_BK (zero in the padding)
  int32_t m = 0;
  int device = 0;
  double pmu = 0.0, log_norm = 0.0;
  DevBuf Wt, ct, U;
  // the ONE scratch of the slice partials is shared by every call on this object: a call on another stream than the previous one
  // first waits, on the host, for the device (as a handle's workspace: the caller's stream is compared, never passed back to HIP)
  DevBuf part;
  std::mutex mu;
  hipStream_t last_stream = nullptr;
  bool has_last = false;
};

static inline int marg_slices(int64_t n) { return (int)((n + MP_SLICE - 1) / MP_SLICE); }

extern "C" int cf_selftest_marg_host(const double* part, int32_t n_slice, const double* ct, const double* U, int32_t m,
                                     const double* xi, double pmu, double log_norm, double e, int32_t out_kind, int32_t mode,
                                     double* t, double* q, double* alpha, double* value) {
  const std::string F = "cf_selftest_marg_host: ";
  if (!part || !ct || !U) return cf_set_error(CF_ERR_INVALID, F + "null argument");
  if (n_slice < 1 || n_slice > marg_slices(MARG_MAX_N)) return cf_set_error(CF_ERR_INVALID, F + "n_slice out of range");
  if (m < 1 || m > CF_MARG_MAX_M) return cf_set_error(CF_ERR_INVALID, F + "m must be in 1..16");
  if (out_kind < CF_OUT_CHI2 || out_kind > CF_OUT_LOGP) return cf_set_error(CF_ERR_INVALID, F + "bad out_kind");
  if (mode != CF_MARG_PROFILE && mode != CF_MARG_MARGINAL) return cf_set_error(CF_ERR_INVALID, F + "bad mode");
  double tt[CF_MARG_MAX_M], v[CF_MARG_MAX_M], al[CF_MARG_MAX_M];
  for (int j = 0; j < m; ++j) {
    double s = 0.0;
    for (int b = 0; b < n_slice; ++b) s += part[(int64_t)b * MP_TILE + j];
    tt[j] = s + ct[j];
  }
  double qq = 0.0;
  bool bad = false;
  for (int c = 0; c < m; ++c) {
    qq = marg_q_step(qq, tt[c]);
    bad = bad || !marg_finite(tt[c]);
  }
  const bool dead = bad || marg_dead(e);
  for (int j = 0; j < m; ++j) v[j] = xi ? tt[j] + xi[j] : tt[j];
  for (int c = m - 1; c >= 0; --c) {
    al[c] = v[c] / U[c * m + c];
    for (int j = 0; j < c; ++j) v[j] = marg_back_step(v[j], U[j * m + c], al[c]);
  }
  for (int j = 0; j < m; ++j) {
    if (t) t[j] = bad ? NAN : tt[j];
    if (alpha) alpha[j] = dead ? NAN : al[j];
  }
  if (q) *q = bad ? NAN : qq;
  if (value) *value = marg_combine(out_kind, mode, e, qq, pmu, log_norm, bad);
  return CF_OK;
}

extern "C" int cf_marg_create(const double* Wt, const double* ct, const double* U, int64_t n, int32_t m, double pmu, double log_norm,
                              int32_t device, cf_marg** out) {
  const std::string F = "cf_marg_create: ";
  if (!out) return cf_set_error(CF_ERR_INVALID, F + "null argument");
  *out = nullptr;
  if (!Wt || !ct || !U) return cf_set_error(CF_ERR_INVALID, F + "null argument");
  if (n < 1 || n > MARG_MAX_N) return cf_set_error(CF_ERR_INVALID, F + "n must be in 1..32768");
  if (m < 1 || m > CF_MARG_MAX_M) return cf_set_error(CF_ERR_INVALID, F + "m must be in 1..16");
  if (!std::isfinite(pmu) || !std::isfinite(log_norm)) return cf_set_error(CF_ERR_INVALID, F + "a non-finite pmu or log_norm");
  const int64_t n_pad = (n + MP_BK - 1) / MP_BK * MP_BK;
  std::vector<double> Wp((size_t)n_pad * MP_TILE, 0.0), cp(MP_TILE, 0.0), Up((size_t)m * m, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < m; ++j) {
      const double v = Wt[i * m + j];
      if (!std::isfinite(v)) return cf_set_error(CF_ERR_INVALID, F + "a non-finite entry of Wt");
      Wp[(size_t)i * MP_TILE + j] = v;
    }
  for (int j = 0; j < m; ++j) {
    if (!std::isfinite(ct[j])) return cf_set_error(CF_ERR_INVALID, F + "a non-finite entry of ct");
    cp[j] = ct[j];
    for (int c = j; c < m; ++c) {  // the upper triangle; what lies below the diagonal is never read
      const double v = U[j * m + c];
      if (!std::isfinite(v)) return cf_set_error(CF_ERR_INVALID, F + "a non-finite entry of U");
      Up[(size_t)j * m + c] = v;
    }
    if (!(U[j * m + j] > 0.0)) return cf_set_error(CF_ERR_INVALID, F + "the diagonal of U must be positive");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return cf_set_error(CF_ERR_NO_DEVICE, F + "no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return cf_set_error(CF_ERR_INVALID, F + "device ordinal out of range");
  std::unique_ptr<cf_marg> p(new cf_marg());
  p->n = n;
  p->n_pad = n_pad;
  p->m = m;
  p->device = device;
  p->pmu = pmu;
  p->log_norm = log_norm;
  DeviceScope on_device(device);
  HIP_TRY(on_device.err);
  int rc;
  if ((rc = upload(p->Wt, Wp.data(), (int64_t)Wp.size()))) return rc;
  if ((rc = upload(p->ct, cp.data(), (int64_t)cp.size()))) return rc;
  if ((rc = upload(p->U, Up.data(), (int64_t)Up.size()))) return rc;
  *out = p.release();
  return CF_OK;
}

extern "C" void cf_marg_destroy(cf_marg* p) {
  if (!p) return;
  DeviceScope on_device(p->device);
  delete p;
}

extern "C" int cf_marg_info(const cf_marg* p, int64_t* n, int32_t* m, int32_t* device, double* pmu, double* log_norm) {
  if (!p) return cf_set_error(CF_ERR_INVALID, "cf_marg_info: null cf_marg");
  if (n) *n = p->n;
  if (m) *m = p->m;
  if (device) *device = p->device;
  if (pmu) *pmu = p->pmu;
  if (log_norm) *log_norm = p->log_norm;
  return CF_OK;
}

// The scratch for chunks of `rows` rows, and the order behind the previous call.  p->mu held, p's device current.
static int marg_prepare(cf_marg* p, int64_t rows, hipStream_t st) {
  const size_t need = (size_t)rows * (size_t)marg_slices(p->n) * MP_TILE * 8;
  const bool grow = need > p->part.bytes;
  if (grow || (p->has_last && p->last_stream != st)) HIP_TRY(hipDeviceSynchronize());
  if (grow && p->part.ensure(need)) return CF_ERR_HIP;
  p->last_stream = st;
  p->has_last = true;
  return 0;
}

// One chunk: rows at d_rows (row pitch `pitch`) and the row kernel's arguments already offset to the chunk.
static int marg_chunk(cf_marg* p, const double* d_rows, int64_t pitch, int64_t rows, cf_marg_row_args a, hipStream_t st,
                      const char* fn) {
  const int n_slice = marg_slices(p->n);
  const dim3 grid((unsigned)((rows + MP_WAVES * MP_TILE - 1) / (MP_WAVES * MP_TILE)), (unsigned)n_slice);
  hipLaunchKernelGGL(marg_proj_kernel, grid, dim3(MP_TPB), 0, st, d_rows, pitch, (int)p->n, rows, p->Wt.as<const double>(), n_slice,
                     p->part.as<double>());
  if (int rc = cf_launch_status(fn)) return rc;
  a.part = p->part.as<const double>();
  a.ct = p->ct.as<const double>();
  a.U = p->U.as<const double>();
  a.pmu = p->pmu;
  a.log_norm = p->log_norm;
  a.m = p->m;
  a.n_slice = n_slice;
  hipLaunchKernelGGL(marg_row_kernel, dim3((unsigned)((rows + MR_ROWS_PER_WG - 1) / MR_ROWS_PER_WG)), dim3(MR_TPB), 0, st, rows, a);
  return cf_launch_status(fn);
}

extern "C" int cf_marg_apply_device(cf_marg* p, const double* d_rows, int64_t pitch, int64_t S, const double* d_xi, double* d_t,
                                    double* d_q, double* d_alpha, void* hip_stream) {
  const std::string F = "cf_marg_apply_device: ";
  if (!p) return cf_set_error(CF_ERR_INVALID, F + "null cf_marg");
  if (S < 0 || S > CF_RESID_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, F + "S out of range");
  if (pitch < p->n) return cf_set_error(CF_ERR_INVALID, F + "a pitch below n");
  if (!d_t && !d_q && !d_alpha) return cf_set_error(CF_ERR_INVALID, F + "no output requested");
  if (S == 0) return CF_OK;
  if (!d_rows) return cf_set_error(CF_ERR_INVALID, F + "null rows");
  std::lock_guard<std::mutex> lock(p->mu);
  DeviceScope on_device(p->device);
  HIP_TRY(on_device.err);
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t chunk = std::min<int64_t>(S, CF_MARG_CHUNK);
  const int64_t m = p->m;
  int rc;
  if ((rc = marg_prepare(p, chunk, st))) return rc;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t rows = std::min(chunk, S - s0);
    cf_marg_row_args a{};
    a.xi = d_xi ? d_xi + s0 * m : nullptr;
    a.t = d_t ? d_t + s0 * m : nullptr;
    a.q = d_q ? d_q + s0 : nullptr;
    a.alpha = d_alpha ? d_alpha + s0 * m : nullptr;
    if ((rc = marg_chunk(p, d_rows + s0 * pitch, pitch, rows, a, st, "cf_marg_apply_device"))) return rc;
  }
  return CF_OK;
}

extern "C" int cf_marg_check_args(int64_t n_sn, int32_t is_quasar, int32_t n_devices, int32_t handle_device, int32_t has_marg,
                                  int64_t marg_n, int32_t marg_device, const void* theta, int64_t S, int32_t out_kind, int32_t mode,
                                  const void* out, const void* alpha) {
  const std::string F = "cf_marg: ";
  if (is_quasar) return cf_set_error(CF_ERR_INVALID, F + "a quasar handle has no accessor path to take the residuals from");
  if (n_devices > 1) return cf_set_error(CF_ERR_INVALID, F + "this handle spans several devices; use one handle per device");
  if (n_sn < 1) return cf_set_error(CF_ERR_INVALID, F + "this handle has no SN block");
  if (!has_marg) return cf_set_error(CF_ERR_INVALID, F + "null cf_marg");
  if (marg_n != n_sn) return cf_set_error(CF_ERR_INVALID, F + "cf_marg.n is not the number of SNe of the handle");
  if (marg_device != handle_device) return cf_set_error(CF_ERR_INVALID, F + "the cf_marg lives on another device than the handle");
  if (out_kind != CF_OUT_CHI2 && out_kind != CF_OUT_LOGL && out_kind != CF_OUT_LOGP)
    return cf_set_error(CF_ERR_INVALID, F + "out_kind must be CF_OUT_CHI2, CF_OUT_LOGL or CF_OUT_LOGP");
  if (mode != CF_MARG_PROFILE && mode != CF_MARG_MARGINAL)
    return cf_set_error(CF_ERR_INVALID, F + "mode must be CF_MARG_PROFILE or CF_MARG_MARGINAL");
  if (S < 0 || S > CF_RESID_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, F + "S out of range");
  if (!out && !alpha) return cf_set_error(CF_ERR_INVALID, F + "no output requested");
  if (S > 0 && !theta) return cf_set_error(CF_ERR_INVALID, F + "null theta");
  return CF_OK;
}

static int marg_check(cf_handle* h, cf_marg* p, const void* theta, int64_t S, int32_t out_kind, int32_t mode, const void* out,
                      const void* alpha) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_marg: null handle");
  return cf_marg_check_args(h->d.n_sn, h->qsr ? 1 : 0, 1 + (int32_t)h->peers.size(), h->device, p ? 1 : 0, p ? p->n : 0,
                            p ? p->device : 0, theta, S, out_kind, mode, out, alpha);
}

extern "C" int cf_marg_set_chunk(cf_handle* h, int64_t rows) { return set_chunk(h, &cf_handle::marg_chunk, rows, "cf_marg_set_chunk"); }

// Arguments checked.  Device pointers throughout.  The residual rows come from the accessor path one chunk at a time exactly as
// mock_run gets them (rows at h->delta, pitch n_ld); the engine's value of the asked kind lands in h->out and the two kernels
// follow on the same stream.
static int marg_run(const HandleScope& hs, cf_marg* p, const double* d_theta, int64_t S, int32_t out_kind, int32_t mode,
                    const double* d_xi, double* d_out, double* d_alpha, hipStream_t st) {
  cf_handle* const h = hs.h;
  int rc;
  const int64_t chunk = std::min<int64_t>(S, h->marg_chunk > 0 ? h->marg_chunk : CF_MARG_CHUNK);
  if ((rc = ensure_workspace(h, chunk))) return rc;
  if ((rc = resid_prepare(hs, chunk))) return rc;
  std::lock_guard<std::mutex> lock(p->mu);
  if ((rc = marg_prepare(p, chunk, st))) return rc;
  const cf_dev_desc& d = h->d;
  const int64_t m = p->m;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t rows = std::min(chunk, S - s0);
    // a mu_corr buffer selects the accessor form of the per-walker kernel (residual rows in row layout), as in resid_run
    if ((rc = launch_path(h, d_theta + s0 * d.ndim, rows, h->out.as<double>(), out_kind, st, nullptr, h->r_mc.as<double>(),
                          h->r_blk.as<double>(), d.n_bao > 0 ? h->r_bt.as<double>() : nullptr)))
      return rc;
    cf_marg_row_args a{};
    a.xi = d_xi ? d_xi + s0 * m : nullptr;
    a.eng = h->out.as<const double>();
    a.out = d_out ? d_out + s0 : nullptr;
    a.alpha = d_alpha ? d_alpha + s0 * m : nullptr;
    a.out_kind = out_kind;
    a.mode = mode;
    if ((rc = marg_chunk(p, h->delta.as<const double>(), (int64_t)d.n_ld, rows, a, st, "cf_marg_eval_device"))) return rc;
  }
  return CF_OK;
}

extern "C" int cf_marg_eval_device(cf_handle* h, cf_marg* p, const double* d_theta, int64_t S, int32_t out_kind, int32_t mode,
                                   const double* d_xi, double* d_out, double* d_alpha, void* hip_stream) {
  int rc = marg_check(h, p, d_theta, S, out_kind, mode, d_out, d_alpha);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  return marg_run(hs, p, d_theta, S, out_kind, mode, d_xi, d_out, d_alpha, (hipStream_t)hip_stream);
}

// Host-buffer twin: rows in pieces through temporary device buffers on the handle's own stream.
#define CF_MARG_HOST_PIECE 4096

extern "C" int cf_marg_eval(cf_handle* h, cf_marg* p, const double* theta, int64_t S, int32_t out_kind, int32_t mode, const double* xi,
                            double* out, double* alpha) {
  int rc = marg_check(h, p, theta, S, out_kind, mode, out, alpha);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  RowStage rows(h->stream, std::min<int64_t>(S, CF_MARG_HOST_PIECE));
  const double* dth = rows.in(theta, (size_t)h->d.ndim * 8);
  const double* dxi = rows.in(xi, (size_t)p->m * 8);
  double* dout = rows.out(out, 8);
  double* dal = rows.out(alpha, (size_t)p->m * 8);
  return rows.run(S, [&](int64_t, int64_t m) { return marg_run(hs, p, dth, m, out_kind, mode, dxi, dout, dal, h->stream); });
}
