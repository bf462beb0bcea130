// cosmofit_infl.hip — which data carry a chi^2: per-datum attribution and leave-one-out residuals of every chain sample
// (include/cosmofit.h: cf_infl_device, cf_prec_apply_device; the kernels, then the host-side precision matrix cf_prec, the
// argument checks and the chunk loop; the driver is cosmology-model-fit_amd/influence.py).
//
// Everything follows from one vector per sample, g = K r with K = C^-1 the precision matrix of the block:
//   contrib_i = r_i g_i            (sum_i contrib_i = chi^2: an exact additive split of the chi^2 over the data)
//   loo_i     = g_i / K_ii         (datum i minus its prediction from all the others; its error is 1 / sqrt(K_ii))
//   z_i       = g_i / sqrt(K_ii)   (the z-score of that leave-one-out residual)
//   chi^2 without datum i = chi^2 - g_i^2 / K_ii
//
// prec_gemm_kernel: G[S, n] = R[S, n] K[n, n] on FP64 matrix cores (v_mfma_f64_16x16x4_f64; operand maps as in
// tri_gemm_chi2_kernel of cosmofit_kernels.hip: lane l holds A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15], result register r
// of the lane is D[(l>>4) + 4 r][l&15]).  A workgroup of four waves owns a 64 x 64 block of G, wave (wr, wc) its 32 x 32
// quarter as 2 x 2 tiles; the K range is walked in tiles of 32 staged through LDS (R rows at pitch 34, K rows at pitch 80
// doubles: the fragment reads of a half wave fall on 32 different 8-byte banks), the next tile's global loads issued before
// the current tile's MFMAs.  Every output has ONE accumulator and the k loop is ascending in steps of 4 over ceil(n / 32) * 32
// columns whatever S is, so an element of G depends on its row of R and on K only -- not on S, the row's position, the chunking or
// the tile the row fell in.  Rows >= S and columns >= n of R are never read (a select, not a product with zero: what lies in the
// padding of the residual rows cannot reach a result); a NaN or inf in a row of R stays in that row of G.
//
// infl_row_kernel: ONE WAVE PER ROW, four rows per 256-thread workgroup, no LDS and no atomics (as resid_sample_kernel).  chi^2
// is summed as lane-strided partials (lane l takes i = l, l + 64, ...) combined by the fixed xor butterfly (32, 16, .., 1).  A
// datum whose K_ii is 0 is one the likelihood ignores (a zeroed row and column of a BAO inverse covariance): z, loo and its
// deletion drop are 0 there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_handle.h"
#include "cf_wave.h"
#include "cosmofit_group.h"
#include "cosmofit_resid.h"

// Where the residuals of a chunk lie, as in cf_resid_src.  SN block (and caller-supplied rows): r = rows[s][i] (row pitch
// `pitch`, columns >= n are never read).  BAO block: r = data[i] - rows[s][i], formed where it is read.
struct cf_infl_src {
  const double* rows;
  const double* data;  // BAO: val; else unused
  int64_t pitch;       // doubles between rows of `rows`
  int32_t n, bao;
};

// what infl_row_kernel reads beside the residuals and writes: g at pitch g_pitch, the row arrays at pitch n (any may be null)
struct cf_infl_rows {
  const double* g;
  int64_t g_pitch;
  const double* kdiag;           // [n] K_ii
  const double* inv_sqrt_kdiag;  // [n] 1 / sqrt(K_ii), 0 where K_ii = 0
  double* contrib;
  double* z;
  double* loo;
  double* sample;                // [rows][CF_INFL_NCOL] or null
};

typedef double d4 __attribute__((ext_vector_type(4)));

#define PG_TPB 256
#define PG_BM 64
#define PG_BN 64
#define PG_BK 32
#define PG_RP (PG_BK + 2)   // LDS pitch of a staged R row
#define PG_KP (PG_BN + 16)  // LDS pitch of a staged K row

__device__ __forceinline__ double infl_r_at(const cf_infl_src& src, int64_t s, int i) {
  const double v = src.rows[s * src.pitch + i];
  return src.bao ? src.data[i] - v : v;
}

__global__ void __launch_bounds__(PG_TPB) prec_gemm_kernel(cf_infl_src src, int64_t S, const double* __restrict__ K, int64_t kp,
                                                           double* __restrict__ G, int64_t g_pitch) {
  __shared__ double Rs[PG_BM * PG_RP];
  __shared__ double Ks[PG_BK * PG_KP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * PG_BM;
  const int col0 = blockIdx.y * PG_BN;
  const int n = src.n;
  // staging: thread t fetches R[row0 + (t>>5) + 8 j][k0 + (t&31)] and K[k0 + (t>>6) + 4 j][col0 + (t&63)], j < 8
  const int rk = tid & 31, rr = tid >> 5;
  const int kc = tid & 63, kr = tid >> 6;
  double rreg[8], kreg[8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t row = row0 + rr + 8 * j;
      const int k = k0 + rk;
      rreg[j] = (row < S && k < n) ? infl_r_at(src, row, k) : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + kr + 4 * j, c = col0 + kc;
      kreg[j] = (k < kp && c < kp) ? K[(int64_t)k * kp + c] : 0.0;
    }
  };
  const int wr = wave >> 1, wc = wave & 1;
  const double* a_lds = Rs + (32 * wr + (lane & 15)) * PG_RP + (lane >> 4);
  const double* b_lds = Ks + (lane >> 4) * PG_KP + 32 * wc + (lane & 15);
  d4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) acc[t][u] = d4{0.0, 0.0, 0.0, 0.0};
  const int n_tiles = (n + PG_BK - 1) / PG_BK;
  fetch(0);
  for (int tile = 0; tile < n_tiles; ++tile) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Rs[(rr + 8 * j) * PG_RP + rk] = rreg[j];
      Ks[(kr + 4 * j) * PG_KP + kc] = kreg[j];
    }
    __syncthreads();
    if (tile + 1 < n_tiles) fetch((tile + 1) * PG_BK);
#pragma unroll
    for (int kk = 0; kk < PG_BK; kk += 4) {
      const double a0 = a_lds[kk], a1 = a_lds[16 * PG_RP + kk];
      const double b0 = b_lds[kk * PG_KP], b1 = b_lds[kk * PG_KP + 16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = col0 + 32 * wc + 16 * u + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 32 * wr + 16 * t + (lane >> 4) + 4 * r;
        if (row < S && col < n) G[row * g_pitch + col] = acc[t][u][r];
      }
    }
}

#define IR_TPB 256
#define IR_ROWS_PER_WG (IR_TPB / 64)

__global__ void __launch_bounds__(IR_TPB) infl_row_kernel(cf_infl_src src, int64_t rows, cf_infl_rows a) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * IR_ROWS_PER_WG + (threadIdx.x >> 6);
  if (s >= rows) return;  // whole waves leave: no cross-lane step below has a missing partner
  const int n = src.n;
  const double* __restrict__ g = a.g + s * a.g_pitch;
  const int64_t o = s * (int64_t)n;
  double chi = 0.0, zmax = -1.0, dmax = -1.0;
  int zidx = 0x7fffffff, didx = 0x7fffffff;
  for (int i = lane; i < n; i += 64) {
    const double r = infl_r_at(src, s, i), gi = g[i], kd = a.kdiag[i];
    const bool live = kd > 0.0;
    const double c = r * gi;
    const double z = live ? gi * a.inv_sqrt_kdiag[i] : 0.0;
    const double e = live ? gi / kd : 0.0;
    const double drop = live ? (gi * gi) / kd : 0.0;
    chi += c;
    if (a.contrib) a.contrib[o + i] = c;
    if (a.z) a.z[o + i] = z;
    if (a.loo) a.loo[o + i] = e;
    if (argmax_before(fabs(z), i, zmax, zidx)) { zmax = fabs(z); zidx = i; }
    if (argmax_before(drop, i, dmax, didx)) { dmax = drop; didx = i; }
  }
  if (!a.sample) return;
  chi = wave_sum(chi);
  wave_argmax(zmax, zidx);
  wave_argmax(dmax, didx);
  if (lane == 0) {
    double* out = a.sample + (int64_t)CF_INFL_NCOL * s;
    out[CF_IS_CHI2] = chi;
    out[CF_IS_MAX_Z] = zmax;
    out[CF_IS_MAX_Z_IDX] = (double)zidx;
    out[CF_IS_MAX_DROP] = dmax;
    out[CF_IS_MAX_DROP_IDX] = (double)didx;
  }
}

// G[rows, n] = R[rows, n] K[n, n]; K row-major at pitch kp = n rounded up to 16, zero in the padding.
static int cf_prec_gemm_launch(const cf_infl_src& src, int64_t rows, const double* K, int64_t kp, double* g, int64_t g_pitch,
                        hipStream_t st) {
  const dim3 grid((unsigned)((rows + PG_BM - 1) / PG_BM), (unsigned)((src.n + PG_BN - 1) / PG_BN));
  hipLaunchKernelGGL(prec_gemm_kernel, grid, dim3(PG_TPB), 0, st, src, rows, K, kp, g, g_pitch);
  return cf_launch_status("cf_prec_apply_device");
}

static int cf_infl_row_launch(const cf_infl_src& src, int64_t rows, const cf_infl_rows& a, hipStream_t st) {
  hipLaunchKernelGGL(infl_row_kernel, dim3((unsigned)((rows + IR_ROWS_PER_WG - 1) / IR_ROWS_PER_WG)), dim3(IR_TPB), 0, st, src, rows,
                     a);
  return cf_launch_status("cf_infl_device");
}

// ------------------------------------------------------------------------------------------------
// Host side of the attribution and leave-one-out residuals.  Everything follows from
// g = K r with K = C^-1: the precision matrix is formed once on the host (cf_prec), the residual rows come from the accessor
// path one chunk at a time exactly as resid_run gets them, prec_gemm_kernel forms g behind them on the same stream,
// infl_row_kernel the per-row quantities, and the fit report's resid_datum_kernel continues the per-datum accumulators over the
// z and contrib rows (a unit sigma, so its thresholds are in sigmas).
// ------------------------------------------------------------------------------------------------
#define CF_PREC_MAX_N 32768

struct cf_prec {
  int64_t n = 0, kp = 0;  // kp: row pitch of K on the device, n rounded up to 16 (zero in the padding)
  int device = 0;
  DevBuf K, kdiag, inv_sqrt_kdiag, ones;
  std::vector<double> kdiag_host;
};

static unsigned prec_threads(int64_t n) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt == 0 ? 1 : (nt > 16 ? 16 : nt);
  return n < 256 ? 1 : nt;
}

template <class F>
static void prec_parallel(unsigned nt, F work) {
  if (nt == 1) {
    work(0u);
    return;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(work, t);
  for (auto& x : th) x.join();
}

// s + c carries the running sum: c collects what each addition rounds away (Knuth's TwoSum, branch-free)
static inline void prec_add(long double& s, long double& c, long double p) {
  const long double t = s + p, z = t - s;
  c += (s - (t - z)) + (p - z);
  s = t;
}

// Column j of Linv in extended precision, col[j .. n-1] indexed by the row: the forward substitution of cf_invert_lower
// (cf_pack.h) with compensated sums.  The plain recurrence loses sqrt(n) cond(L) 2^-64 of an entry, which on the Pantheon+-like
// covariances (cond(L) of a few hundred) is several units of the double the precision matrix is rounded to.
static void prec_inverse_column(const double* L, int64_t n, int64_t ld, int64_t j, long double* col) {
  col[j] = 1.0L / (long double)L[j * ld + j];
  for (int64_t i = j + 1; i < n; ++i) {
    const double* row = L + i * ld;
    long double s0 = 0.0L, c0 = 0.0L, s1 = 0.0L, c1 = 0.0L;
    int64_t k = j;
    for (; k + 1 < i; k += 2) {
      prec_add(s0, c0, (long double)row[k] * col[k]);
      prec_add(s1, c1, (long double)row[k + 1] * col[k + 1]);
    }
    if (k < i) prec_add(s0, c0, (long double)row[k] * col[k]);
    prec_add(s0, c0, s1);
    col[i] = -(s0 + (c0 + c1)) / (long double)row[i];
  }
}

// K = Linv^T Linv [n x n] of the lower-triangular factor L, every product and sum in `long double`: the columns of Linv stay in
// extended precision (column j packed as its n - j entries from the diagonal down), K_ij = sum_{k >= max(i, j)} Linv_ki Linv_kj
// in four accumulation chains, and the stored double is the one rounding of that sum.
static void prec_from_factor(const double* L, int64_t n, int64_t ld, std::vector<double>& K) {
  std::vector<size_t> off((size_t)n + 1, 0);
  for (int64_t j = 0; j < n; ++j) off[j + 1] = off[j] + (size_t)(n - j);
  std::vector<long double> X(off[n]);
  const unsigned nt = prec_threads(n);
  // interleaved columns / rows: neighbours cost the same
  prec_parallel(nt, [&](unsigned t) {
    for (int64_t j = t; j < n; j += nt) prec_inverse_column(L, n, ld, j, X.data() + off[j] - j);
  });
  K.assign((size_t)n * n, 0.0);
  prec_parallel(nt, [&](unsigned t) {
    for (int64_t i = t; i < n; i += nt) {
      const long double* xi = X.data() + off[i] - i;  // indexed by the row k >= i
      for (int64_t j = 0; j <= i; ++j) {
        const long double* xj = X.data() + off[j] - j;
        long double a0 = 0.0L, a1 = 0.0L, a2 = 0.0L, a3 = 0.0L;
        int64_t k = i;
        for (; k + 3 < n; k += 4) {
          a0 += xi[k] * xj[k];
          a1 += xi[k + 1] * xj[k + 1];
          a2 += xi[k + 2] * xj[k + 2];
          a3 += xi[k + 3] * xj[k + 3];
        }
        for (; k < n; ++k) a0 += xi[k] * xj[k];
        const double v = (double)((a0 + a1) + (a2 + a3));
        K[(size_t)i * n + j] = v;
        K[(size_t)j * n + i] = v;
      }
    }
  });
}

static int prec_check_shape(const char* fn, const void* a, int64_t n, int64_t ld) {
  const std::string F = std::string(fn) + ": ";
  if (!a) return cf_set_error(CF_ERR_INVALID, F + "null matrix");
  if (n < 1 || n > CF_PREC_MAX_N) return cf_set_error(CF_ERR_INVALID, F + "n must be in 1..32768");
  if (ld < n) return cf_set_error(CF_ERR_INVALID, F + "ld < n");
  return CF_OK;
}

static int prec_check_factor(const char* fn, const double* L, int64_t n, int64_t ld) {
  int rc = prec_check_shape(fn, L, n, ld);
  if (rc) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (!(L[i * ld + i] > 0.0) || !std::isfinite(L[i * ld + i])) return cf_set_error(CF_ERR_NOT_POSDEF, std::string(fn) + ": bad pivot");
  return CF_OK;
}

extern "C" int cf_selftest_prec_host(const double* L, int64_t n, int64_t ld, double* K_out, double* kdiag_out) {
  int rc = prec_check_factor("cf_selftest_prec_host", L, n, ld);
  if (rc) return rc;
  std::vector<double> K;
  prec_from_factor(L, n, ld, K);
  if (K_out) memcpy(K_out, K.data(), K.size() * 8);
  if (kdiag_out)
    for (int64_t i = 0; i < n; ++i) kdiag_out[i] = K[(size_t)i * n + i];
  return CF_OK;
}

// K [n x n] to the device: zero-padded to pitch kp, its diagonal, 1 / sqrt(diagonal) (0 for a datum the likelihood ignores) and
// the unit sigma the accumulators of the z and contrib rows divide by.
static int prec_upload(const char* fn, const std::vector<double>& K, int64_t n, int32_t device, cf_prec** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return cf_set_error(CF_ERR_NO_DEVICE, std::string(fn) + ": no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return cf_set_error(CF_ERR_INVALID, std::string(fn) + ": device ordinal out of range");
  std::unique_ptr<cf_prec> p(new cf_prec());
  p->n = n;
  p->kp = (n + 15) / 16 * 16;
  p->device = device;
  std::vector<double> Kp((size_t)p->kp * p->kp, 0.0), isk((size_t)n), ones((size_t)n, 1.0);
  p->kdiag_host.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    memcpy(&Kp[(size_t)i * p->kp], &K[(size_t)i * n], (size_t)n * 8);
    const double kd = K[(size_t)i * n + i];
    p->kdiag_host[i] = kd;
    isk[i] = kd > 0.0 ? (double)(1.0L / sqrtl((long double)kd)) : 0.0;
  }
  DeviceScope on_device(device);
  HIP_TRY(on_device.err);
  int rc;
  if ((rc = upload(p->K, Kp.data(), (int64_t)Kp.size()))) return rc;
  if ((rc = upload(p->kdiag, p->kdiag_host.data(), n))) return rc;
  if ((rc = upload(p->inv_sqrt_kdiag, isk.data(), n))) return rc;
  if ((rc = upload(p->ones, ones.data(), n))) return rc;
  *out = p.release();
  return CF_OK;
}

extern "C" int cf_prec_create(const double* L, int64_t n, int64_t ld, int32_t device, cf_prec** out) {
  if (!out) return cf_set_error(CF_ERR_INVALID, "cf_prec_create: null argument");
  *out = nullptr;
  int rc = prec_check_factor("cf_prec_create", L, n, ld);
  if (rc) return rc;
  std::vector<double> K;
  prec_from_factor(L, n, ld, K);
  return prec_upload("cf_prec_create", K, n, device, out);
}

extern "C" int cf_prec_create_inv(const double* inv_cov, int64_t n, int64_t ld, int32_t device, cf_prec** out) {
  if (!out) return cf_set_error(CF_ERR_INVALID, "cf_prec_create_inv: null argument");
  *out = nullptr;
  int rc = prec_check_shape("cf_prec_create_inv", inv_cov, n, ld);
  if (rc) return rc;
  std::vector<double> K((size_t)n * n);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = 0; j < n; ++j) {
      const double v = 0.5 * (inv_cov[i * ld + j] + inv_cov[j * ld + i]);
      if (!std::isfinite(v) || (i == j && v < 0.0))
        return cf_set_error(CF_ERR_NOT_POSDEF, "cf_prec_create_inv: a non-finite entry or a negative diagonal entry");
      K[(size_t)i * n + j] = v;
    }
  return prec_upload("cf_prec_create_inv", K, n, device, out);
}

extern "C" void cf_prec_destroy(cf_prec* p) {
  if (!p) return;
  DeviceScope on_device(p->device);
  delete p;
}

extern "C" int cf_prec_diag(cf_prec* p, double* out_n) {
  if (!p || !out_n) return cf_set_error(CF_ERR_INVALID, "cf_prec_diag: null argument");
  memcpy(out_n, p->kdiag_host.data(), p->kdiag_host.size() * 8);
  return CF_OK;
}

// what cosmofit_group.hip reads of a cf_prec (cosmofit_group.h)
int cf_prec_look(const cf_prec* p, cf_prec_view* out) {
  if (!p || !out) return cf_set_error(CF_ERR_INVALID, "cf_group: null cf_prec");
  *out = cf_prec_view{p->n, p->kp, p->device, p->K.as<const double>(), p->kdiag_host.data()};
  return CF_OK;
}

extern "C" int cf_prec_apply_device(cf_prec* p, const double* d_rows, int64_t pitch, int64_t S, double* d_g, int64_t g_pitch,
                                    void* hip_stream) {
  const std::string F = "cf_prec_apply_device: ";
  if (!p) return cf_set_error(CF_ERR_INVALID, F + "null cf_prec");
  if (S < 0 || S > CF_RESID_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, F + "S out of range");
  if (pitch < p->n || g_pitch < p->n) return cf_set_error(CF_ERR_INVALID, F + "a pitch below n");
  if (S == 0) return CF_OK;
  if (!d_rows || !d_g) return cf_set_error(CF_ERR_INVALID, F + "null rows or g");
  DeviceScope on_device(p->device);
  HIP_TRY(on_device.err);
  const cf_infl_src src{d_rows, nullptr, pitch, (int32_t)p->n, 0};
  return cf_prec_gemm_launch(src, S, p->K.as<const double>(), p->kp, d_g, g_pitch, (hipStream_t)hip_stream);
}

static int infl_check_acc(const std::string& F, const char* name, const cf_resid_acc* acc, int64_t n, int32_t n_thr) {
  const std::string A = F + name;
  if (acc->struct_size != (int32_t)sizeof(cf_resid_acc)) return cf_set_error(CF_ERR_INVALID, A + ".struct_size mismatch");
  if (acc->n != n) return cf_set_error(CF_ERR_INVALID, A + ".n is not the number of data of the block");
  if (acc->n_thr != n_thr) return cf_set_error(CF_ERR_INVALID, A + (n_thr ? ".n_thr differs from n_thr" : ".n_thr must be 0"));
  if (acc_lacks_an_array(acc, n_thr)) return cf_set_error(CF_ERR_INVALID, A + " has a null array");
  return CF_OK;
}

extern "C" int cf_infl_check_args(int64_t n_sn, int32_t n_bao, int32_t is_quasar, int32_t n_devices, int32_t handle_device,
                                  int32_t has_prec, int64_t prec_n, int32_t prec_device, const void* theta, int64_t S, int32_t block,
                                  const double* thresholds, int32_t n_thr, const cf_infl_out* out, const cf_resid_acc* acc_z,
                                  const cf_resid_acc* acc_contrib) {
  const std::string F = "cf_infl: ";
  if (is_quasar) return cf_set_error(CF_ERR_INVALID, F + "a quasar handle has no accessor path to take the residuals from");
  if (n_devices > 1) return cf_set_error(CF_ERR_INVALID, F + "this handle spans several devices; use one handle per device");
  int rc;
  if ((rc = check_block(F, n_sn, n_bao, block))) return rc;
  const int64_t n = block == CF_RB_SN ? n_sn : n_bao;
  if (!has_prec) return cf_set_error(CF_ERR_INVALID, F + "null cf_prec");
  if (prec_n != n) return cf_set_error(CF_ERR_INVALID, F + "cf_prec.n is not the number of data of the block");
  if (prec_device != handle_device) return cf_set_error(CF_ERR_INVALID, F + "the cf_prec lives on another device than the handle");
  if ((rc = check_rows_thresholds(F, S, thresholds, n_thr))) return rc;
  if (out && out->struct_size != (int32_t)sizeof(cf_infl_out)) return cf_set_error(CF_ERR_INVALID, F + "cf_infl_out.struct_size mismatch");
  const bool any_out = out && (out->g || out->contrib || out->z || out->loo || out->sample);
  if (!any_out && !acc_z && !acc_contrib) return cf_set_error(CF_ERR_INVALID, F + "no output requested");
  if (acc_z && (rc = infl_check_acc(F, "acc_z", acc_z, n, n_thr))) return rc;
  if (acc_contrib && (rc = infl_check_acc(F, "acc_contrib", acc_contrib, n, 0))) return rc;
  if (S > 0 && !theta) return cf_set_error(CF_ERR_INVALID, F + "null theta");
  return CF_OK;
}

static int infl_check(cf_handle* h, cf_prec* prec, const void* theta, int64_t S, int32_t block, const double* thresholds,
                      int32_t n_thr, const cf_infl_out* out, const cf_resid_acc* acc_z, const cf_resid_acc* acc_contrib) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_infl: null handle");
  return cf_infl_check_args(h->d.n_sn, h->d.n_bao, h->qsr ? 1 : 0, 1 + (int32_t)h->peers.size(), h->device, prec ? 1 : 0,
                            prec ? prec->n : 0, prec ? prec->device : 0, theta, S, block, thresholds, n_thr, out, acc_z, acc_contrib);
}

extern "C" int cf_infl_set_chunk(cf_handle* h, int64_t rows) { return set_chunk(h, &cf_handle::infl_chunk, rows, "cf_infl_set_chunk"); }

// The chunk buffers of g and of the contrib / z rows.  Growing frees buffers an earlier call on a caller's stream may still use:
// synchronise first, as resid_prepare does.
static int infl_prepare(const HandleScope& hs, int64_t rows, int64_t n, bool need_g, bool need_contrib, bool need_z) {
  cf_handle* const h = hs.h;
  const size_t bytes = (size_t)rows * (size_t)n * 8;
  DevBuf* const buf[3] = {&h->i_g, &h->i_contrib, &h->i_z};
  const bool need[3] = {need_g, need_contrib, need_z};
  bool grow = false;
  for (int k = 0; k < 3; ++k) grow = grow || (need[k] && bytes > buf[k]->bytes);
  if (!grow) return 0;
  HIP_TRY(hipDeviceSynchronize());
  for (int k = 0; k < 3; ++k)
    if (need[k] && buf[k]->ensure(bytes)) return CF_ERR_HIP;
  return 0;
}

// Arguments checked.  Device pointers throughout.
static int infl_run(const HandleScope& hs, const cf_prec* prec, const double* d_theta, int64_t S, const double* d_w, int32_t block,
                    const double* thresholds, int32_t n_thr, const cf_infl_out& out, const cf_resid_acc* acc_z,
                    const cf_resid_acc* acc_contrib, hipStream_t st) {
  cf_handle* const h = hs.h;
  int rc;
  const int64_t chunk = std::min<int64_t>(S, h->infl_chunk > 0 ? h->infl_chunk : CF_INFL_CHUNK);
  if ((rc = ensure_workspace(h, chunk))) return rc;
  if ((rc = resid_prepare(hs, chunk))) return rc;
  const int64_t n = prec->n;
  if ((rc = infl_prepare(hs, chunk, n, !out.g, acc_contrib && !out.contrib, acc_z && !out.z))) return rc;
  const cf_dev_desc& d = h->d;
  const cf_infl_src src = block == CF_RB_SN
                              ? cf_infl_src{h->delta.as<const double>(), nullptr, (int64_t)d.n_ld, (int32_t)d.n_sn, 0}
                              : cf_infl_src{h->r_bt.as<const double>(), d.bao_val, (int64_t)d.n_bao, (int32_t)d.n_bao, 1};
  const cf_resid_blocks no_blocks{nullptr, nullptr, nullptr, nullptr};
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t m = std::min(chunk, S - s0);
    // a mu_corr buffer selects the accessor form of the per-walker kernel (residual rows in row layout), as in resid_run
    if ((rc = launch_path(h, d_theta + s0 * d.ndim, m, h->out.as<double>(), CF_OUT_CHI2, st, nullptr,
                          d.n_sn > 0 ? h->r_mc.as<double>() : nullptr, nullptr, d.n_bao > 0 ? h->r_bt.as<double>() : nullptr)))
      return rc;
    double* g = out.g ? out.g + s0 * n : h->i_g.as<double>();
    if ((rc = cf_prec_gemm_launch(src, m, prec->K.as<const double>(), prec->kp, g, n, st))) return rc;
    cf_infl_rows a{};
    a.g = g;
    a.g_pitch = n;
    a.kdiag = prec->kdiag.as<const double>();
    a.inv_sqrt_kdiag = prec->inv_sqrt_kdiag.as<const double>();
    a.contrib = out.contrib ? out.contrib + s0 * n : (acc_contrib ? h->i_contrib.as<double>() : nullptr);
    a.z = out.z ? out.z + s0 * n : (acc_z ? h->i_z.as<double>() : nullptr);
    a.loo = out.loo ? out.loo + s0 * n : nullptr;
    a.sample = out.sample ? out.sample + (int64_t)CF_INFL_NCOL * s0 : nullptr;
    if (a.contrib || a.z || a.loo || a.sample)
      if ((rc = cf_infl_row_launch(src, m, a, st))) return rc;
    cf_resid_src rows{};
    rows.sigma = prec->ones.as<const double>();
    rows.pitch = n;
    rows.n = (int32_t)n;
    if (acc_z) {
      rows.rows = a.z;
      if ((rc = cf_resid_launch(rows, m, nullptr, no_blocks, d_w ? d_w + s0 : nullptr, thresholds, n_thr, acc_z, st))) return rc;
    }
    if (acc_contrib) {
      rows.rows = a.contrib;
      if ((rc = cf_resid_launch(rows, m, nullptr, no_blocks, d_w ? d_w + s0 : nullptr, nullptr, 0, acc_contrib, st))) return rc;
    }
  }
  return CF_OK;
}

extern "C" int cf_infl_device(cf_handle* h, cf_prec* prec, const double* d_theta, int64_t S, const double* d_w, int32_t block,
                              const double* thresholds, int32_t n_thr, cf_infl_out* out, cf_resid_acc* acc_z,
                              cf_resid_acc* acc_contrib, void* hip_stream) {
  int rc = infl_check(h, prec, d_theta, S, block, thresholds, n_thr, out, acc_z, acc_contrib);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  return infl_run(hs, prec, d_theta, S, d_w, block, thresholds, n_thr, out ? *out : cf_infl_out{}, acc_z, acc_contrib,
                  (hipStream_t)hip_stream);
}

// Host-buffer twin: rows in pieces through temporary device buffers on the handle's own stream (a piece is a chunk: the row
// arrays are [piece][n]).
#define CF_INFL_HOST_PIECE 4096

extern "C" int cf_infl(cf_handle* h, cf_prec* prec, const double* theta, int64_t S, const double* w, int32_t block,
                       const double* thresholds, int32_t n_thr, cf_infl_out* out, cf_resid_acc* acc_z, cf_resid_acc* acc_contrib) {
  int rc = infl_check(h, prec, theta, S, block, thresholds, n_thr, out, acc_z, acc_contrib);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  const size_t row = (size_t)prec->n * 8;
  const cf_infl_out ho = out ? *out : cf_infl_out{};
  RowStage rows(h->stream, std::min<int64_t>(S, CF_INFL_HOST_PIECE));
  const double* dth = rows.in(theta, (size_t)h->d.ndim * 8);
  const double* dw = rows.in(w, 8);
  cf_infl_out dout{};
  dout.struct_size = (int32_t)sizeof(cf_infl_out);
  dout.g = rows.out(ho.g, row); dout.contrib = rows.out(ho.contrib, row); dout.z = rows.out(ho.z, row); dout.loo = rows.out(ho.loo, row);
  dout.sample = rows.out(ho.sample, (size_t)CF_INFL_NCOL * 8);
  HostAccTwin az, ac;
  if ((rc = az.up(acc_z, h->stream)) || (rc = ac.up(acc_contrib, h->stream))) return rc;
  if ((rc = rows.run(S, [&](int64_t, int64_t m) {
         return infl_run(hs, prec, dth, m, dw, block, thresholds, n_thr, dout, az.ptr(), ac.ptr(), h->stream);
       })))
    return rc;
  if ((rc = az.down()) || (rc = ac.down())) return rc;
  return CF_OK;
}
