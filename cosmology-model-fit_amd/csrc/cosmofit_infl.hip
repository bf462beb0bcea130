// cosmofit_infl.hip — which data carry a chi^2: per-datum attribution and leave-one-out residuals of every chain sample
// (include/cosmofit.h: cf_infl_device, cf_prec_apply_device; the launcher, the host-side precision matrix and the argument checks
// are in cosmofit_api.hip, the driver is cosmology-model-fit_amd/influence.py).
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

#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"
#include "cosmofit_infl.h"

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

__device__ __forceinline__ double infl_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

// np.argmax's order on (value, index): a NaN beats every number, among equals the lower index wins
__device__ __forceinline__ bool infl_before(double a, int ia, double b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return an;
  if (an || a == b) return ia < ib;
  return a > b;
}

__device__ __forceinline__ void infl_wave_argmax(double& v, int& idx) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double vo = __shfl_xor(v, m);
    const int io = __shfl_xor(idx, m);
    if (infl_before(vo, io, v, idx)) { v = vo; idx = io; }
  }
}

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
    if (infl_before(fabs(z), i, zmax, zidx)) { zmax = fabs(z); zidx = i; }
    if (infl_before(drop, i, dmax, didx)) { dmax = drop; didx = i; }
  }
  if (!a.sample) return;
  chi = infl_wave_sum(chi);
  infl_wave_argmax(zmax, zidx);
  infl_wave_argmax(dmax, didx);
  if (lane == 0) {
    double* out = a.sample + (int64_t)CF_INFL_NCOL * s;
    out[CF_IS_CHI2] = chi;
    out[CF_IS_MAX_Z] = zmax;
    out[CF_IS_MAX_Z_IDX] = (double)zidx;
    out[CF_IS_MAX_DROP] = dmax;
    out[CF_IS_MAX_DROP_IDX] = (double)didx;
  }
}

int cf_prec_gemm_launch(const cf_infl_src& src, int64_t rows, const double* K, int64_t kp, double* g, int64_t g_pitch,
                        hipStream_t st) {
  const dim3 grid((unsigned)((rows + PG_BM - 1) / PG_BM), (unsigned)((src.n + PG_BN - 1) / PG_BN));
  hipLaunchKernelGGL(prec_gemm_kernel, grid, dim3(PG_TPB), 0, st, src, rows, K, kp, g, g_pitch);
  return cf_launch_status("cf_prec_apply_device");
}

int cf_infl_row_launch(const cf_infl_src& src, int64_t rows, const cf_infl_rows& a, hipStream_t st) {
  hipLaunchKernelGGL(infl_row_kernel, dim3((unsigned)((rows + IR_ROWS_PER_WG - 1) / IR_ROWS_PER_WG)), dim3(IR_TPB), 0, st, src, rows,
                     a);
  return cf_launch_status("cf_infl_device");
}
