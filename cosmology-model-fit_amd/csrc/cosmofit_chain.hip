// cosmofit_chain.hip — statistics of a recorded chain: emcee's integrated autocorrelation time from direct lag sums.
//
// emcee's integrated_time takes the normalised autocorrelation of every (walker, dim) series by FFT, averages it over the
// walkers and reads it at the first lag where lag >= c tau (the window).  The window needs only a prefix of the lags (a
// few times tau, against thousands of steps), so the lags are summed directly here and the host grows the lag range until
// the window is found (chain_stats.py).  A chain [n_t, n_w, ndim] lies in memory as n_t rows of n_s = n_w ndim series:
// lanes take consecutive series (coalesced row loads), the waves of a workgroup take consecutive time segments of the same
// 64 series, and the per-segment partial sums meet in LDS in ascending segment order.  No float atomics anywhere: the same
// chain gives the same bits on every run and for any split of the work between processes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"

#define CF_CHAIN_SEGS 8  // time segments (one wave each) per workgroup of 64 series
#define CF_CHAIN_R 16    // lags held in registers per pass over a segment

// length of one time segment: a multiple of CF_CHAIN_R, so that only the last non-empty segment ends inside a chunk
__device__ __forceinline__ int64_t chain_seg_len(int64_t n_t) {
  return ((n_t + CF_CHAIN_SEGS - 1) / CF_CHAIN_SEGS + CF_CHAIN_R - 1) / CF_CHAIN_R * CF_CHAIN_R;
}

// mean[s] = (sum over the segments, ascending, of the segment's sequential sum) / n_t
extern "C" __global__ void __launch_bounds__(64 * CF_CHAIN_SEGS)
chain_mean_kernel(const double* __restrict__ x, int64_t n_t, int64_t n_s, double* __restrict__ mean) {
  __shared__ double part[CF_CHAIN_SEGS][64];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int64_t s = blockIdx.x * 64ll + lane;
  const int64_t len = chain_seg_len(n_t), t0 = seg * len, t1 = t0 + len < n_t ? t0 + len : n_t;
  double acc = 0.0;
  if (s < n_s)
    for (int64_t t = t0; t < t1; ++t) acc += x[t * n_s + s];
  part[seg][lane] = acc;
  __syncthreads();
  if (seg == 0 && s < n_s) {
    double tot = part[0][lane];
#pragma unroll
    for (int g = 1; g < CF_CHAIN_SEGS; ++g) tot += part[g][lane];
    mean[s] = tot / (double)n_t;
  }
}

// out[j][s] = sum_{t < n_t - tau} (x_t - m)(x_{t + tau} - m), tau = lag0 + j, j < nlag.
// Per sub-block of CF_CHAIN_R lags L .. L + R - 1 a thread walks its segment in chunks of R steps: a[i] = d[t0 + i] and the
// sliding window w[0 .. 2R - 1] = d[t0 + L .. t0 + L + 2R - 1] are registers (every index is a compile-time constant after
// unrolling), acc[k] += a[i] w[i + k] in ascending t.  A value past the end of the chain reads as 0.
extern "C" __global__ void __launch_bounds__(64 * CF_CHAIN_SEGS)
chain_lagsum_kernel(const double* __restrict__ x, const double* __restrict__ mean, int64_t n_t, int64_t n_s, int64_t lag0,
                    int nlag, double* __restrict__ out) {
  __shared__ double part[CF_CHAIN_SEGS][CF_CHAIN_R][64];
  const int lane = threadIdx.x & 63, seg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the wave's segment: uniform
  const int64_t s = blockIdx.x * 64ll + lane;
  // a lane past the last series reads the last series (no branch around the loads) and its sums are never written
  const double* __restrict__ col = x + blockIdx.x * 64ll;
  const unsigned off = (unsigned)(s < n_s ? lane : n_s - 1 - blockIdx.x * 64ll);
  const double m = mean[blockIdx.x * 64ll + off];
  const int64_t len = chain_seg_len(n_t), tb = seg * len, te = tb + len < n_t ? tb + len : n_t;
  // row t of the 64 series: a wave-uniform row address plus a 32-bit lane offset
  auto dev = [&](int64_t t) -> double { return t < n_t ? col[t * n_s + off] - m : 0.0; };
  for (int j0 = 0; j0 < nlag; j0 += CF_CHAIN_R) {
    const int64_t L = lag0 + j0;
    double acc[CF_CHAIN_R], w[2 * CF_CHAIN_R];
#pragma unroll
    for (int k = 0; k < CF_CHAIN_R; ++k) {
      acc[k] = 0.0;
      w[k] = dev(tb + L + k);
    }
    for (int64_t t0 = tb; t0 < te; t0 += CF_CHAIN_R) {
      double a[CF_CHAIN_R];
#pragma unroll
      for (int k = 0; k < CF_CHAIN_R; ++k) {
        w[CF_CHAIN_R + k] = dev(t0 + L + CF_CHAIN_R + k);
        a[k] = dev(t0 + k);  // t0 + k >= te only in the last segment, where it is >= n_t too
      }
#pragma unroll
      for (int i = 0; i < CF_CHAIN_R; ++i)
#pragma unroll
        for (int k = 0; k < CF_CHAIN_R; ++k) acc[k] = fma(a[i], w[i + k], acc[k]);
#pragma unroll
      for (int k = 0; k < CF_CHAIN_R; ++k) w[k] = w[CF_CHAIN_R + k];
    }
#pragma unroll
    for (int k = 0; k < CF_CHAIN_R; ++k) part[seg][k][lane] = acc[k];
    __syncthreads();
    for (int o = threadIdx.x; o < CF_CHAIN_R * 64; o += 64 * CF_CHAIN_SEGS) {
      const int k = o >> 6, ln = o & 63;
      const int64_t so = blockIdx.x * 64ll + ln;
      double tot = part[0][k][ln];
#pragma unroll
      for (int g = 1; g < CF_CHAIN_SEGS; ++g) tot += part[g][k][ln];
      if (j0 + k < nlag && so < n_s) out[(int64_t)(j0 + k) * n_s + so] = tot;
    }
    __syncthreads();  // part is rewritten by the next sub-block
  }
}

// f[j][d] = (sum_{w ascending} lagsum[j][w ndim + d] / c0[w ndim + d]) / n_w: emcee's walker average of the normalised
// autocorrelation (a walker that never moved has c0 = 0 and makes the average NaN, as in emcee)
extern "C" __global__ void __launch_bounds__(256)
chain_acf_mean_kernel(const double* __restrict__ lagsum, const double* __restrict__ c0, int64_t n_w, int ndim, int nlag,
                      double* __restrict__ f) {
  const int64_t o = blockIdx.x * 256ll + threadIdx.x;
  if (o >= (int64_t)nlag * ndim) return;
  const int64_t j = o / ndim, d = o - j * ndim, n_s = n_w * ndim;
  const double* row = lagsum + j * n_s + d;
  const double* nrm = c0 + d;
  double acc = 0.0;
  for (int64_t w = 0; w < n_w; ++w) acc += row[w * ndim] / nrm[w * ndim];
  f[o] = acc / (double)n_w;
}

// ------------------------------------------------------------------------------------------------
static int chain_blocks(int64_t n_s) { return (int)((n_s + 63) / 64); }

extern "C" int cf_chain_mean(const double* d_x, int64_t n_t, int64_t n_s, double* d_mean, void* hip_stream) {
  if (!d_x || !d_mean) return cf_set_error(CF_ERR_INVALID, "cf_chain_mean: null argument");
  if (n_t < 1 || n_s < 1 || (n_s + 63) / 64 > INT32_MAX) return cf_set_error(CF_ERR_INVALID, "cf_chain_mean: bad chain shape");
  hipLaunchKernelGGL(chain_mean_kernel, dim3(chain_blocks(n_s)), dim3(64 * CF_CHAIN_SEGS), 0, (hipStream_t)hip_stream, d_x, n_t, n_s,
                     d_mean);
  return cf_launch_status("cf_chain_mean");
}

extern "C" int cf_chain_lagsum(const double* d_x, const double* d_mean, int64_t n_t, int64_t n_s, int64_t lag0, int32_t nlag,
                               double* d_out, void* hip_stream) {
  if (!d_x || !d_mean || !d_out) return cf_set_error(CF_ERR_INVALID, "cf_chain_lagsum: null argument");
  if (n_t < 1 || n_s < 1 || (n_s + 63) / 64 > INT32_MAX) return cf_set_error(CF_ERR_INVALID, "cf_chain_lagsum: bad chain shape");
  if (lag0 < 0 || nlag < 1) return cf_set_error(CF_ERR_INVALID, "cf_chain_lagsum: need lag0 >= 0 and nlag >= 1");
  hipLaunchKernelGGL(chain_lagsum_kernel, dim3(chain_blocks(n_s)), dim3(64 * CF_CHAIN_SEGS), 0, (hipStream_t)hip_stream, d_x, d_mean,
                     n_t, n_s, lag0, (int)nlag, d_out);
  return cf_launch_status("cf_chain_lagsum");
}

extern "C" int cf_chain_acf_mean(const double* d_lagsum, const double* d_c0, int64_t n_w, int32_t ndim, int32_t nlag, double* d_f,
                                 void* hip_stream) {
  if (!d_lagsum || !d_c0 || !d_f) return cf_set_error(CF_ERR_INVALID, "cf_chain_acf_mean: null argument");
  if (n_w < 1 || ndim < 1 || nlag < 1) return cf_set_error(CF_ERR_INVALID, "cf_chain_acf_mean: need n_w, ndim, nlag >= 1");
  const int64_t n = (int64_t)nlag * ndim;
  hipLaunchKernelGGL(chain_acf_mean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, d_lagsum, d_c0,
                     n_w, (int)ndim, (int)nlag, d_f);
  return cf_launch_status("cf_chain_acf_mean");
}
