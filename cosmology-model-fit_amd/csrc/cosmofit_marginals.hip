// cosmofit_marginals.hip — the numbers behind a corner plot: bin indices of a flat chain, then its 1-D and 2-D histograms.
//
// Two passes.  marg_bin_kernel reads the chain [n, ndim] float64 once and writes one byte per value: numpy's bin of the value
// in its column's edges, or 255 for a value that numpy does not count (below, above, NaN, +-inf).  The histogram kernels then
// read bytes only: one workgroup per (pair, row segment) holds the pair's nbins x nbins histogram in LDS, fills it with LDS
// integer atomics and adds its non-zero bins to the result with global 64-bit integer atomics.  Counts are integers and
// weights are fixed-point integers (quantised once per row), so the sums are exact: the same input gives the same bits on
// every run, for every number of segments and for every order of the rows.  No float atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"

#define CF_MARG_THREADS 256
#define CF_MARG_PER_THREAD 4  // consecutive values per thread of the index pass: one 4-byte store

// ---- index pass ---------------------------------------------------------------------------------------------------
// numpy's rule on the edges it made itself (np.linspace): bin i iff edges[i] <= x < edges[i + 1], the last bin also takes
// x == edges[nbins].  The guess (x - lo) * (nbins / (hi - lo)) can be off by one for a value on or next to an edge, so it is
// corrected against the edges themselves (held in LDS): down while x < edges[g], up while x >= edges[g + 1].
__device__ __forceinline__ unsigned marg_bin_of(double x, const double* __restrict__ e, double scale, int nbins) {
  const double lo = e[0], hi = e[nbins];
  if (!(x >= lo && x <= hi)) return 255u;  // NaN fails both comparisons
  // clamped in double before the cast: a range whose width overflows or is subnormal makes the product inf or NaN, which
  // then starts the correction from bin 0 instead of reaching the conversion
  const double t = (x - lo) * scale;
  int g = t >= 0.0 ? (t < (double)nbins ? (int)t : nbins - 1) : 0;
  while (g > 0 && x < e[g]) --g;
  while (g < nbins - 1 && x >= e[g + 1]) ++g;
  return (unsigned)g;
}

extern "C" __global__ void __launch_bounds__(CF_MARG_THREADS)
marg_bin_kernel(const double* __restrict__ x, int64_t total, int ndim, int nbins, const double* __restrict__ edges,
                uint8_t* __restrict__ idx, int aligned4) {
  extern __shared__ double marg_edges[];  // [ndim][nbins + 1], then scale [ndim]
  const int ne = ndim * (nbins + 1);
  double* scale = marg_edges + ne;
  for (int i = threadIdx.x; i < ne; i += CF_MARG_THREADS) marg_edges[i] = edges[i];
  for (int c = threadIdx.x; c < ndim; c += CF_MARG_THREADS)
    scale[c] = (double)nbins / (edges[c * (nbins + 1) + nbins] - edges[c * (nbins + 1)]);
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * CF_MARG_THREADS * CF_MARG_PER_THREAD;
  for (int64_t e0 = ((int64_t)blockIdx.x * CF_MARG_THREADS + threadIdx.x) * CF_MARG_PER_THREAD; e0 < total; e0 += stride) {
    int c = (int)(e0 % ndim);
    if (e0 + CF_MARG_PER_THREAD <= total) {
      double v[CF_MARG_PER_THREAD];
#pragma unroll
      for (int k = 0; k < CF_MARG_PER_THREAD; ++k) v[k] = x[e0 + k];
      unsigned b[CF_MARG_PER_THREAD];
#pragma unroll
      for (int k = 0; k < CF_MARG_PER_THREAD; ++k) {
        b[k] = marg_bin_of(v[k], marg_edges + c * (nbins + 1), scale[c], nbins);
        c = c + 1 == ndim ? 0 : c + 1;
      }
      if (aligned4) {
        *reinterpret_cast<uint32_t*>(idx + e0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < CF_MARG_PER_THREAD; ++k) idx[e0 + k] = (uint8_t)b[k];
      }
    } else {
      for (int64_t e = e0; e < total; ++e) {
        idx[e] = (uint8_t)marg_bin_of(x[e], marg_edges + c * (nbins + 1), scale[c], nbins);
        c = c + 1 == ndim ? 0 : c + 1;
      }
    }
  }
}

// ---- histogram pass -----------------------------------------------------------------------------------------------
// The fixed-point weight of a row: rint(w / w_max * 2^s), at most 2^s; n of them sum to at most 2^62 (s = 62 - ceil(log2 n)).
__device__ __forceinline__ unsigned long long marg_quantise(double w, double w_max, double two_s) {
  return (unsigned long long)__double2ll_rn(w / w_max * two_s);
}

struct marg_pairs {
  uint8_t a[CF_MARG_MAX_PAIRS], b[CF_MARG_MAX_PAIRS];
};

// rows [r0, r1) of segment `seg` out of `nseg`
__device__ __forceinline__ void marg_segment(int64_t n, int seg, int nseg, int64_t* r0, int64_t* r1) {
  const int64_t len = (n + nseg - 1) / nseg;
  const int64_t b = (int64_t)seg * len, e = b + len;
  *r0 = b < n ? b : n;
  *r1 = e < n ? e : n;
}

// 1-D histograms of every column: one LDS histogram [ndim][nbins] per workgroup, threads walk the bytes of the segment
// (consecutive lanes hold consecutive columns, which spreads the LDS addresses of a wave over the columns).
template <typename CNT, bool WEIGHTED>
__global__ void __launch_bounds__(CF_MARG_THREADS)
marg_hist1_kernel(const uint8_t* __restrict__ idx, const double* __restrict__ w, double w_max, double two_s, int64_t n, int ndim,
                  int nbins, unsigned long long* __restrict__ h1) {
  extern __shared__ unsigned long long marg_lds[];
  CNT* h = reinterpret_cast<CNT*>(marg_lds);
  const int nh = ndim * nbins;
  for (int i = threadIdx.x; i < nh; i += CF_MARG_THREADS) h[i] = 0;
  __syncthreads();
  int64_t r0, r1;
  marg_segment(n, blockIdx.x, gridDim.x, &r0, &r1);
  const int64_t e1 = r1 * ndim;
  for (int64_t e = r0 * ndim + threadIdx.x; e < e1; e += CF_MARG_THREADS) {
    const unsigned v = idx[e];
    if (v < (unsigned)nbins) {  // 255 (not counted), and never an index outside the LDS histogram
      const int64_t r = e / ndim;
      const int c = (int)(e - r * ndim);
      if (WEIGHTED) {
        const unsigned long long q = marg_quantise(w[r], w_max, two_s);
        if (q) atomicAdd(&h[c * nbins + v], (CNT)q);
      } else {
        atomicAdd(&h[c * nbins + v], (CNT)1);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nh; i += CF_MARG_THREADS) {
    const CNT v = h[i];
    if (v) atomicAdd(&h1[i], (unsigned long long)v);
  }
}

// 2-D histogram of one pair per blockIdx.y over the row segment blockIdx.x: H[i][j] counts rows with column a in bin i and
// column b in bin j (np.histogram2d's orientation).  The 32-bit counters of the unweighted path cannot wrap: a segment has
// fewer than 2^31 rows.
template <typename CNT, bool WEIGHTED>
__global__ void __launch_bounds__(CF_MARG_THREADS)
marg_hist2_kernel(const uint8_t* __restrict__ idx, const double* __restrict__ w, double w_max, double two_s, int64_t n, int ndim,
                  int nbins, marg_pairs pairs, unsigned long long* __restrict__ h2) {
  extern __shared__ unsigned long long marg_lds[];
  CNT* h = reinterpret_cast<CNT*>(marg_lds);
  const int nh = nbins * nbins;
  for (int i = threadIdx.x; i < nh; i += CF_MARG_THREADS) h[i] = 0;
  __syncthreads();
  const int ca = pairs.a[blockIdx.y], cb = pairs.b[blockIdx.y];
  int64_t r0, r1;
  marg_segment(n, blockIdx.x, gridDim.x, &r0, &r1);
  for (int64_t r = r0 + threadIdx.x; r < r1; r += CF_MARG_THREADS) {
    const uint8_t* row = idx + r * ndim;
    const unsigned i = row[ca], j = row[cb];
    if (i < (unsigned)nbins && j < (unsigned)nbins) {  // 255: not counted; never an index outside the LDS histogram
      if (WEIGHTED) {
        const unsigned long long q = marg_quantise(w[r], w_max, two_s);
        if (q) atomicAdd(&h[i * nbins + j], (CNT)q);
      } else {
        atomicAdd(&h[i * nbins + j], (CNT)1);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = h2 + (int64_t)blockIdx.y * nh;
  for (int i = threadIdx.x; i < nh; i += CF_MARG_THREADS) {
    const CNT v = h[i];
    if (v) atomicAdd(&out[i], (unsigned long long)v);
  }
}

// ------------------------------------------------------------------------------------------------
static int marg_ceil_log2(int64_t n) {
  int k = 0;
  while (((int64_t)1 << k) < n) ++k;
  return k;
}

static bool marg_shape_ok(int64_t n, int32_t ndim, int32_t nbins) {
  return n >= 1 && n <= (int64_t)INT32_MAX && ndim >= 1 && ndim <= CF_MARG_MAX_NDIM && nbins >= 1 && nbins <= CF_MARG_MAX_BINS;
}

template <typename K>
static bool marg_allow_lds(K kernel, size_t bytes) {
  return bytes <= 65536 || hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)bytes) == hipSuccess;
}

extern "C" int cf_marg_bin(const double* d_x, int64_t n, int32_t ndim, const double* d_edges, int32_t nbins, uint8_t* d_idx,
                           void* hip_stream) {
  if (!d_x || !d_edges || !d_idx) return cf_set_error(CF_ERR_INVALID, "cf_marg_bin: null argument");
  if (!marg_shape_ok(n, ndim, nbins))
    return cf_set_error(CF_ERR_INVALID, "cf_marg_bin: need 1 <= n <= 2^31 - 1, 1 <= ndim <= 16, 1 <= nbins <= 128");
  const int64_t total = n * ndim;
  const int64_t per_block = (int64_t)CF_MARG_THREADS * CF_MARG_PER_THREAD;
  int64_t blocks = (total + per_block - 1) / per_block;
  if (blocks > 8192) blocks = 8192;  // grid-stride beyond: 32 workgroups per CU keep the loads in flight
  const size_t lds = ((size_t)ndim * (nbins + 1) + ndim) * sizeof(double);
  hipLaunchKernelGGL(marg_bin_kernel, dim3((unsigned)blocks), dim3(CF_MARG_THREADS), lds, (hipStream_t)hip_stream, d_x, total,
                     (int)ndim, (int)nbins, d_edges, d_idx, (int)(((uintptr_t)d_idx & 3) == 0));
  return cf_launch_status("cf_marg_bin");
}

extern "C" int cf_marg_hist(const uint8_t* d_idx, const double* d_w, double w_max, int64_t n, int32_t ndim, int32_t nbins,
                            const int32_t* pairs, int32_t npairs, int64_t* d_h1, int64_t* d_h2, int32_t n_segments,
                            void* hip_stream) {
  if (!d_idx || !d_h1) return cf_set_error(CF_ERR_INVALID, "cf_marg_hist: null argument");
  if (!marg_shape_ok(n, ndim, nbins))
    return cf_set_error(CF_ERR_INVALID, "cf_marg_hist: need 1 <= n <= 2^31 - 1, 1 <= ndim <= 16, 1 <= nbins <= 128");
  if (npairs < 0 || npairs > CF_MARG_MAX_PAIRS || (npairs > 0 && (!pairs || !d_h2)))
    return cf_set_error(CF_ERR_INVALID, "cf_marg_hist: need 0 <= npairs <= 256, with the pair list and d_h2 if npairs > 0");
  if (n_segments < 0 || n_segments > CF_MARG_MAX_SEGMENTS)
    return cf_set_error(CF_ERR_INVALID, "cf_marg_hist: need 0 <= n_segments <= 65536 (0: chosen by the library)");
  if (d_w && !(w_max > 0.0 && std::isfinite(w_max)))
    return cf_set_error(CF_ERR_INVALID, "cf_marg_hist: weighted histograms need a finite w_max > 0 (the largest weight)");
  marg_pairs pr;
  for (int p = 0; p < npairs; ++p) {
    const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= ndim || b < 0 || b >= ndim) return cf_set_error(CF_ERR_INVALID, "cf_marg_hist: pair index out of range");
    pr.a[p] = (uint8_t)a;
    pr.b[p] = (uint8_t)b;
  }
  const bool weighted = d_w != nullptr;
  const size_t cnt = weighted ? 8 : 4;
  const size_t lds1 = (size_t)ndim * nbins * cnt, lds2 = (size_t)nbins * nbins * cnt;
  // automatic geometry: enough workgroups to fill the CUs at the occupancy the LDS histogram allows, at least 4096 rows each
  int nseg1 = n_segments, nseg2 = n_segments;
  if (n_segments == 0) {
    const int64_t most = (n + 4095) / 4096;
    const int64_t per_cu = 163840 / (int64_t)(lds2 > 20480 ? lds2 : 20480);  // 1 .. 8 workgroups per CU
    int64_t want = (256 * per_cu + (npairs > 0 ? npairs : 1) - 1) / (npairs > 0 ? npairs : 1);
    nseg2 = (int)(want < most ? want : most);
    nseg1 = (int)(2048 < most ? 2048 : most);
  }
  const double two_s = weighted ? ldexp(1.0, 62 - marg_ceil_log2(n)) : 0.0;
  hipStream_t st = (hipStream_t)hip_stream;
  auto k1 = weighted ? marg_hist1_kernel<unsigned long long, true> : marg_hist1_kernel<unsigned int, false>;
  auto k2 = weighted ? marg_hist2_kernel<unsigned long long, true> : marg_hist2_kernel<unsigned int, false>;
  if (!marg_allow_lds(k1, lds1) || (npairs > 0 && !marg_allow_lds(k2, lds2)))
    return cf_set_error(CF_ERR_HIP, "cf_marg_hist: the device refused the LDS histogram size");
  if (hipMemsetAsync(d_h1, 0, (size_t)ndim * nbins * sizeof(int64_t), st) != hipSuccess ||
      (npairs > 0 && hipMemsetAsync(d_h2, 0, (size_t)npairs * nbins * nbins * sizeof(int64_t), st) != hipSuccess))
    return cf_set_error(CF_ERR_HIP, "cf_marg_hist: clearing the histograms failed");
  hipLaunchKernelGGL(k1, dim3((unsigned)nseg1), dim3(CF_MARG_THREADS), lds1, st, d_idx, d_w, w_max, two_s, n, (int)ndim, (int)nbins,
                     reinterpret_cast<unsigned long long*>(d_h1));
  if (npairs > 0)
    hipLaunchKernelGGL(k2, dim3((unsigned)nseg2, (unsigned)npairs), dim3(CF_MARG_THREADS), lds2, st, d_idx, d_w, w_max, two_s, n,
                       (int)ndim, (int)nbins, pr, reinterpret_cast<unsigned long long*>(d_h2));
  return cf_launch_status("cf_marg_hist");
}
