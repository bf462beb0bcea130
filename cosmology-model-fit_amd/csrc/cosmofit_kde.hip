// cosmofit_kde.hip — all-pairs isotropic Gaussian kernel sums on whitened points: the density step of the parameter-shift
// estimator (tension.py), n queries x n samples x one exp.
//
//   out[i] = sum over j != self(i) of  t_ij,        t_ij = w_j * exp(-0.5 * |q_i - y_j|^2),   i < m, j < n
//   sq[i]  = sum over the same j of    t_ij^2       (optional)
//
// Shape: the N-body one.  A workgroup of CF_KDE_THREADS threads owns CF_KDE_THREADS * CF_KDE_QPT queries, each thread holding
// its CF_KDE_QPT queries in registers (the dimension is a template parameter, 1 .. CF_KDE_MAX_NDIM).  Samples and weights are
// staged through LDS a tile of CF_KDE_TILE samples at a time; in the inner loop every lane reads the same sample, so the LDS
// reads are broadcasts without bank conflicts.  Differences are formed directly as q - y (no |q|^2 + |y|^2 - 2 q.y form: exp
// binds here, not the distance, and the direct form has no cancellation).
//
// ORDER OF SUMMATION (fixed; a function of n alone).  The samples are cut into slices of CF_KDE_SLICE consecutive samples
// (the last one shorter).  Within a slice the terms of a query are added one by one in ascending j to a partial sum that
// starts at 0.0; |q - y|^2 is accumulated over the coordinates in ascending order with fused multiply-adds, t^2 enters the sq
// partial with one fused multiply-add.  The partial sums of the slices are then added in ascending slice order to a total that
// starts at 0.0.  Tiles only stage data and do not appear in the order.  So the bits of out[i] and sq[i] depend on the
// samples, the weights, the query and self(i) only: not on m, not on the position of i in the call, not on the stream, not on
// repetition, and not on which of the two launch forms below ran.
//
// Two launch forms compute that same order.  "Direct": one workgroup per query block walks every slice and writes out / sq
// itself; it needs no workspace and is used when the query blocks alone fill the device.  "Split": one workgroup per (query
// block, slice) stores its partial to a per-call workspace [n_slices, m] with plain vector stores, and kde_combine_kernel adds
// the partials of a query in ascending slice order.  Split is what keeps m = 1, n = 10^6 from being one serial loop.  The
// workspace is allocated and freed in stream order inside the call; there is no global state.  If the allocation is refused
// the direct form runs instead: same bits, fewer workgroups.
//
// Leave-one-out is exact: the term j == self(i) = self_offset + i is replaced by +0.0 inside the loop, before it is added
// (adding +0.0 to a sum of non-negative terms changes no bit, so this is the sum without that term); nothing is subtracted
// afterwards.  A zero weight gives a term of +0.0 likewise.
//
// A plain sum is enough: every exponent is <= 0, so nothing overflows.  exp(-0.5 r^2) is subnormal from r = 37.7 and exactly
// 0.0 from r = 38.6, so a query more than ~37 units from every sample gets 0.0.  No log-sum-exp rescaling.
// A NaN or infinite coordinate in query i gives NaN in row i (out and sq) and touches no other row.  Samples and weights are
// taken as finite (the Python layer rejects others).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"

#define CF_KDE_THREADS 256
#define CF_KDE_QPT 2  // queries per thread: two independent exp chains per lane
#define CF_KDE_QBLOCK (CF_KDE_THREADS * CF_KDE_QPT)
static_assert(CF_KDE_QBLOCK == CF_KDE_QUERY_BLOCK, "the header states the queries per workgroup");
static_assert(CF_KDE_SLICE % CF_KDE_TILE == 0, "a slice is a whole number of tiles");
static_assert(CF_KDE_TILE <= CF_KDE_THREADS, "one thread stages one weight of a tile");

// The split form is chosen while the query blocks alone are fewer than CF_KDE_SPLIT_BELOW_BLOCKS (two workgroups per CU of an
// MI355X) and its workspace stays within this many bytes
#define CF_KDE_MAX_WORKSPACE ((int64_t)1 << 27)

// One slice [j0, j1) for the CF_KDE_QPT queries of this thread: acc / acc2 += terms in ascending j.  Every thread of the
// workgroup calls this (it holds barriers); a thread without a query carries zeros and stores nothing later.
template <int D>
__device__ __forceinline__ void kde_slice(const double* __restrict__ y, const double* __restrict__ w, int64_t j0, int64_t j1,
                                          const double (&qv)[CF_KDE_QPT][D], const int64_t (&self)[CF_KDE_QPT],
                                          double (&acc)[CF_KDE_QPT], double (&acc2)[CF_KDE_QPT], double* __restrict__ lds_y,
                                          double* __restrict__ lds_w) {
  for (int64_t t0 = j0; t0 < j1; t0 += CF_KDE_TILE) {
    const int cnt = (int)(j1 - t0 < CF_KDE_TILE ? j1 - t0 : CF_KDE_TILE);
    __syncthreads();  // the previous tile has been read by everyone
    const double* src = y + t0 * D;
    for (int e = threadIdx.x; e < cnt * D; e += CF_KDE_THREADS) lds_y[e] = src[e];
    if ((int)threadIdx.x < cnt) lds_w[threadIdx.x] = w ? w[t0 + threadIdx.x] : 1.0;
    __syncthreads();
#pragma unroll 2
    for (int jj = 0; jj < cnt; ++jj) {
      double yv[D];
#pragma unroll
      for (int c = 0; c < D; ++c) yv[c] = lds_y[jj * D + c];  // the same address in every lane: a broadcast
      const double wj = lds_w[jj];
      const int64_t j = t0 + jj;
#pragma unroll
      for (int k = 0; k < CF_KDE_QPT; ++k) {
        double r2 = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
          const double df = qv[k][c] - yv[c];
          r2 = fma(df, df, r2);
        }
        double t = wj * exp(-0.5 * r2);
        t = j == self[k] ? 0.0 : t;
        acc[k] += t;
        acc2[k] = fma(t, t, acc2[k]);
      }
    }
  }
}

// split == 0: grid (query blocks), writes out / sq.  split == 1: grid (query blocks, slices), writes the partials of slice
// blockIdx.y to out / sq taken as [n_slices, m].
template <int D>
__global__ void __launch_bounds__(CF_KDE_THREADS)
kde_sum_kernel(const double* __restrict__ y, const double* __restrict__ w, int64_t n, const double* __restrict__ q, int64_t m,
               int64_t self_offset, int split, double* __restrict__ out, double* __restrict__ sq) {
  __shared__ double lds_y[CF_KDE_TILE * D];
  __shared__ double lds_w[CF_KDE_TILE];
  double qv[CF_KDE_QPT][D];
  int64_t self[CF_KDE_QPT], row[CF_KDE_QPT];
  bool finite[CF_KDE_QPT];
#pragma unroll
  for (int k = 0; k < CF_KDE_QPT; ++k) {
    row[k] = (int64_t)blockIdx.x * CF_KDE_QBLOCK + k * CF_KDE_THREADS + threadIdx.x;  // consecutive lanes, consecutive rows
    const bool live = row[k] < m;
    finite[k] = true;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      qv[k][c] = live ? q[row[k] * D + c] : 0.0;
      finite[k] = finite[k] && isfinite(qv[k][c]);
    }
    self[k] = live && self_offset >= 0 ? self_offset + row[k] : -1;
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int64_t n_slices = (n + CF_KDE_SLICE - 1) / CF_KDE_SLICE;
  const int64_t s_begin = split ? blockIdx.y : 0, s_end = split ? s_begin + 1 : n_slices;
  double tot[CF_KDE_QPT], tot2[CF_KDE_QPT];
#pragma unroll
  for (int k = 0; k < CF_KDE_QPT; ++k) tot[k] = tot2[k] = 0.0;
  for (int64_t s = s_begin; s < s_end; ++s) {
    const int64_t j0 = s * CF_KDE_SLICE, j1 = j0 + CF_KDE_SLICE < n ? j0 + CF_KDE_SLICE : n;
    double acc[CF_KDE_QPT], acc2[CF_KDE_QPT];
#pragma unroll
    for (int k = 0; k < CF_KDE_QPT; ++k) acc[k] = acc2[k] = 0.0;
    kde_slice<D>(y, w, j0, j1, qv, self, acc, acc2, lds_y, lds_w);
#pragma unroll
    for (int k = 0; k < CF_KDE_QPT; ++k) {
      tot[k] += finite[k] ? acc[k] : nan;
      tot2[k] += finite[k] ? acc2[k] : nan;
    }
  }
  const int64_t base = split ? (int64_t)blockIdx.y * m : 0;
#pragma unroll
  for (int k = 0; k < CF_KDE_QPT; ++k)
    if (row[k] < m) {
      out[base + row[k]] = tot[k];
      if (sq) sq[base + row[k]] = tot2[k];
    }
}

// out[i] = part[0][i] + part[1][i] + ... in ascending slice order, from 0.0: the order the direct form uses.
extern "C" __global__ void __launch_bounds__(CF_KDE_THREADS)
kde_combine_kernel(const double* __restrict__ part, const double* __restrict__ part2, int64_t n_slices, int64_t m,
                   double* __restrict__ out, double* __restrict__ sq) {
  const int64_t i = (int64_t)blockIdx.x * CF_KDE_THREADS + threadIdx.x;
  if (i >= m) return;
  double tot = 0.0, tot2 = 0.0;
  for (int64_t s = 0; s < n_slices; ++s) {
    tot += part[s * m + i];
    if (part2) tot2 += part2[s * m + i];
  }
  out[i] = tot;
  if (sq) sq[i] = tot2;
}

template <int D>
static void kde_launch(dim3 grid, hipStream_t st, const double* y, const double* w, int64_t n, const double* q, int64_t m,
                       int64_t self_offset, int split, double* out, double* sq) {
  hipLaunchKernelGGL(kde_sum_kernel<D>, grid, dim3(CF_KDE_THREADS), 0, st, y, w, n, q, m, self_offset, split, out, sq);
}

extern "C" int cf_kde_sum_device(const double* d_y, const double* d_w, int64_t n, int32_t ndim, const double* d_q, int64_t m,
                                 int64_t self_offset, double* d_out, double* d_sq, void* hip_stream) {
  if (!d_y || !d_q || !d_out) return cf_set_error(CF_ERR_INVALID, "cf_kde_sum_device: null argument (d_y, d_q and d_out are needed)");
  if (ndim < 1 || ndim > CF_KDE_MAX_NDIM) return cf_set_error(CF_ERR_INVALID, "cf_kde_sum_device: need 1 <= ndim <= 8");
  if (n < 1 || m < 1) return cf_set_error(CF_ERR_INVALID, "cf_kde_sum_device: need n >= 1 and m >= 1");
  if (n > ((int64_t)1 << 40) || m > ((int64_t)1 << 40))
    return cf_set_error(CF_ERR_INVALID, "cf_kde_sum_device: need n <= 2^40 and m <= 2^40");
  if (self_offset < -1 || (self_offset >= 0 && self_offset + m > n))
    return cf_set_error(CF_ERR_INVALID, "cf_kde_sum_device: need self_offset = -1 (none) or 0 <= self_offset, self_offset + m <= n "
                                        "(query i is sample self_offset + i)");
  hipStream_t st = (hipStream_t)hip_stream;
  const int64_t q_blocks = (m + CF_KDE_QBLOCK - 1) / CF_KDE_QBLOCK;
  const int64_t n_slices = (n + CF_KDE_SLICE - 1) / CF_KDE_SLICE;
  if (q_blocks > (int64_t)INT32_MAX) return cf_set_error(CF_ERR_INVALID, "cf_kde_sum_device: too many queries for one call");
  // the split form: enough workgroups when the queries are few
  double* work = nullptr;
  const int64_t work_doubles = n_slices * m * (d_sq ? 2 : 1);
  if (n_slices > 1 && n_slices <= 65535 && q_blocks < CF_KDE_SPLIT_BELOW_BLOCKS &&
      work_doubles * (int64_t)sizeof(double) <= CF_KDE_MAX_WORKSPACE) {
    if (hipMallocAsync(reinterpret_cast<void**>(&work), (size_t)work_doubles * sizeof(double), st) != hipSuccess) {
      (void)hipGetLastError();  // refused: the direct form computes the same bits
      work = nullptr;
    }
  }
  const int split = work != nullptr;
  const dim3 grid((unsigned)q_blocks, split ? (unsigned)n_slices : 1u);
  double* o = split ? work : d_out;
  double* o2 = split ? (d_sq ? work + n_slices * m : nullptr) : d_sq;
  switch (ndim) {
    case 1: kde_launch<1>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
    case 2: kde_launch<2>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
    case 3: kde_launch<3>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
    case 4: kde_launch<4>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
    case 5: kde_launch<5>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
    case 6: kde_launch<6>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
    case 7: kde_launch<7>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
    default: kde_launch<8>(grid, st, d_y, d_w, n, d_q, m, self_offset, split, o, o2); break;
  }
  hipError_t err = hipGetLastError();
  if (split) {
    if (err == hipSuccess) {
      hipLaunchKernelGGL(kde_combine_kernel, dim3((unsigned)((m + CF_KDE_THREADS - 1) / CF_KDE_THREADS)), dim3(CF_KDE_THREADS), 0, st,
                         (const double*)o, (const double*)o2, n_slices, m, d_out, d_sq);
      err = hipGetLastError();
    }
    const hipError_t freed = hipFreeAsync(work, st);  // stream-ordered: after the combine kernel
    if (err == hipSuccess) err = freed;
  }
  return err == hipSuccess ? CF_OK : cf_set_error(CF_ERR_HIP, "cf_kde_sum_device: launch failed");
}
