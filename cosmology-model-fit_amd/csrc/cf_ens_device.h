// cf_ens_device.h -- the device code of the ensemble moves that cosmofit_ensemble.hip (one ensemble, sharded over processes)
// and cosmofit_replica.hip (R independent ensembles per launch) share: the splits of a step, the rows of a complementary set,
// the KDE fit, the log Hastings factor of the KDE move and the three proposals.  Both files call the SAME functions with the
// same arguments for a given ensemble, so replica r of a batched run is the chain of a stand-alone ensemble to the bit: every
// per-element expression and every reduction order below is part of that promise.
#ifndef CF_ENS_DEVICE_H
#define CF_ENS_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "cf_rng.h"

#define CF_ENS_MAX_NDIM 16

// ens_mix / ens_uniform / ens_normal: cf_rng.h (shared with cosmofit_mock.hip)

// ---- the splits of a step (emcee's RedBlueMove: `nsplits` sets updated in turn, each proposing from the others) ----------
// Walkers are taken in consecutive groups of S = n_splits (S = 2: pairs -- StretchMove, KDEMove; S = 3: triples -- emcee's
// DEMove sets nsplits = 3): walker S c + b belongs to split perm_c[b], where perm_c is the identity for split_key == 0 (fixed
// classes id mod S) and otherwise a counter-based random permutation of (split_key, c), re-drawn every step.  Every split
// then holds exactly one member of every group, so any contiguous shard owns its fair share of each split, and the partition
// does not depend on the walkers' positions (detailed balance as for emcee's shuffled index array).
// S = 2: perm = (flip, 1 - flip) with flip = the top bit of the same two-round hash as ens_uniform (ensemble.py: split_perm).
__device__ __host__ __forceinline__ uint64_t ens_mix_h(uint64_t x) {
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __host__ __forceinline__ uint64_t ens_group_hash(uint64_t split_key, int64_t c) {
  return ens_mix_h(ens_mix_h((uint64_t)c * 0x9E3779B97F4A7C15ull + split_key) + 0x9E3779B97F4A7C15ull);
}
// split of member b of group c, packed permutations of three: entry p holds perm[b] in bits 2b .. 2b + 1
// p: 0 = (0,1,2), 1 = (0,2,1), 2 = (1,0,2), 3 = (1,2,0), 4 = (2,0,1), 5 = (2,1,0)
__device__ __host__ __forceinline__ int ens_split_of(uint64_t split_key, int S, int64_t c, int b) {
  if (split_key == 0) return b;
  const uint64_t x = ens_group_hash(split_key, c);
  if (S == 2) return b ^ (int)(x >> 63);
  const unsigned p = (unsigned)(((x >> 40) * 6ull) >> 24);  // floor(6 u), u = the top 24 bits as a fraction
  const unsigned packed = 0x24u | (0x18u << 6) | (0x21u << 12) | (0x09u << 18) | (0x12u << 24);  // p = 0..4; p = 5 below
  const unsigned e = p == 5 ? 0x06u : (packed >> (6 * p)) & 0x3Fu;
  return (int)((e >> (2 * b)) & 3u);
}
// member b of group c that belongs to split s (exactly one)
__device__ __host__ __forceinline__ int ens_member_in(uint64_t split_key, int S, int64_t c, int s) {
  for (int b = 0; b < S - 1; ++b)
    if (ens_split_of(split_key, S, c, b) == s) return b;
  return S - 1;
}

// row m of the complementary set of split s: the walkers of every other split in ascending index order, i.e. the r-th
// (r = m mod (S - 1)) member of group c = m / (S - 1) that is not in split s
__device__ __forceinline__ const double* comp_row(const double* all_pos, int ndim, int S, int s, uint64_t split_key, int64_t m) {
  if (S == 2) return all_pos + (2 * m + ens_member_in(split_key, 2, m, 1 - s)) * ndim;
  const int64_t c = m / (S - 1);
  int r = (int)(m - c * (S - 1)), b = 0;
  for (; b < S - 1; ++b)
    if (ens_split_of(split_key, S, c, b) != s && r-- == 0) break;
  return all_pos + (S * c + b) * ndim;
}

// KDE preparation for a compile-time dimension D <= 8 (one 256-thread workgroup): ONE pass over the complementary set for the first
// and second moments of x - x_ref (x_ref = its first row, inside the cloud, so the subtraction in the covariance cancels nothing it
// needs), every row loaded once with unconditional loads; covariance, Cholesky factor and inverse by thread 0 in registers; the
// whitened set in a second pass.  The run-time-dimension form in ens_kde_prepare_body reads the rows D + D (D + 1) / 2 times with a
// block reduction each, branches around every element load and does its linear algebra through LDS: 57 us at nc = 2048, D = 4
// (profiles/r02_kde_kernels_ab.txt).
template <int D>
__device__ __forceinline__ void kde_prepare_small(const double* __restrict__ all_pos, int64_t nc, int S, int half, uint64_t split_key, double h,
                                                  double* __restrict__ params, double* __restrict__ wc) {
  constexpr int NM = D + D * (D + 1) / 2;
  __shared__ double wsum[4][NM], tot[NM], inv_s[D * D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double x0[D], mom[NM];
  {
    const double* r0 = comp_row(all_pos, D, S, half, split_key, 0);
#pragma unroll
    for (int k = 0; k < D; ++k) x0[k] = r0[k];
  }
#pragma unroll
  for (int k = 0; k < NM; ++k) mom[k] = 0.0;
  for (int64_t c = tid; c < nc; c += 256) {
    const double* r = comp_row(all_pos, D, S, half, split_key, c);
    double dd[D];
#pragma unroll
    for (int k = 0; k < D; ++k) dd[k] = r[k] - x0[k];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      mom[a] += dd[a];
#pragma unroll
      for (int b = 0; b <= a; ++b) mom[D + a * (a + 1) / 2 + b] += dd[a] * dd[b];
    }
  }
#pragma unroll
  for (int k = 0; k < NM; ++k) {
    double v = mom[k];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) wsum[wave][k] = v;
  }
  __syncthreads();
  if (tid < NM) tot[tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
  __syncthreads();
  if (tid == 0) {
    double Lm[D][D], It[D][D];
#pragma unroll
    for (int j = 0; j < D; ++j) {  // Cholesky (lower) of the covariance h^2 (S2 - S1 S1^T / n) / (n - 1)
      auto cov = [&](int a, int b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        return (tot[D + hi * (hi + 1) / 2 + lo] - tot[hi] * tot[lo] / (double)nc) / (double)(nc - 1) * (h * h);
      };
      double sj = cov(j, j);
#pragma unroll
      for (int k = 0; k < j; ++k) sj -= Lm[j][k] * Lm[j][k];
      Lm[j][j] = sqrt(sj);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        if (i < j) Lm[i][j] = 0.0;
        if (i > j) {
          double t = cov(i, j);
#pragma unroll
          for (int k = 0; k < j; ++k) t -= Lm[i][k] * Lm[j][k];
          Lm[i][j] = t / Lm[j][j];
        }
      }
    }
    double log_det = 0.0;
#pragma unroll
    for (int col = 0; col < D; ++col) {  // inv(chol) by forward substitution, stored transposed: It[k][m] = inv[m][k]
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double t = i == col ? 1.0 : 0.0;
#pragma unroll
        for (int k = col; k < i; ++k) t -= Lm[i][k] * It[col][k];
        It[col][i] = i < col ? 0.0 : t / Lm[i][i];
      }
      log_det += log(Lm[col][col]);
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        params[a * D + b] = Lm[a][b];
        params[D * D + a * D + b] = It[a][b];
        inv_s[a * D + b] = It[a][b];
      }
    params[2 * D * D] = -log((double)nc) - 0.5 * D * log(2.0 * 3.14159265358979323846) - log_det;
  }
  __syncthreads();
  double inv[D * D];
#pragma unroll
  for (int k = 0; k < D * D; ++k) inv[k] = inv_s[k];
  for (int64_t c = tid; c < nc; c += 256) {  // whitened complementary set: wc = comp @ inv_t
    const double* r = comp_row(all_pos, D, S, half, split_key, c);
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = r[k];
#pragma unroll
    for (int m = 0; m < D; ++m) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) t += x[k] * inv[k * D + m];
      wc[c * D + m] = t;
    }
  }
}

// ---- KDE (scipy.stats.gaussian_kde, bw_method="silverman", as emcee's KDEMove uses it) -----------------
// params = { chol[d*d] (lower), chol_inv_t[d*d], log_norm }, wc = comp @ chol_inv_t  [nc * d]
// The work of ONE 256-thread workgroup on one ensemble's complementary set (every thread of the workgroup calls it).
__device__ __forceinline__ void ens_kde_prepare_body(const double* __restrict__ all_pos, int64_t nc, int ndim, int S, int half,
                                                     uint64_t split_key, double* __restrict__ params, double* __restrict__ wc) {
  __shared__ double red[256];
  __shared__ double mean[CF_ENS_MAX_NDIM], cov[CF_ENS_MAX_NDIM * CF_ENS_MAX_NDIM], chol[CF_ENS_MAX_NDIM * CF_ENS_MAX_NDIM],
      inv_t[CF_ENS_MAX_NDIM * CF_ENS_MAX_NDIM];
  const int tid = threadIdx.x, d = ndim;
  auto block_sum = [&](double v) {
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
  };
  const double h = pow((double)nc * (d + 2) / 4.0, -1.0 / (d + 4));  // silverman_factor
  if (d <= 8) {  // compile-time dimension: everything in registers, every load unconditional (see kde_prepare_small)
    switch (d) {
      case 1: kde_prepare_small<1>(all_pos, nc, S, half, split_key, h, params, wc); break;
      case 2: kde_prepare_small<2>(all_pos, nc, S, half, split_key, h, params, wc); break;
      case 3: kde_prepare_small<3>(all_pos, nc, S, half, split_key, h, params, wc); break;
      case 4: kde_prepare_small<4>(all_pos, nc, S, half, split_key, h, params, wc); break;
      case 5: kde_prepare_small<5>(all_pos, nc, S, half, split_key, h, params, wc); break;
      case 6: kde_prepare_small<6>(all_pos, nc, S, half, split_key, h, params, wc); break;
      case 7: kde_prepare_small<7>(all_pos, nc, S, half, split_key, h, params, wc); break;
      default: kde_prepare_small<8>(all_pos, nc, S, half, split_key, h, params, wc); break;
    }
    return;
  } else {
    for (int k = 0; k < d; ++k) {
      double s = 0.0;
      for (int64_t c = tid; c < nc; c += 256) s += comp_row(all_pos, d, S, half, split_key, c)[k];
      const double tot = block_sum(s);
      if (tid == 0) mean[k] = tot / (double)nc;
    }
    __syncthreads();
    for (int a = 0; a < d; ++a)
      for (int b = 0; b <= a; ++b) {
        double s = 0.0;
        for (int64_t c = tid; c < nc; c += 256) {
          const double* r = comp_row(all_pos, d, S, half, split_key, c);
          s += (r[a] - mean[a]) * (r[b] - mean[b]);
        }
        const double tot = block_sum(s);
        if (tid == 0) cov[a * d + b] = cov[b * d + a] = tot / (double)(nc - 1) * (h * h);
      }
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < d * d; ++i) chol[i] = 0.0;
    for (int j = 0; j < d; ++j) {  // Cholesky, lower
      double s = cov[j * d + j];
      for (int k = 0; k < j; ++k) s -= chol[j * d + k] * chol[j * d + k];
      chol[j * d + j] = sqrt(s);
      for (int i = j + 1; i < d; ++i) {
        double t = cov[i * d + j];
        for (int k = 0; k < j; ++k) t -= chol[i * d + k] * chol[j * d + k];
        chol[i * d + j] = t / chol[j * d + j];
      }
    }
    // inv(chol) by forward substitution, stored transposed: inv_t[k][m] = inv[m][k]
    double log_det = 0.0;
    for (int col = 0; col < d; ++col) {
      for (int i = 0; i < d; ++i) {
        double t = i == col ? 1.0 : 0.0;
        for (int k = col; k < i; ++k) t -= chol[i * d + k] * inv_t[col * d + k];
        inv_t[col * d + i] = i < col ? 0.0 : t / chol[i * d + i];
      }
      log_det += log(chol[col * d + col]);
    }
    for (int i = 0; i < d * d; ++i) {
      params[i] = chol[i];
      params[d * d + i] = inv_t[i];
    }
    params[2 * d * d] = -log((double)nc) - 0.5 * d * log(2.0 * 3.14159265358979323846) - log_det;
  }
  __syncthreads();
  for (int64_t c = tid; c < nc; c += 256) {
    const double* r = comp_row(all_pos, d, S, half, split_key, c);
    for (int m = 0; m < d; ++m) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s += r[k] * inv_t[k * d + m];
      wc[c * d + m] = s;
    }
  }
}

// log Hastings factor of the KDE move, log kde(x) - log kde(q), of ONE active walker (position xa, proposal q) by one 256-thread
// WORKGROUP: thread t takes the complementary walkers t, t + 256, ...; log-sum-exp in two passes over registers (maximum, then
// the sum), both reduced over the workgroup (wave shuffles + four LDS slots).  One WAVE per walker left the chip with 2 waves per
// SIMD on chains of dependent exp evaluations: 44 us per half-step of 2048 walkers against 28 us (profiles/r02_kde_kernels_ab.txt).
#define CF_ENS_KDE_CHUNK 8  // complementary walkers per thread held in registers at a time
__device__ __forceinline__ void ens_kde_logfactor_body(const double* __restrict__ xa, int64_t nc, int ndim,
                                                       const double* __restrict__ kde_params, const double* __restrict__ wc,
                                                       const double* __restrict__ q, double* __restrict__ log_factor_i) {
  __shared__ double xch[4][4];  // per wave {max a, max q, sum a, sum q}
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = ndim;
  const double* inv_t = kde_params + d * d;
  const double log_norm = kde_params[2 * d * d];
  double wa[CF_ENS_MAX_NDIM], wq[CF_ENS_MAX_NDIM];
  for (int m = 0; m < d; ++m) {
    double sa = 0.0, sq = 0.0;
    for (int k = 0; k < d; ++k) {
      sa += xa[k] * inv_t[k * d + m];
      sq += q[k] * inv_t[k * d + m];
    }
    wa[m] = sa;
    wq[m] = sq;
  }
  auto wave_max = [](double v) {
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
  };
  auto wave_add = [](double v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  };
  // running (maximum, scaled sum) per point over chunks of 256 * CF_ENS_KDE_CHUNK complementary walkers
  double mxa = -INFINITY, mxq = -INFINITY, sa = 0.0, sq = 0.0;
  for (int64_t c0 = 0; c0 < nc; c0 += 256 * CF_ENS_KDE_CHUNK) {
    double ea[CF_ENS_KDE_CHUNK], eq[CF_ENS_KDE_CHUNK];
    double la = -INFINITY, lq = -INFINITY;
#pragma unroll
    for (int t = 0; t < CF_ENS_KDE_CHUNK; ++t) {
      const int64_t c = c0 + tid + 256 * t;
      ea[t] = eq[t] = -INFINITY;
      if (c < nc) {
        double da = 0.0, dq = 0.0;
        for (int m = 0; m < d; ++m) {
          const double w = wc[c * d + m];
          da += (wa[m] - w) * (wa[m] - w);
          dq += (wq[m] - w) * (wq[m] - w);
        }
        ea[t] = -0.5 * da;
        eq[t] = -0.5 * dq;
      }
      la = fmax(la, ea[t]);
      lq = fmax(lq, eq[t]);
    }
    la = wave_max(la);
    lq = wave_max(lq);
    if (lane == 0) {
      xch[wave][0] = la;
      xch[wave][1] = lq;
    }
    __syncthreads();
    const double na = fmax(mxa, fmax(fmax(xch[0][0], xch[1][0]), fmax(xch[2][0], xch[3][0])));
    const double nq = fmax(mxq, fmax(fmax(xch[0][1], xch[1][1]), fmax(xch[2][1], xch[3][1])));
    double pa = 0.0, pq = 0.0;
#pragma unroll
    for (int t = 0; t < CF_ENS_KDE_CHUNK; ++t) {
      pa += exp(ea[t] - na);  // exp(-inf) = 0 for the slots past nc
      pq += exp(eq[t] - nq);
    }
    pa = wave_add(pa);
    pq = wave_add(pq);
    if (lane == 0) {
      xch[wave][2] = pa;
      xch[wave][3] = pq;
    }
    __syncthreads();
    sa = sa * exp(mxa - na) + (((xch[0][2] + xch[1][2]) + xch[2][2]) + xch[3][2]);
    sq = sq * exp(mxq - nq) + (((xch[0][3] + xch[1][3]) + xch[2][3]) + xch[3][3]);
    mxa = na;
    mxq = nq;
    __syncthreads();  // xch is rewritten by the next chunk
  }
  if (tid == 0) *log_factor_i = ((mxa + log(sa)) + log_norm) - ((mxq + log(sq)) + log_norm);
}

// The proposal of ONE active walker (one thread): kind 0 stretch (emcee StretchMove, a), 1 DE (emcee DEMove, gamma0 = 2.38 /
// sqrt(2 ndim), sigma; an ordered pair j != k of the complementary set, which for emcee's DEMove is the other TWO thirds of the
// ensemble: n_splits = 3), 2 KDE (independence proposal from the Gaussian KDE of the complementary set).  all_pos [w * ndim] is the
// walker's own ensemble, id its index in it (the counter of every random draw), nc the size of the complementary set; y_i [ndim]
// receives the proposal and *log_factor_i the log of the Hastings factor (KDE: left to ens_kde_logfactor_body).
__device__ __forceinline__ void ens_propose_row(int kind, const double* __restrict__ all_pos, int64_t nc, int ndim, int S, int half,
                                                uint64_t split_key, int64_t id, uint64_t key0, double a, double de_sigma,
                                                const double* __restrict__ kde_params, double* __restrict__ y_i,
                                                double* __restrict__ log_factor_i) {
  const int d = ndim;
  const double* xa = all_pos + id * d;
  int64_t j = (int64_t)(ens_uniform(key0, 0, id) * (double)nc);
  j = j > nc - 1 ? nc - 1 : j;
  const double* cj = comp_row(all_pos, d, S, half, split_key, j);
  if (kind == 0) {
    const double t = (a - 1.0) * ens_uniform(key0, 1, id) + 1.0;
    const double z = t * t / a;
    for (int k = 0; k < d; ++k) y_i[k] = cj[k] + z * (xa[k] - cj[k]);
    *log_factor_i = (d - 1) * log(z);
  } else if (kind == 1) {
    int64_t k2 = (int64_t)(ens_uniform(key0, 1, id) * (double)(nc - 1));
    k2 = k2 > nc - 2 ? nc - 2 : k2;
    k2 += k2 >= j ? 1 : 0;
    const double* ck = comp_row(all_pos, d, S, half, split_key, k2);
    const double gamma = (2.38 / sqrt(2.0 * d)) * (1.0 + de_sigma * ens_normal(key0, 3, id));
    for (int k = 0; k < d; ++k) y_i[k] = xa[k] + gamma * (cj[k] - ck[k]);
    *log_factor_i = 0.0;
  } else {
    const double* chol = kde_params;
    double noise[CF_ENS_MAX_NDIM], q[CF_ENS_MAX_NDIM];
    for (int k = 0; k < d; ++k) noise[k] = ens_normal(key0, 4 + 2 * k, id);
    for (int r = 0; r < d; ++r) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s += noise[k] * chol[r * d + k];  // noise @ chol.T
      q[r] = cj[r] + s;
      y_i[r] = q[r];
    }
    // log_factor: ens_kde_logfactor_body (one workgroup per walker)
  }
}

#endif
