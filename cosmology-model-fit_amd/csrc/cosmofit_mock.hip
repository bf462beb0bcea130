// cosmofit_mock.hip — mock-data ensembles: one likelihood whose data differ per row (include/cosmofit.h: cf_mock_eval_device,
// cf_mock_normals; the launcher and the argument checks are in cosmofit_api.hip, the driver is
// cosmology-model-fit_amd/mocks.py).
//
// The scripts quote a Delta chi^2 and read it through Wilks' theorem ("delta chi2 = 11.7 -> 3.4 sigma", sn/pantheon_dipole.py:172;
// sn/union3_1.py:145-161) with parameters on box faces, where the theorem does not hold.  The calibration is a Monte-Carlo one:
// thousands of data sets drawn from the null, both models fitted to each.  All data enter the residual linearly, so for the data
// `data + d_k` of mock k
//     chi2_k(theta) = chi2(theta) + 2 r(theta) . g_k + c_k,   g_k = C^-1 d_k,  c_k = d_k . g_k:
// no second handle, no second factor, the hot kernels untouched.  The residual rows are the ones the accessor path of the
// likelihood leaves in the handle's workspace (as for cosmofit_resid.hip), one chunk of rows at a time.
//
// mock_shift_kernel: ONE WAVE PER ROW, four rows per 256-thread workgroup.  The row's mock index selects a row of g, read once
// from HBM with 64 consecutive doubles per load; the residual row was written a kernel ago and comes from L2.  No LDS, no
// barrier, no atomics: every sum is lane-strided partials (lane l takes i = l, l + 64, ...) combined by the fixed xor butterfly
// of resid_sample_kernel (32, 16, .., 1), one block after another in the order SN, BAO, CMB, so a row's bits depend on
// (theta, k) only -- not on S, the row's position, the chunking or device / host pointers.
//
// mock_normals_kernel: one thread per value, the ensemble's counter-based generator (cf_rng.h) with counter k n + i.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/cosmofit.h"
#include "cf_host.h"
#include "cf_rng.h"
#include "cosmofit_mock.h"

#define MK_TPB 256
#define MK_ROWS_PER_WG (MK_TPB / 64)

__device__ __forceinline__ double mock_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

__global__ void __launch_bounds__(MK_TPB) mock_shift_kernel(cf_mock_args a, int64_t rows, const int32_t* __restrict__ mock,
                                                            double* __restrict__ out, double* __restrict__ cross) {
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * MK_ROWS_PER_WG + (threadIdx.x >> 6);
  if (s >= rows) return;  // whole waves leave: no cross-lane step below has a missing partner
  const int k = mock[s];  // wave-uniform
  const double base = a.base[s];
  double x_sn = 0.0, x_bao = 0.0, x_cmb = 0.0, value;
  if (k < 0) {
    value = base;  // the observed data
  } else if (k >= a.n_mocks) {
    value = __builtin_nan("");  // no such mock: nothing of the set is read
  } else {
    if (a.n_sn > 0) {
      const double* __restrict__ r = a.sn_rows + s * a.sn_pitch;
      const double* __restrict__ g = a.g_sn + (int64_t)k * a.n_sn;
      double p = 0.0;
      for (int i = lane; i < a.n_sn; i += 64) p += r[i] * g[i];
      x_sn = mock_wave_sum(p);
    }
    if (a.n_bao > 0) {
      const double* __restrict__ t = a.bao_theory + s * (int64_t)a.n_bao;
      const double* __restrict__ g = a.g_bao + (int64_t)k * a.n_bao;
      double p = 0.0;
      for (int i = lane; i < a.n_bao; i += 64) p += (a.bao_val[i] - t[i]) * g[i];
      x_bao = mock_wave_sum(p);
    }
    if (a.n_cmb > 0) {
      double p = 0.0;
      if (lane < 3) {
        const double prior = lane == 0 ? a.cmb_prior[0] : (lane == 1 ? a.cmb_prior[1] : a.cmb_prior[2]);
        p = (prior - a.b8[8 * s + 2 + lane]) * a.g_cmb[(int64_t)k * 3 + lane];
      }
      x_cmb = mock_wave_sum(p);
    }
    const double shift = 2.0 * ((x_sn + x_bao) + x_cmb) + a.c[k];
    if (a.out_kind == CF_OUT_CHI2)
      value = base + shift;
    else  // a row the likelihood rejects (outside the box, a non-finite chi^2) stays rejected whatever its residuals hold
      value = base == -INFINITY ? base : base - 0.5 * shift;
  }
  if (lane == 0) {
    out[s] = value;
    if (cross) {
      cross[3 * s + 0] = x_sn;
      cross[3 * s + 1] = x_bao;
      cross[3 * s + 2] = x_cmb;
    }
  }
}

__global__ void __launch_bounds__(MK_TPB) mock_normals_kernel(uint64_t key, int64_t id0, int64_t count, double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * MK_TPB;
  for (int64_t e = (int64_t)blockIdx.x * MK_TPB + threadIdx.x; e < count; e += stride) out[e] = ens_normal(key, 0, id0 + e);
}

int cf_mock_launch(const cf_mock_args& a, int64_t rows, const int32_t* d_mock, double* d_out, double* d_cross, hipStream_t st) {
  hipLaunchKernelGGL(mock_shift_kernel, dim3((unsigned)((rows + MK_ROWS_PER_WG - 1) / MK_ROWS_PER_WG)), dim3(MK_TPB), 0, st, a, rows,
                     d_mock, d_out, d_cross);
  return cf_launch_status("cf_mock_eval_device");
}

extern "C" int cf_mock_normals(uint64_t key, int64_t k0, int64_t K, int32_t n, double* d_out, void* hip_stream) {
  if (k0 < 0 || K < 0 || n < 1) return cf_set_error(CF_ERR_INVALID, "cf_mock_normals: k0 >= 0, K >= 0 and n >= 1 are required");
  const int64_t lim = (int64_t)1 << 62;
  if (k0 > lim || K > lim || k0 + K > lim / n) return cf_set_error(CF_ERR_INVALID, "cf_mock_normals: (k0 + K) n must not exceed 2^62");
  if (K == 0) return CF_OK;
  if (!d_out) return cf_set_error(CF_ERR_INVALID, "cf_mock_normals: null output");
  const int64_t count = K * n, blocks = (count + MK_TPB - 1) / MK_TPB;
  hipLaunchKernelGGL(mock_normals_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(MK_TPB), 0, (hipStream_t)hip_stream,
                     key, k0 * n, count, d_out);
  return cf_launch_status("cf_mock_normals");
}
