// cosmofit_mock.hip — mock-data ensembles: one likelihood whose data differ per row (include/cosmofit.h: cf_mock_eval_device,
// cf_mock_normals; the kernels, then the argument checks and the chunk loop; the driver is
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
#include "cf_handle.h"
#include "cf_rng.h"
#include "cf_wave.h"
#include "cosmofit_resid.h"

// Where the residual rows of a chunk lie (the accessor path's outputs in the handle's workspace, as cf_resid_src) and the
// mock set they are multiplied with.  A block with n = 0 is not shifted.
struct cf_mock_args {
  const double* sn_rows;     // [rows][sn_pitch] the SN residual rows
  const double* bao_theory;  // [rows][n_bao]; r = bao_val - theory
  const double* bao_val;     // [n_bao]
  const double* b8;          // [rows][8] small_blocks_kernel's outputs; the CMB theory vector is columns 2..4
  const double* base;        // [rows] the likelihood's own value for out_kind
  const double* g_sn;        // [n_mocks][n_sn]
  const double* g_bao;       // [n_mocks][n_bao]
  const double* g_cmb;       // [n_mocks][3]
  const double* c;           // [n_mocks]
  double cmb_prior[3];       // r = cmb_prior - vector
  int64_t sn_pitch;
  int32_t n_sn, n_bao, n_cmb, n_mocks, out_kind, pad;
};

#define MK_TPB 256
#define MK_ROWS_PER_WG (MK_TPB / 64)

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
      x_sn = wave_sum(p);
    }
    if (a.n_bao > 0) {
      const double* __restrict__ t = a.bao_theory + s * (int64_t)a.n_bao;
      const double* __restrict__ g = a.g_bao + (int64_t)k * a.n_bao;
      double p = 0.0;
      for (int i = lane; i < a.n_bao; i += 64) p += (a.bao_val[i] - t[i]) * g[i];
      x_bao = wave_sum(p);
    }
    if (a.n_cmb > 0) {
      double p = 0.0;
      if (lane < 3) {
        const double prior = lane == 0 ? a.cmb_prior[0] : (lane == 1 ? a.cmb_prior[1] : a.cmb_prior[2]);
        p = (prior - a.b8[8 * s + 2 + lane]) * a.g_cmb[(int64_t)k * 3 + lane];
      }
      x_cmb = wave_sum(p);
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

// One chunk of `rows` rows: d_out[s] and d_cross[3 s + b] (null: not wanted) for the mocks d_mock[s].
static int cf_mock_launch(const cf_mock_args& a, int64_t rows, const int32_t* d_mock, double* d_out, double* d_cross, hipStream_t st) {
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

// ------------------------------------------------------------------------------------------------
// Host side: the likelihood on per-row shifted data.  The residual rows come from the
// accessor path, one chunk of rows at a time into the handle's workspace, exactly as resid_run gets them (the CMB theory vector
// is columns 2..4 of r_blk); the likelihood's own value for out_kind lands in h->out and mock_shift_kernel adds the shift
// behind it on the same stream.
// ------------------------------------------------------------------------------------------------
extern "C" int cf_mock_check_args(int64_t n_sn, int32_t n_bao, int32_t has_cmb, int32_t is_quasar, int32_t n_devices,
                                  const cf_mock_set* set, const void* theta, int64_t S, const void* mock, int32_t out_kind,
                                  const void* out) {
  const std::string F = "cf_mock_eval: ";
  if (is_quasar) return cf_set_error(CF_ERR_UNSUPPORTED, F + "a quasar handle has no accessor path to take the residuals from");
  if (n_devices > 1) return cf_set_error(CF_ERR_UNSUPPORTED, F + "this handle spans several devices; use one handle per device");
  if (!set) return cf_set_error(CF_ERR_INVALID, F + "null cf_mock_set");
  if (set->struct_size != (int32_t)sizeof(cf_mock_set)) return cf_set_error(CF_ERR_INVALID, F + "cf_mock_set.struct_size mismatch");
  if (set->n_mocks < 1) return cf_set_error(CF_ERR_INVALID, F + "n_mocks must be >= 1");
  if (set->n_sn != 0 && n_sn <= 0) return cf_set_error(CF_ERR_INVALID, F + "this likelihood has no SN block");
  if (set->n_bao != 0 && n_bao <= 0) return cf_set_error(CF_ERR_INVALID, F + "this likelihood has no BAO block");
  if (set->n_cmb != 0 && !has_cmb) return cf_set_error(CF_ERR_INVALID, F + "this likelihood has no CMB block");
  if (set->n_sn != 0 && (int64_t)set->n_sn != n_sn) return cf_set_error(CF_ERR_INVALID, F + "cf_mock_set.n_sn is neither 0 nor the handle's n_sn");
  if (set->n_bao != 0 && set->n_bao != n_bao) return cf_set_error(CF_ERR_INVALID, F + "cf_mock_set.n_bao is neither 0 nor the handle's n_bao");
  if (set->n_cmb != 0 && set->n_cmb != 3) return cf_set_error(CF_ERR_INVALID, F + "cf_mock_set.n_cmb must be 0 or 3");
  if (set->n_sn == 0 && set->n_bao == 0 && set->n_cmb == 0) return cf_set_error(CF_ERR_INVALID, F + "no shifted block");
  if ((set->n_sn != 0 && !set->g_sn) || (set->n_bao != 0 && !set->g_bao) || (set->n_cmb != 0 && !set->g_cmb) || !set->c)
    return cf_set_error(CF_ERR_INVALID, F + "null array in cf_mock_set");
  if (out_kind < CF_OUT_CHI2 || out_kind > CF_OUT_LOGP) return cf_set_error(CF_ERR_INVALID, F + "bad out_kind");
  if (S < 0 || S > CF_RESID_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, F + "S out of range");
  if (S > 0 && (!theta || !mock || !out)) return cf_set_error(CF_ERR_INVALID, F + "null theta, mock or out");
  return CF_OK;
}

static int mock_check(cf_handle* h, const cf_mock_set* set, const void* theta, int64_t S, const void* mock, int32_t out_kind,
                      const void* out) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_mock_eval: null handle");
  return cf_mock_check_args(h->d.n_sn, h->d.n_bao, h->d.cmb_mode != 0 ? 1 : 0, h->qsr ? 1 : 0, 1 + (int32_t)h->peers.size(), set, theta,
                            S, mock, out_kind, out);
}

extern "C" int cf_mock_set_chunk(cf_handle* h, int64_t rows) { return set_chunk(h, &cf_handle::mock_chunk, rows, "cf_mock_set_chunk"); }

// Arguments checked.  Device pointers throughout (the set's arrays too).
static int mock_run(const HandleScope& hs, const cf_mock_set& set, const double* d_theta, int64_t S, const int32_t* d_mock,
                    int32_t out_kind, double* d_out, double* d_cross, hipStream_t st) {
  cf_handle* const h = hs.h;
  int rc;
  const int64_t chunk = std::min<int64_t>(S, h->mock_chunk > 0 ? h->mock_chunk : CF_MOCK_CHUNK);
  if ((rc = ensure_workspace(h, chunk))) return rc;
  if ((rc = resid_prepare(hs, chunk))) return rc;
  const cf_dev_desc& d = h->d;
  cf_mock_args a{};
  a.sn_rows = h->delta.as<const double>();
  a.sn_pitch = d.n_ld;
  a.bao_theory = h->r_bt.as<const double>();
  a.bao_val = d.bao_val;
  a.b8 = h->r_blk.as<const double>();
  a.base = h->out.as<const double>();
  a.g_sn = set.g_sn; a.g_bao = set.g_bao; a.g_cmb = set.g_cmb; a.c = set.c;
  for (int i = 0; i < 3; ++i) a.cmb_prior[i] = d.cmb_prior[i];
  a.n_sn = set.n_sn; a.n_bao = set.n_bao; a.n_cmb = set.n_cmb; a.n_mocks = set.n_mocks;
  a.out_kind = out_kind;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t m = std::min(chunk, S - s0);
    // a mu_corr buffer selects the accessor form of the per-walker kernel (residual rows in row layout), as in resid_run
    if ((rc = launch_path(h, d_theta + s0 * d.ndim, m, h->out.as<double>(), out_kind, st, nullptr,
                          d.n_sn > 0 ? h->r_mc.as<double>() : nullptr, h->r_blk.as<double>(),
                          d.n_bao > 0 ? h->r_bt.as<double>() : nullptr)))
      return rc;
    if ((rc = cf_mock_launch(a, m, d_mock + s0, d_out + s0, d_cross ? d_cross + 3 * s0 : nullptr, st))) return rc;
  }
  return CF_OK;
}

extern "C" int cf_mock_eval_device(cf_handle* h, const cf_mock_set* set, const double* d_theta, int64_t S, const int32_t* d_mock,
                                   int32_t out_kind, double* d_out, double* d_cross, void* hip_stream) {
  int rc = mock_check(h, set, d_theta, S, d_mock, out_kind, d_out);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  return mock_run(hs, *set, d_theta, S, d_mock, out_kind, d_out, d_cross, (hipStream_t)hip_stream);
}

// Host-buffer twin: the set goes to the device once, the rows in pieces through temporary device buffers on the handle's stream.
extern "C" int cf_mock_eval(cf_handle* h, const cf_mock_set* set, const double* theta, int64_t S, const int32_t* mock,
                            int32_t out_kind, double* out, double* cross) {
  int rc = mock_check(h, set, theta, S, mock, out_kind, out);
  if (rc) return rc;
  if (S == 0) return CF_OK;
  HandleScope hs(h);
  HIP_TRY(hs.err);
  const int64_t K = set->n_mocks;
  DevBuf gs, gb, gc, cc;
  cf_mock_set dset = *set;
  if (set->n_sn) {
    if (gs.ensure((size_t)K * set->n_sn * 8)) return CF_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(gs.p, set->g_sn, (size_t)K * set->n_sn * 8, hipMemcpyHostToDevice, h->stream));
    dset.g_sn = gs.as<const double>();
  }
  if (set->n_bao) {
    if (gb.ensure((size_t)K * set->n_bao * 8)) return CF_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(gb.p, set->g_bao, (size_t)K * set->n_bao * 8, hipMemcpyHostToDevice, h->stream));
    dset.g_bao = gb.as<const double>();
  }
  if (set->n_cmb) {
    if (gc.ensure((size_t)K * 3 * 8)) return CF_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(gc.p, set->g_cmb, (size_t)K * 3 * 8, hipMemcpyHostToDevice, h->stream));
    dset.g_cmb = gc.as<const double>();
  }
  if (cc.ensure((size_t)K * 8)) return CF_ERR_HIP;
  HIP_TRY(hipMemcpyAsync(cc.p, set->c, (size_t)K * 8, hipMemcpyHostToDevice, h->stream));
  dset.c = cc.as<const double>();
  RowStage rows(h->stream, std::min<int64_t>(S, CF_RESID_HOST_PIECE));
  const double* dth = rows.in(theta, (size_t)h->d.ndim * 8);
  const int32_t* dmk = rows.in(mock, 4);
  double* dout = rows.out(out, 8);
  double* dcr = rows.out(cross, 3 * 8);
  return rows.run(S, [&](int64_t, int64_t m) { return mock_run(hs, dset, dth, m, dmk, out_kind, dout, dcr, h->stream); });
}
