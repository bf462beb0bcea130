// cosmofit_quasar.hip — the quasar Hubble-diagram likelihoods (quasars/qsr_*.py; include/cosmofit.h: cf_create_quasar).
//
// The quasar scripts use an older distance algorithm than the rest of the engine: the cumulative trapezoid of 1 / E on a
// linspace grid to max(z_qsr) (and, for one script, a second grid to max(z_sn)), LINEAR interpolation (np.interp) at the data,
// a free intrinsic scatter s of the quasar block with its sum ln(sigma^2 + s^2), and in the BAO scripts a separate trapezoid
// on linspace(0, z_i, G) per BAO datum.
//
// One workgroup of 256 threads per walker (qsr_walker_kernel):
//   1. each grid's cumulative table goes to LDS (G doubles: 24 KB at G = 3000, 48 KB for two grids): thread t owns a
//      contiguous chunk of nodes, sums its intervals in order (one interval per node: width x (y_prev + y) / 2, as scipy's
//      cumulative_trapezoid), the chunk totals are scanned with the wave64 DPP scan of the distance-table build
//      (cf_wave.h) and the four wave totals in order;
//   2. the SN residuals obs - offset - mu(z) go to Delta[w][n_ld] in the layout the solve kernels read (tri_gemm_* /
//      trsm_chi2_kernel then compute Delta^T C^-1 Delta unchanged);
//   3. chi2_q and sum ln(sigma^2 + s^2) over the quasars, each a per-thread sum in index order then the fixed-order block sum;
//   4. BAO: each DISTINCT redshift once, the threads strided across its G nodes (trapezoid weights), the same fixed-order
//      block sum;
//      thread 0 forms the predictions and Delta^T inv_cov Delta.
// Every sum runs in an order that depends only on the walker's own row, never on W: a walker's bits do not depend on the batch.
// Per node and walker the table costs one exp, one multiply-add and one rsqrt: (1 + z)^3 and ln(n X / (1 + (n - 1) X)) are
// tabulated at create time.
// The quasar and BAO chi^2 reach the output through chi2_extra, as the small-blocks kernel's do: the solve kernels (SN block)
// or finalize_kernel (no SN block) add it and apply the prior / output epilogue.  For CF_OUT_LOGL / CF_OUT_LOGP the kernel adds
// sum ln(sigma^2 + s^2) to chi2_extra as well, so that the shared epilogue's -0.5 chi^2 is the script's log-likelihood.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/cosmofit.h"
#include "cf_handle.h"
#include "cf_wave.h"
#include "cosmofit_device.h"

#define QSR_TPB 256
#define QSR_WAVES (QSR_TPB / 64)
#define QSR_MAX_DEVICES 64  // device ordinals whose dynamic-LDS allowance is remembered (cf_qsr_launch)

__device__ __forceinline__ double qsr_slot(const cf_dev_slot& s, const double* th) { return s.idx >= 0 ? th[s.idx] * s.scale : s.fixed; }

// 1 / E at a tabulated node: E^2 = Om (1 + z)^3 + (1 - Om) exp(p (1 + w0) ln(n X / (1 + (n - 1) X)))
__device__ __forceinline__ double qsr_inv_e(double om, double ea, double zp3, double lnf) {
  return rsqrt(om * zp3 + (1.0 - om) * exp(ea * lnf));
}

// Sum over the workgroup in a fixed order: the wave's DPP scan, then the four wave totals left to right.  All threads call it.
__device__ __forceinline__ double qsr_block_sum(double v, double* red) {
  const double incl = wave_inclusive_scan(v);
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = incl;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int k = 1; k < QSR_WAVES; ++k) s += red[k];
  __syncthreads();
  return s;
}

// np.interp on the table through a create-time record (node j, z - z_j, z_{j+1} - z_j); t == 0 is node j exactly
__device__ __forceinline__ double qsr_interp(const double* tab, int j, double t, double h) {
  const double c0 = tab[j];
  return t == 0.0 ? c0 : (tab[j + 1] - c0) / h * t + c0;
}

// The cumulative trapezoid of 1 / E on table `tb` into lds[0, G).
__device__ __forceinline__ void qsr_build_table(const cf_qsr_args& a, int tb, double om, double ea, double* lds, double* red) {
  const int G = a.n_grid, CH = (G + QSR_TPB - 1) / QSR_TPB;
  const int g0 = (int)threadIdx.x * CH, g1 = min(g0 + CH, G);
  const double* wd = a.node_w + (size_t)tb * G;
  const double* zp3 = a.node_zp3 + (size_t)tb * G;
  const double* lnf = a.node_lnf + (size_t)tb * G;
  double yprev = (g0 > 0 && g0 < G) ? qsr_inv_e(om, ea, zp3[g0 - 1], lnf[g0 - 1]) : 0.0;
  double run = 0.0;
  for (int g = g0; g < g1; ++g) {
    const double y = qsr_inv_e(om, ea, zp3[g], lnf[g]);
    if (g > 0) run += wd[g] * (yprev + y) * 0.5;
    lds[g] = run;
    yprev = y;
  }
  // exclusive prefix of the chunk totals: the lane before in the wave (DPP wave_shr:1), plus the waves before, in order
  const double incl = wave_inclusive_scan(run);
  const double excl = dpp_move<0x138, 0xF>(incl);
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = incl;
  __syncthreads();
  double base = 0.0;
  for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) base += red[k];
  base += excl;
  for (int g = g0; g < g1; ++g) lds[g] += base;
  __syncthreads();
}

extern "C" __global__ void __launch_bounds__(QSR_TPB)
qsr_walker_kernel(cf_qsr_args a, const double* __restrict__ theta, int64_t W, double* __restrict__ delta, double* __restrict__ extra,
                  int with_ln, double* __restrict__ th_copy, double* __restrict__ parts, double* __restrict__ mu_sn_out,
                  double* __restrict__ mu_q_out, double* __restrict__ bao_out) {
  extern __shared__ double lds[];  // [1 + two_grids][G]
  __shared__ double red[QSR_WAVES];
  __shared__ double th[CF_MAX_NDIM];
  __shared__ double bz_dm[CF_MAX_BAO], bz_e[CF_MAX_BAO];
  const int64_t w = blockIdx.x;
  if (w >= W) return;
  const int tid = threadIdx.x, G = a.n_grid;
  if (tid < a.ndim) {
    const double v = theta[w * a.ndim + tid];
    th[tid] = v;
    if (th_copy) th_copy[w * a.ndim + tid] = v;  // later kernels of the evaluation read the row from device memory
  }
  __syncthreads();
  const double om = qsr_slot(a.om, th), ea = a.fde_a * (1.0 + qsr_slot(a.w0, th));
  const double c_h0 = a.c / qsr_slot(a.h0, th);
  const int ng = 1 + a.two_grids;
  for (int tb = 0; tb < ng; ++tb) qsr_build_table(a, tb, om, ea, lds + (size_t)tb * G, red);

  // SN residuals in the solve kernels' layout
  if (a.n_sn > 0) {
    const double* tab = lds + (size_t)(a.two_grids ? G : 0);
    const double off = qsr_slot(a.off_sn, th);
    double* dl = delta + w * (int64_t)a.n_ld;
    for (int i = tid; i < a.n_sn; i += QSR_TPB) {
      const double mu = 25.0 + 5.0 * log10(a.sn_zp1[i] * c_h0 * qsr_interp(tab, a.sn_j[i], a.sn_t[i], a.sn_h[i]));
      dl[i] = (a.sn_obs[i] - off) - mu;
      if (mu_sn_out) mu_sn_out[w * a.n_sn + i] = mu;
    }
  }
  // quasars
  const double dmq = qsr_slot(a.off_q, th), s = qsr_slot(a.scat, th), s2 = s * s;
  double chi = 0.0, lnv = 0.0;
  for (int i = tid; i < a.n_qsr; i += QSR_TPB) {
    const double mu = 25.0 + 5.0 * log10(a.q_zp1[i] * c_h0 * qsr_interp(lds, a.q_j[i], a.q_t[i], a.q_h[i]));
    const double d = (a.q_mu[i] - dmq) - mu, var = a.q_var[i] + s2;
    const double term = d * d / var;
    chi += term == term ? term : 0.0;  // the scripts' pandas sum skips NaN terms (E^2 < 0 past some z: outside the box only)
    lnv += log(var);
    if (mu_q_out) mu_q_out[w * a.n_qsr + i] = mu;
  }
  chi = qsr_block_sum(chi, red);
  lnv = qsr_block_sum(lnv, red);

  // BAO: one quadrature per distinct redshift, weights x 1 / E summed per thread over nodes tid, tid + 256, .. (coalesced
  // table loads), then the block sum
  double chi_bao = 0.0;
  if (a.n_bao > 0) {
    for (int b = 0; b < a.n_bz; ++b) {
      const size_t tb = (size_t)(ng + b) * G;
      double acc = 0.0;
      for (int g = tid; g < G; g += QSR_TPB) acc += a.node_w[tb + g] * qsr_inv_e(om, ea, a.node_zp3[tb + g], a.node_lnf[tb + g]);
      acc = qsr_block_sum(acc, red);
      if (tid == 0) {
        bz_dm[b] = c_h0 * acc;  // D_M: the last value of its own trapezoid of c / H
        bz_e[b] = sqrt(om * a.node_zp3[tb + G - 1] + (1.0 - om) * exp(ea * a.node_lnf[tb + G - 1]));  // E(z_i): the top node is z_i
      }
    }
    if (tid == 0) {
      const double rd = qsr_slot(a.rd, th), h0 = qsr_slot(a.h0, th);
      double dv[CF_MAX_BAO];
      for (int k = 0; k < a.n_bao; ++k) {
        const int b = a.bao_zi[k];
        const double dh = a.c / (h0 * bz_e[b]), dm = bz_dm[b];
        const int q = a.bao_qty[k];
        const double pred = (q == CF_BAO_DM ? dm : (q == CF_BAO_DH ? dh : pow(a.bao_z[k] * dh * (dm * dm), 1.0 / 3.0))) / rd;
        dv[k] = a.bao_val[k] - pred;
        if (bao_out) bao_out[w * a.n_bao + k] = pred;
      }
      for (int i = 0; i < a.n_bao; ++i) {
        double r = 0.0;
        for (int j = 0; j < a.n_bao; ++j) r += a.bao_inv[i * a.n_bao + j] * dv[j];
        chi_bao += dv[i] * r;
      }
    }
  }
  if (tid == 0) {
    extra[w] = chi + chi_bao + (with_ln ? lnv : 0.0);
    if (parts) {
      parts[3 * w + 1] = chi;
      parts[3 * w + 2] = chi_bao;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Host side: create-time tables and the launch.
// ------------------------------------------------------------------------------------------------
struct cf_qsr_state {
  cf_qsr_args args{};
  std::vector<void*> bufs;
  int64_t n_qsr = 0;
  int32_t n_bao = 0;
  // accessor outputs (device), set around one launch under the handle's lock by cf_qsr_eval_parts (below)
  double* parts = nullptr;
  double* mu_sn = nullptr;
  double* mu_q = nullptr;
  double* bao = nullptr;
};

void cf_qsr_free(cf_qsr_state* q) {
  if (!q) return;
  for (void* p : q->bufs) (void)hipFree(p);
  delete q;
}

template <class T>
static int qsr_upload(cf_qsr_state* q, const std::vector<T>& v, const T** dst) {
  void* p = nullptr;
  const size_t n = std::max<size_t>(v.size(), 1) * sizeof(T);
  if (hipMalloc(&p, n) != hipSuccess) return cf_set_error(CF_ERR_HIP, "cf_create_quasar: hipMalloc failed");
  q->bufs.push_back(p);
  if (!v.empty() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    return cf_set_error(CF_ERR_HIP, "cf_create_quasar: hipMemcpy failed");
  *dst = (const T*)p;
  return 0;
}

// np.linspace(0, top, G): j * step, the last node forced to top
static std::vector<double> qsr_linspace(double top, int G) {
  std::vector<double> x((size_t)G);
  const double step = top / (double)(G - 1);
  for (int j = 0; j < G; ++j) x[(size_t)j] = (double)j * step;
  x[(size_t)G - 1] = top;
  return x;
}

// np.interp record of z on nodes x: (j, z - x_j, x_{j+1} - x_j); t = 0 when z is node j, at / above the top or below 0
static void qsr_record(const std::vector<double>& x, double z, int32_t& j, double& t, double& h) {
  const int G = (int)x.size();
  j = 0, t = 0.0, h = 1.0;
  if (!(z < x[(size_t)G - 1])) { j = G - 1; return; }
  if (!(z > x[0])) return;
  const int k = (int)(std::upper_bound(x.begin(), x.end(), z) - x.begin()) - 1;  // x[k] <= z < x[k + 1]
  j = k;
  t = z - x[(size_t)k];
  if (t != 0.0) h = x[(size_t)k + 1] - x[(size_t)k];
}

// Per-node tables of one grid: widths (trapezoid weights when `weights`), (1 + z)^3, ln(n X / (1 + (n - 1) X)).
static void qsr_node_tables(const std::vector<double>& x, const cf_qsr_ext* e, bool weights, std::vector<double>& wd,
                            std::vector<double>& zp3, std::vector<double>& lnf) {
  const size_t G = x.size();
  std::vector<double> dx(G + 1, 0.0);
  for (size_t j = 1; j < G; ++j) dx[j] = x[j] - x[j - 1];  // np.diff
  for (size_t j = 0; j < G; ++j) {
    const double zp1 = 1.0 + x[j];
    const long double X = powl((long double)zp1, (long double)e->fde_k);
    wd.push_back(weights ? 0.5 * (dx[j] + dx[j + 1]) : dx[j]);
    zp3.push_back((double)((long double)zp1 * zp1 * zp1));
    lnf.push_back((double)logl((long double)e->fde_n * X / (1.0L + ((long double)e->fde_n - 1.0L) * X)));
  }
}

static cf_dev_slot qsr_dev_slot(const cf_param& p) {
  cf_dev_slot s;
  s.idx = p.idx;
  s.pad = 0;
  s.scale = p.scale;
  s.fixed = p.fixed;
  return s;
}

// Validate the extension against the descriptor and upload every table on the current device.
static int cf_qsr_prepare(const cf_desc* c, const cf_qsr_ext* e, int64_t n_ld, cf_qsr_state** out) {
  *out = nullptr;
  auto bad = [](const char* m) { return cf_set_error(CF_ERR_INVALID, std::string("cf_create_quasar: ") + m); };
  if (e->struct_size != (int32_t)sizeof(cf_qsr_ext)) return bad("extension size mismatch");
  if (e->n_grid < 16 || e->n_grid > 8192) return bad("n_grid must be in 16..8192");
  if (e->n_qsr < 1 || e->n_qsr > CF_QSR_MAX_QSR) return bad("n_qsr must be in 1..65536");
  if (!e->qsr_z || !e->qsr_mu || !e->qsr_sigma) return bad("quasar arrays must not be null");
  if (e->qsr_offset.idx >= c->ndim || e->qsr_scatter.idx >= c->ndim) return bad("quasar slot index >= ndim");
  if (!std::isfinite(e->fde_n) || !std::isfinite(e->fde_k) || !std::isfinite(e->fde_p)) return bad("(n, k, p) must be finite");
  if (!(e->qsr_z_top > 0.0) || !std::isfinite(e->qsr_z_top)) return bad("qsr_z_top must be > 0");
  if (!(e->sn_z_top >= 0.0) || !std::isfinite(e->sn_z_top)) return bad("sn_z_top must be >= 0 (0: the quasar grid)");
  if ((e->sn_zhel | 1) != 1) return bad("sn_zhel must be 0 or 1");
  for (int64_t i = 0; i < e->n_qsr; ++i)
    if (!(e->qsr_z[i] >= 0.0)) return bad("quasar redshifts must be >= 0");
  if (c->n_bao != 0 || c->cmb_mode != CF_CMB_NONE || c->n_cc != 0 || c->n_fs8 != 0 || c->ez_model != CF_EZ_LATE_FLAT)
    return bad("the descriptor must carry no BAO / CMB / chronometer / growth block and use CF_EZ_LATE_FLAT");
  if (c->n_sn > 0 && (c->sn_fixed_mu || c->sn_lin_coef || c->sn_dir)) return bad("the SN block takes no fixed mu / linear term / directions");
  if (e->bao_mode == CF_QSR_BAO_NONE) {
    if (e->n_bao != 0) return bad("n_bao must be 0 without a BAO mode");
  } else if (e->bao_mode == CF_QSR_BAO_QUAD) {
    if (e->n_bao < 1 || e->n_bao > CF_MAX_BAO) return bad("n_bao must be in 1..64");
    if (!e->bao_z || !e->bao_val || !e->bao_qty || !e->bao_inv_cov) return bad("BAO arrays must not be null");
    for (int k = 0; k < e->n_bao; ++k) {
      if (e->bao_qty[k] < CF_BAO_DV || e->bao_qty[k] > CF_BAO_DH) return bad("bao_qty must be D_V, D_M or D_H");
      if (!(e->bao_z[k] > 0.0) || !std::isfinite(e->bao_z[k])) return bad("BAO redshifts must be > 0");
    }
    if (c->param[CF_P_RD].idx < 0 && !(c->param[CF_P_RD].fixed > 0.0)) return bad("the BAO block needs r_d (slot CF_P_RD)");
  } else {
    return bad("bad bao_mode");
  }
  const int G = e->n_grid;
  const bool two = c->n_sn > 0 && e->sn_z_top > 0.0;
  cf_qsr_state* q = new cf_qsr_state();
  auto bail = [&](int rc) { cf_qsr_free(q); return rc; };
  cf_qsr_args& a = q->args;
  a.ndim = c->ndim;
  a.n_grid = G;
  a.n_sn = (int32_t)c->n_sn;
  a.n_ld = (int32_t)n_ld;
  a.n_qsr = (int32_t)e->n_qsr;
  a.two_grids = two ? 1 : 0;
  a.n_bao = e->n_bao;
  a.c = c->c_km_s;
  a.fde_a = e->fde_p;
  a.om = qsr_dev_slot(c->param[CF_P_OM]);
  a.w0 = qsr_dev_slot(c->param[CF_P_W0]);
  a.h0 = qsr_dev_slot(c->param[CF_P_H0]);
  a.off_sn = qsr_dev_slot(c->param[CF_P_OFFSET]);
  a.rd = qsr_dev_slot(c->param[CF_P_RD]);
  a.off_q = qsr_dev_slot(e->qsr_offset);
  a.scat = qsr_dev_slot(e->qsr_scatter);

  // grids: quasars, the SN grid of its own, then the distinct BAO redshifts in first-seen order
  std::vector<std::vector<double>> grids{qsr_linspace(e->qsr_z_top, G)};
  if (two) grids.push_back(qsr_linspace(e->sn_z_top, G));
  std::vector<double> bz;
  std::vector<int32_t> bzi;
  for (int k = 0; k < e->n_bao; ++k) {
    int b = (int)(std::find(bz.begin(), bz.end(), e->bao_z[k]) - bz.begin());
    if (b == (int)bz.size()) bz.push_back(e->bao_z[k]);
    bzi.push_back(b);
  }
  a.n_bz = (int32_t)bz.size();
  std::vector<double> wd, zp3, lnf;
  for (auto& x : grids) qsr_node_tables(x, e, false, wd, zp3, lnf);
  for (double z : bz) qsr_node_tables(qsr_linspace(z, G), e, true, wd, zp3, lnf);
  int rc;
  if ((rc = qsr_upload(q, wd, &a.node_w)) || (rc = qsr_upload(q, zp3, &a.node_zp3)) || (rc = qsr_upload(q, lnf, &a.node_lnf))) return bail(rc);

  std::vector<int32_t> jj;
  std::vector<double> tt, hh, zp, v1, v2;
  if (c->n_sn > 0) {
    const std::vector<double>& x = grids[two ? 1 : 0];
    for (int64_t i = 0; i < c->n_sn; ++i) {
      int32_t j;
      double t, h;
      qsr_record(x, c->sn_z_cmb[i], j, t, h);
      jj.push_back(j), tt.push_back(t), hh.push_back(h);
      zp.push_back(1.0 + (e->sn_zhel ? c->sn_z_hel[i] : c->sn_z_cmb[i]));
      v1.push_back(c->sn_obs[i]);
    }
    if ((rc = qsr_upload(q, jj, &a.sn_j)) || (rc = qsr_upload(q, tt, &a.sn_t)) || (rc = qsr_upload(q, hh, &a.sn_h)) ||
        (rc = qsr_upload(q, zp, &a.sn_zp1)) || (rc = qsr_upload(q, v1, &a.sn_obs)))
      return bail(rc);
  }
  jj.clear(), tt.clear(), hh.clear(), zp.clear(), v1.clear();
  for (int64_t i = 0; i < e->n_qsr; ++i) {
    int32_t j;
    double t, h;
    qsr_record(grids[0], e->qsr_z[i], j, t, h);
    jj.push_back(j), tt.push_back(t), hh.push_back(h);
    zp.push_back(1.0 + e->qsr_z[i]);
    v1.push_back(e->qsr_mu[i]);
    v2.push_back(e->qsr_sigma[i] * e->qsr_sigma[i]);
  }
  if ((rc = qsr_upload(q, jj, &a.q_j)) || (rc = qsr_upload(q, tt, &a.q_t)) || (rc = qsr_upload(q, hh, &a.q_h)) ||
      (rc = qsr_upload(q, zp, &a.q_zp1)) || (rc = qsr_upload(q, v1, &a.q_mu)) || (rc = qsr_upload(q, v2, &a.q_var)))
    return bail(rc);
  if (e->n_bao > 0) {
    const std::vector<double> z(e->bao_z, e->bao_z + e->n_bao), val(e->bao_val, e->bao_val + e->n_bao),
        inv(e->bao_inv_cov, e->bao_inv_cov + (size_t)e->n_bao * e->n_bao);
    const std::vector<int32_t> qty(e->bao_qty, e->bao_qty + e->n_bao);
    if ((rc = qsr_upload(q, z, &a.bao_z)) || (rc = qsr_upload(q, val, &a.bao_val)) || (rc = qsr_upload(q, inv, &a.bao_inv)) ||
        (rc = qsr_upload(q, qty, &a.bao_qty)) || (rc = qsr_upload(q, bzi, &a.bao_zi)))
      return bail(rc);
  }
  q->n_qsr = e->n_qsr;
  q->n_bao = e->n_bao;
  *out = q;
  return 0;
}

// The per-walker kernel of one evaluation on `st`: SN residuals into delta, chi2_q (+ sum ln) + chi2_bao into extra.
int cf_qsr_launch(const cf_qsr_state* q, const double* theta, int64_t W, double* delta, double* extra, int out_kind,
                  double* th_copy, hipStream_t st) {
  const size_t lds = (size_t)(1 + q->args.two_grids) * q->args.n_grid * sizeof(double);
  // 8192 nodes are 64 KiB of dynamic LDS, 128 KiB with an SN grid of its own, next to about 1.2 KB of static LDS: at or past
  // the 64 KiB a launch may take by default.  The first launch on a device whose table could come near that default (half of
  // it: the scripts' 3000 nodes stay below and never pay for the call) raises the kernel's allowance, once, to the largest
  // table cf_create_quasar accepts.  Per device: a handle may have replicas on several.  Two threads that race here both
  // set the same value.
  static std::atomic<bool> raised[QSR_MAX_DEVICES];
  constexpr int max_lds = 2 * 8192 * (int)sizeof(double);
  if (lds > 32 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return cf_set_error(CF_ERR_HIP, "cf_qsr_launch: hipGetDevice failed");
    if (dev >= QSR_MAX_DEVICES || !raised[dev].load(std::memory_order_acquire)) {
      if (hipFuncSetAttribute((const void*)&qsr_walker_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess)
        return cf_set_error(CF_ERR_HIP, "cf_qsr_launch: " + std::to_string(max_lds) + " bytes of dynamic LDS refused on device " +
                                            std::to_string(dev));
      if (dev < QSR_MAX_DEVICES) raised[dev].store(true, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(qsr_walker_kernel, dim3((unsigned)W), dim3(QSR_TPB), lds, st, q->args, theta, W, delta, extra,
                     out_kind != CF_OUT_CHI2 ? 1 : 0, th_copy, q->parts, q->mu_sn, q->mu_q, q->bao);
  // a refused launch is this call's error: the kernels behind it would otherwise finish the evaluation on stale residuals
  return cf_launch_status("cf_qsr_launch: qsr_walker_kernel (or an earlier HIP call of this thread)");
}

// ------------------------------------------------------------------------------------------------
// Entry points.  A quasar handle is an ordinary handle (cf_handle.h) whose per-walker kernel is the one above; the SN solve, the
// epilogue, the workspace, timing and the completion words are the handle's own.
// ------------------------------------------------------------------------------------------------
extern "C" int cf_create_quasar(const cf_desc* c, const cf_qsr_ext* e, cf_handle** out) {
  if (!c || !e || !out) return cf_set_error(CF_ERR_INVALID, "cf_create_quasar: null argument");
  *out = nullptr;
  if (c->n_devices != 0) return cf_set_error(CF_ERR_UNSUPPORTED, "cf_create_quasar: a quasar handle lives on one device (n_devices must be 0)");
  int rc = validate_desc(c);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return cf_set_error(CF_ERR_NO_DEVICE, "cf_create_quasar: no HIP device visible (this library has no CPU path)");
  if (c->device < 0 || c->device >= ndev) return cf_set_error(CF_ERR_INVALID, "cf_create_quasar: device ordinal out of range");
  HostPrep prep;
  cf_handle* h = nullptr;
  if ((rc = create_one(c, c->device, prep, &h))) return rc;
  {
    DeviceScope on_device(h->device);
    if (on_device.err != hipSuccess) rc = cf_set_error(CF_ERR_HIP, "hipSetDevice failed");
    else rc = cf_qsr_prepare(c, e, h->d.n_ld, &h->qsr);
  }
  if (rc) {
    const std::string keep = cf_last_error();
    cf_destroy(h);
    return cf_set_error(rc, keep);
  }
  *out = h;
  return CF_OK;
}

extern "C" int cf_qsr_eval_parts(cf_handle* h, const double* theta, int64_t W, double* chi2_blocks, double* mu_sn, double* mu_qsr,
                                 double* bao_theory) {
  if (!h || !theta) return cf_set_error(CF_ERR_INVALID, "cf_qsr_eval_parts: null argument");
  if (!h->qsr) return cf_set_error(CF_ERR_INVALID, "cf_qsr_eval_parts: not a quasar handle (cf_create_quasar)");
  if (W <= 0 || W > (1 << 20)) return cf_set_error(CF_ERR_INVALID, "cf_qsr_eval_parts: W out of range");
  if (mu_sn && h->d.n_sn == 0) return cf_set_error(CF_ERR_INVALID, "cf_qsr_eval_parts: this likelihood has no SN block");
  cf_qsr_state* const q = h->qsr;
  const int64_t nq = q->n_qsr, nb = q->n_bao, n = h->d.n_sn;
  if (bao_theory && nb == 0) return cf_set_error(CF_ERR_INVALID, "cf_qsr_eval_parts: this likelihood has no BAO block");
  HandleScope hs(h);
  HIP_TRY(hs.err);
  int rc;
  if ((rc = ensure_workspace(h, W))) return rc;
  DevBuf parts, snb, ms, mq, bt;
  if (parts.ensure((size_t)W * 3 * 8) || snb.ensure((size_t)W * 8)) return CF_ERR_HIP;
  HIP_TRY(hipMemsetAsync(parts.p, 0, (size_t)W * 3 * 8, h->stream));
  HIP_TRY(hipMemsetAsync(snb.p, 0, (size_t)W * 8, h->stream));
  if (mu_sn && ms.ensure((size_t)W * n * 8)) return CF_ERR_HIP;
  if (mu_qsr && mq.ensure((size_t)W * nq * 8)) return CF_ERR_HIP;
  if (bao_theory && bt.ensure((size_t)W * nb * 8)) return CF_ERR_HIP;
  HIP_TRY(hipMemcpyAsync(h->theta.p, theta, (size_t)W * h->d.ndim * 8, hipMemcpyHostToDevice, h->stream));
  q->parts = parts.as<double>(), q->mu_sn = ms.as<double>(), q->mu_q = mq.as<double>(), q->bao = bt.as<double>();
  rc = launch_path(h, h->theta.as<const double>(), W, h->out.as<double>(), CF_OUT_CHI2, h->stream, nullptr, nullptr, nullptr, nullptr,
                   n > 0 ? snb.as<double>() : nullptr);
  q->parts = q->mu_sn = q->mu_q = q->bao = nullptr;
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (mu_sn) HIP_TRY(hipMemcpy(mu_sn, ms.p, (size_t)W * n * 8, hipMemcpyDeviceToHost));
  if (mu_qsr) HIP_TRY(hipMemcpy(mu_qsr, mq.p, (size_t)W * nq * 8, hipMemcpyDeviceToHost));
  if (bao_theory) HIP_TRY(hipMemcpy(bao_theory, bt.p, (size_t)W * nb * 8, hipMemcpyDeviceToHost));
  if (chi2_blocks) {
    std::vector<double> sn((size_t)W);
    HIP_TRY(hipMemcpy(chi2_blocks, parts.p, (size_t)W * 3 * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sn.data(), snb.p, (size_t)W * 8, hipMemcpyDeviceToHost));
    for (int64_t w = 0; w < W; ++w) chi2_blocks[3 * w] = sn[(size_t)w];
  }
  return CF_OK;
}
