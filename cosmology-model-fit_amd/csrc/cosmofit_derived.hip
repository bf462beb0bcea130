// cosmofit_derived.hip — derived parameters and prediction curves of posterior samples (include/cosmofit.h: cf_derived_device,
// cf_curves_device; the driver is cosmology-model-fit_amd/derived.py).
//
// What the post-fit blocks of the scripts do first with their samples: Omega_m, omega_m, z*, r_d, S8, q0, j0, z_drag, z_eq
// (bao/desi_cmb.py:196-199, bao/desi_cmb_union3_fs8.py:282-287, cmb/cmb.py:118-138), the blobs of cmb/cmb.py:45-63, and the
// H(z) / D_M(z) / BAO / mu(z) curves of the prediction plots (bao/plot_predictions.py:23) -- here for every row of a
// device-resident chain, so that 1e5-1e7 samples never leave the GPU between the sampler and the corner plot.
//
// derived_kernel: ONE THREAD PER ROW.  The closed forms are a handful of operations per row and the kernel is then bound by
// the rows it reads and the columns it writes; the Gauss-Legendre quantities are 2 n_gl evaluations of H per row, a loop whose
// trip count and branches are the same in every lane (wave-uniform), so a thread per row keeps all 64 lanes busy with no
// cross-lane step, and the sum runs in node order -- the reference's own order (cmb/data_planck_act_compression.py:160-197).
// Lanes-per-row (the likelihood's small_blocks_kernel: sixteen lanes, a butterfly) is the form for a few walkers that must
// fill the chip; a chain has 1e5+ rows and fills it with a thread each.
//
// curves_kernel: ONE 256-THREAD WORKGROUP PER ROW.  The row's {cum_dm, dh} table (n_grid x 16 B = 64 KB at the scripts' 4000
// nodes, LDS, two workgroups per CU) is built once -- E(z) at the nodes strided over the threads, the cumulative trapezoid as
// chunk-sequential sums plus the chunk totals added left to right -- and serves all nz redshifts: cubic Hermite for D_M (linear
// extrapolation outside the grid, interpolator.py:71-108), PCHIP or c / H for D_H as the handle's BAO block does.  FP64 VALU
// bound: ~n_grid E(z) evaluations per row.
//
// Every sum runs in an order fixed by the row alone: a row's bits depend neither on S, nor on its position, nor on the grid of
// the launch.  A non-finite theta entry reaches the columns that read it as NaN (slot reads turn +-inf into NaN); no index ever
// depends on theta, and a non-finite redshift gives NaN before any table look-up.
//
// The device helpers below restate the few expressions of cosmofit_kernels.hip these kernels share with the likelihood (slot
// read-out, E^2(z), the fitting formulae, Hermite / PCHIP on the table), as cosmofit_quasar.hip does: the likelihood's
// translation unit is not touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <cmath>
#include <string>

#include "../../include/cosmofit.h"
#include "cf_handle.h"
#include "cosmofit_device.h"

typedef double d2 __attribute__((ext_vector_type(2)));

#define DQ_TPB 256
#define DQ_MAX_DEVICES 64  // device ordinals whose dynamic-LDS allowance is remembered (cf_curves_launch)

// ------------------------------------------------------------------------------------------------
// Slots and E^2(z): make_cosmo / f_de / omnu_z / e2_of_z of cosmofit_kernels.hip, model and dark-energy form at run time
// (wave-uniform branches)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dq_slot(const cf_dev_desc& d, int s, const double* __restrict__ th) {
  const cf_dev_slot& p = d.slot[s];
  if (p.idx < 0) return p.fixed;
  const double v = th[p.idx];
  return isfinite(v) ? p.scale * v : __builtin_nan("");
}

struct DqCosmo {
  double H0, Om, w0, wa, c;
  double Or, Obc, Ode, Onu;  // CF_EZ_PHYSICAL densities (omega / h^2)
  double wb, wc;             // slots CF_P_OBH2 / CF_P_OCH2
};

__device__ __forceinline__ DqCosmo dq_cosmo(const cf_dev_desc& d, const double* __restrict__ th) {
  DqCosmo wc;
  wc.H0 = dq_slot(d, CF_P_H0_D, th);
  wc.Om = dq_slot(d, CF_P_OM_D, th);
  const double h = wc.H0 / 100, h2 = h * h;
  if (d.om_mode) wc.Om = wc.Om / h2;  // bao/desi_omh2.py:18-20
  wc.w0 = dq_slot(d, CF_P_W0_D, th);
  wc.wa = dq_slot(d, CF_P_WA_D, th);
  wc.c = d.c;
  wc.wb = dq_slot(d, CF_P_OBH2_D, th);
  wc.wc = dq_slot(d, CF_P_OCH2_D, th);
  wc.Or = wc.Obc = wc.Ode = wc.Onu = 0.0;
  if (d.ez_model == CF_EZ_PHYSICAL_D) {  // bao/desi_cmb_des5y.py:35-39
    wc.Onu = d.omnu_h2 / h2;
    wc.Or = d.or_h2 / h2;
    wc.Obc = (wc.wb + wc.wc) / h2;
    wc.Ode = 1.0 - wc.Obc - wc.Or - wc.Onu;
  }
  return wc;
}

__device__ __forceinline__ double dq_fde(const cf_dev_desc& d, const DqCosmo& wc, double z, double zp1, double cubed) {
  if (d.fde == CF_FDE_LCDM_D) return 1.0;
  if (d.fde == CF_FDE_WCDM_D) return exp(3 * (1 + wc.w0) * log(zp1));  // sn/pantheon_and_sh0es.py:26-28
  if (d.fde == CF_FDE_THAWING_D) {                                      // bao/desi.py:26-28
    const double r = 2 * cubed / ((1.0 + wc.w0) + (1.0 - wc.w0) * cubed);
    return r * r;
  }
  return exp(fma(3 * (1 + wc.w0 + wc.wa), log(zp1), -3 * wc.wa * z / zp1));  // bao/desi_fs_lya_cmb.py:19-22
}

// 5-node massive-neutrino density, cmb/data_planck_act_compression.py:53-66
__device__ __forceinline__ double dq_omnu(const cf_dev_desc& d, double zp1) {
  const double r = d.nu_m0 / zp1, mz_sq = r * r;
  const double ws = sqrt(d.nu_qs_sq[0] + mz_sq) * d.nu_ws[0] + sqrt(d.nu_qs_sq[1] + mz_sq) * d.nu_ws[1] +
                    sqrt(d.nu_qs_sq[2] + mz_sq) * d.nu_ws[2] + sqrt(d.nu_qs_sq[3] + mz_sq) * d.nu_ws[3] +
                    sqrt(d.nu_qs_sq[4] + mz_sq) * d.nu_ws[4];
  const double zp1_2 = zp1 * zp1;
  return zp1_2 * zp1_2 * ws / d.nu_rho0;
}

// `nu` < 0: evaluate the neutrino density here; otherwise the value tabulated at cf_create for this grid node
__device__ __forceinline__ double dq_e2(const cf_dev_desc& d, const DqCosmo& wc, double z, double nu = -1.0) {
  const double zp1 = 1.0 + z;
  const double cubed = zp1 * zp1 * zp1;
  const double f = dq_fde(d, wc, z, zp1, cubed);
  if (d.ez_model == CF_EZ_LATE_FLAT_D) return wc.Om * cubed + (1.0 - wc.Om) * f;  // sn/pantheon.py:28-31
  if (nu < 0.0) nu = dq_omnu(d, zp1);
  return wc.Or * (cubed * zp1) + wc.Obc * cubed + wc.Ode * f + wc.Onu * nu;  // bao/desi_cmb_des5y.py:43-48
}

__device__ __forceinline__ double dq_H(const cf_dev_desc& d, const DqCosmo& wc, double z) { return wc.H0 * sqrt(dq_e2(d, wc, z)); }

// matter density handed to the r_drag / z_drag fits: omega_b + omega_c + omega_nu, or Omega_m h^2 (bao/desi_bbn.py:46-60)
__device__ __forceinline__ double dq_wm_drag(const cf_dev_desc& d, const DqCosmo& wc) {
  const double h = wc.H0 / 100;
  return d.rd_wm_late ? wc.Om * (h * h) : wc.wb + wc.wc + d.omnu_h2;
}

// Fitting formulae of arXiv:2106.00428 with the reference's coefficients (cmb/data_planck_act_compression.py:86-138)
__device__ double dq_z_star(const double* f, double wb, double wm) {  // s1 s2 b m e0 c1 e1 e2 c2 e3 e4
  wb = pow(wb, f[2]);
  wm = pow(wm, f[3]);
  return pow(wm, f[4]) + f[0] * f[5] * pow(wb, f[6]) * pow(wm, f[7]) + f[1] * f[8] * pow(wm, f[9]) * pow(wb, f[10]);
}
__device__ double dq_r_drag(const double* f, double wb, double wm) {  // b m a1..a9
  wb = pow(wb, f[0]);
  wm = pow(wm, f[1]);
  const double den = (f[2] * pow(wb, f[3])) + (f[4] * pow(wb, f[5]) * pow(wm, f[6])) + (f[7] * pow(wm, f[8]));
  return 1.0 / den - f[9] / pow(wm, f[10]);
}
__device__ double dq_z_drag(const double* f, double wb, double wm) {  // s1 s2 b m c1 e1 e2 c2 e3 e4
  wb = pow(wb, f[2]);
  wm = pow(wm, f[3]);
  return (1 + f[0] * f[4] * pow(wb, f[5]) * pow(wm, f[6]) + f[1] * f[7] * pow(wm, f[8])) * pow(wm, f[9]);
}

// ------------------------------------------------------------------------------------------------
// Scalar quantities: one thread per row
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DQ_TPB)
derived_kernel(cf_dev_desc d, cf_derived_kargs a, const double* __restrict__ theta, int64_t S, double* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * DQ_TPB + threadIdx.x;
  if (row >= S) return;
  const double* th = theta + row * d.ndim;
  const DqCosmo wc = dq_cosmo(d, th);
  const double h = wc.H0 / 100;
  const bool physical = d.ez_model == CF_EZ_PHYSICAL_D;
  const double wm_phys = wc.wb + wc.wc + d.omnu_h2;                      // bao/desi_cmb.py:196
  const double omh2 = physical ? wm_phys : (d.om_mode ? dq_slot(d, CF_P_OM_D, th) : wc.Om * (h * h));  // bao/desi_union3_bbn.py:175
  const double Om = physical ? wm_phys / (h * h) : wc.Om;                // bao/desi_cmb.py:197
  const double wa = d.fde == CF_FDE_THAWING_D ? -1.5 * (1.0 - wc.w0 * wc.w0) : wc.wa;  // bao/desi_union3_bbn.py:320
  double z_star = 0.0, r_fit = 0.0, z_drag = 0.0, rs_star = 0.0, dm_star = 0.0;
  if (a.need & CF_DQ_NEED_ZSTAR) z_star = dq_z_star(d.zstar_fit, wc.wb, wc.wc + wc.wb + d.omnu_h2);
  if (a.need & CF_DQ_NEED_RDFIT) r_fit = dq_r_drag(a.rdrag_fit, wc.wb, dq_wm_drag(d, wc));
  if (a.need & CF_DQ_NEED_ZDRAG) z_drag = dq_z_drag(a.zdrag_fit, wc.wb, dq_wm_drag(d, wc));
  if (a.need & CF_DQ_NEED_GL) {  // cmb/data_planck_act_compression.py:160-197, node order
    const double half_a = (1.0 / (1.0 + z_star)) / 2.0, half_z = z_star / 2.0;
    double i_rs = 0.0, i_dm = 0.0;
    for (int k = 0; k < d.n_gl; ++k) {
      const double x = d.gl_x[k], w = d.gl_w[k];
      const double ae = half_a * x + half_a;
      const double ze = (1.0 / ae) - 1.0;
      const double Rb = (3.0 / 4.0) * (wc.wb / d.o_gamma_h2) * ae;
      i_rs += w * (d.c / (ae * ae * dq_H(d, wc, ze) * sqrt(3.0 * (1.0 + Rb))));
      i_dm += w * (d.c / dq_H(d, wc, half_z * x + half_z));
    }
    rs_star = half_a * i_rs;
    dm_star = half_z * i_dm;
  }
  double* o = out + row * a.n_q;
  for (int q = 0; q < a.n_q; ++q) {
    double v;
    switch (a.codes[q]) {
      case CF_DQ_H0: v = wc.H0; break;
      case CF_DQ_H: v = h; break;
      case CF_DQ_OM: v = Om; break;
      case CF_DQ_OMH2: v = omh2; break;
      case CF_DQ_OBH2: v = wc.wb; break;
      case CF_DQ_OCH2: v = wc.wc; break;
      case CF_DQ_W0: v = wc.w0; break;
      case CF_DQ_WA: v = wa; break;
      case CF_DQ_Q0: v = Om / 2 + (1.0 + 3 * wc.w0) * (1.0 - Om) / 2; break;                          // bao/desi_cmb_union3_fs8.py:240
      case CF_DQ_J0: v = 1.0 + (3.0 / 2) * (1.0 - Om) * (3 * wc.w0 * (1.0 + wc.w0) + wa); break;      // :245
      case CF_DQ_S8: v = dq_slot(d, CF_P_S8_D, th) * sqrt(Om / 0.3); break;                           // :284
      case CF_DQ_RD: v = d.rd_from_fit ? r_fit : dq_slot(d, CF_P_RD_D, th); break;
      case CF_DQ_Z_STAR: v = z_star; break;
      case CF_DQ_R_DRAG: v = r_fit; break;
      case CF_DQ_Z_DRAG: v = z_drag; break;
      case CF_DQ_Z_EQ: v = -1 + (wc.wb + wc.wc) / a.args[q]; break;                                   // cmb/cmb.py:135
      case CF_DQ_H_AT: v = isfinite(a.args[q]) ? dq_H(d, wc, a.args[q]) : __builtin_nan(""); break;
      case CF_DQ_RS_STAR: v = rs_star; break;
      case CF_DQ_DM_STAR: v = dm_star; break;
      case CF_DQ_THETA_STAR100: v = 100 * (rs_star / dm_star); break;                                 // cmb/cmb.py:56,63
      case CF_DQ_R: v = 100 * sqrt(wc.wc + wc.wb + d.omnu_h2) * dm_star / d.c; break;                 // cmb/data_planck_act_compression.py:210
      case CF_DQ_LA: v = 3.14159265358979323846 * dm_star / rs_star; break;                           // :211
      default: v = __builtin_nan(""); break;
    }
    o[q] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// Curves: one workgroup per row, the row's distance table in LDS
// ------------------------------------------------------------------------------------------------
// element g = {cum_dm[g], dh[g]} at the skewed position g + (g >> chs): thread t owns the 2^chs nodes from t << chs in the
// prefix pass, so the lanes of a wave are an odd number of 16-byte slots apart
struct DqTable {
  const d2* tab;
  int G, chs;
  double step, inv_step, inv_last, z_max;
  __device__ __forceinline__ d2 at(int g) const { return tab[g + (g >> chs)]; }
};

// Cubic Hermite (nodes cum_dm, slopes dh), interval x[i] < xi <= x[i+1], linear extrapolation outside: interpolator.py:71-108
__device__ __forceinline__ double dq_hermite(const DqTable& T, double xi) {
  const int G = T.G;
  if (xi <= 0.0) {
    const d2 e = T.at(0);
    return e.x + e.y * (xi - 0.0);
  }
  if (xi >= T.z_max) {
    const d2 e = T.at(G - 1);
    return e.x + e.y * (xi - T.z_max);
  }
  int i = (int)(xi * T.inv_step);
  i = i > G - 2 ? G - 2 : i;
  double x0 = (double)i * T.step;
  if (x0 >= xi) {  // xi > 0, so i >= 1 here
    --i;
    x0 = (double)i * T.step;
  }
  double x1 = grid_z(i + 1, G, T.step, T.z_max);
  if (x1 < xi) {  // then i + 1 <= G - 2 because xi < z_max
    ++i;
    x0 = x1;
    x1 = grid_z(i + 1, G, T.step, T.z_max);
  }
  const double h_i = x1 - x0;
  const double t = (xi - x0) * (i == G - 2 ? T.inv_last : T.inv_step);
  const double t2 = t * t, t3 = t2 * t;
  const double h00 = 2 * t3 - 3 * t2 + 1;
  const double h10 = t3 - 2 * t2 + t;
  const double h01 = -2 * t3 + 3 * t2;
  const double h11 = t3 - t2;
  const d2 e0 = T.at(i), e1 = T.at(i + 1);
  return h00 * e0.x + h10 * h_i * e0.y + h01 * e1.x + h11 * h_i * e1.y;
}

// PCHIP of the dh grid (BAO D_H, bao/desi_cmb_des5y.py:88 -> interpolator.py:25-66,111-114): the two Fritsch-Carlson slopes at
// the bracketing nodes, clamped outside
__device__ __forceinline__ double dq_sgn(double v) { return (double)((v > 0) - (v < 0)); }

__device__ double dq_pchip_slope(const DqTable& T, int i) {
  const int n = T.G;
  auto X = [&](int k) { return grid_z(k, n, T.step, T.z_max); };
  auto Y = [&](int k) { return T.at(k).y; };
  if (i > 0 && i < n - 1) {
    const double hl = X(i) - X(i - 1), hr = X(i + 1) - X(i);
    const double dl = (Y(i) - Y(i - 1)) / hl, dr = (Y(i + 1) - Y(i)) / hr;
    if (dl != 0.0 && dr != 0.0 && dl * dr > 0.0) {
      const double w1 = 2.0 * hr + hl, w2 = hr + 2.0 * hl;
      return (w1 + w2) / (w1 / dl + w2 / dr);
    }
    return 0.0;
  }
  double h0, h1, d0, d1;
  if (i == 0) {
    h0 = X(1) - X(0); h1 = X(2) - X(1);
    d0 = (Y(1) - Y(0)) / h0; d1 = (Y(2) - Y(1)) / h1;
  } else {
    h0 = X(n - 1) - X(n - 2); h1 = X(n - 2) - X(n - 3);
    d0 = (Y(n - 1) - Y(n - 2)) / h0; d1 = (Y(n - 2) - Y(n - 3)) / h1;
  }
  const double e = ((2 * h0 + h1) * d0 - h0 * d1) / (h0 + h1);
  if (d0 == 0.0 || dq_sgn(e) != dq_sgn(d0)) return 0.0;
  if (dq_sgn(d0) != dq_sgn(d1) && fabs(e) > fabs(3 * d0)) return 3 * d0;
  return e;
}

__device__ double dq_pchip_dh(const DqTable& T, double xi) {
  const int G = T.G;
  if (xi <= 0.0) return T.at(0).y;
  if (xi >= T.z_max) return T.at(G - 1).y;
  int i = (int)(xi * T.inv_step);
  i = i > G - 2 ? G - 2 : i;
  if (i > 0 && grid_z(i, G, T.step, T.z_max) >= xi) --i;
  if (i < G - 2 && grid_z(i + 1, G, T.step, T.z_max) < xi) ++i;
  const double x0 = grid_z(i, G, T.step, T.z_max);
  const double h_i = grid_z(i + 1, G, T.step, T.z_max) - x0;
  const double t = (xi - x0) / h_i;
  const double t2 = t * t, t3 = t2 * t;
  const double h00 = 2 * t3 - 3 * t2 + 1, h10 = t3 - 2 * t2 + t, h01 = -2 * t3 + 3 * t2, h11 = t3 - t2;
  return h00 * T.at(i).y + h10 * h_i * dq_pchip_slope(T, i) + h01 * T.at(i + 1).y + h11 * h_i * dq_pchip_slope(T, i + 1);
}

// dynamic LDS: the skewed table (cosmofit_device.h: chunk_shift<DQ_TPB>, table_slots), then DQ_TPB chunk totals and the row's r_d

__global__ void __launch_bounds__(DQ_TPB)
curves_kernel(cf_dev_desc d, const double* __restrict__ theta, int64_t S, int code, int chs, const double* __restrict__ z, int nz,
              double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char dq_smem[];
  const int64_t row = blockIdx.x;
  if (row >= S) return;
  const int tid = threadIdx.x, G = d.n_grid;
  d2* tab = reinterpret_cast<d2*>(dq_smem);
  double* tot = reinterpret_cast<double*>(tab + table_slots(G, chs));  // [DQ_TPB] chunk totals, then r_d
  const double* th = theta + row * d.ndim;
  const DqCosmo wc = dq_cosmo(d, th);
  const bool need_rd = code == CF_CURVE_DV_RD || code == CF_CURVE_DM_RD || code == CF_CURVE_DH_RD;
  const bool need_table = !(code == CF_CURVE_H || (code == CF_CURVE_DH_RD && d.bao_dh_exact));
  if (need_rd && tid == 0)
    tot[DQ_TPB] = d.rd_from_fit ? dq_r_drag(d.rd_fit, wc.wb, dq_wm_drag(d, wc)) : dq_slot(d, CF_P_RD_D, th);
  if (need_table) {
    // dh = c / H at the nodes, node g = tid, tid + 256, ... (bao/desi_cmb.py:61)
    for (int g = tid; g < G; g += DQ_TPB) {
      const double nu = d.nu_grid ? d.nu_grid[g] : -1.0;
      tab[g + (g >> chs)].y = d.c / (wc.H0 * sqrt(dq_e2(d, wc, grid_z(g, G, d.step, d.z_max), nu)));
    }
    __syncthreads();
    // cumulative trapezoid (:62-64): thread t sums its 2^chs nodes in order, then the totals of the threads before it in order
    const int g0 = tid << chs;
    const int n_own = max(0, min(1 << chs, G - g0));
    double run = 0.0;
    double prev = (g0 > 0 && n_own > 0) ? tab[(g0 - 1) + ((g0 - 1) >> chs)].y : 0.0;
    for (int k = 0; k < n_own; ++k) {
      const int g = g0 + k, p = g + (g >> chs);
      const double cur = tab[p].y;
      if (g >= 1) run += (prev + cur) / 2 * (grid_z(g, G, d.step, d.z_max) - grid_z(g - 1, G, d.step, d.z_max));
      tab[p].x = run;
      prev = cur;
    }
    tot[tid] = run;
    __syncthreads();
    double carry = 0.0;
    for (int u = 0; u < tid; ++u) carry += tot[u];
    for (int k = 0; k < n_own; ++k) {
      const int g = g0 + k;
      tab[g + (g >> chs)].x += carry;
    }
  }
  __syncthreads();
  DqTable T;
  T.tab = tab; T.G = G; T.chs = chs;
  T.step = d.step; T.inv_step = d.inv_step; T.inv_last = d.inv_last; T.z_max = d.z_max;
  const double rd = need_rd ? tot[DQ_TPB] : 1.0;
  double* o = out + row * (int64_t)nz;
  for (int k = tid; k < nz; k += DQ_TPB) {
    const double zq = z[k];
    double v = __builtin_nan("");
    if (isfinite(zq)) {
      double DM = 0.0, DH = 0.0;
      if (code != CF_CURVE_H && code != CF_CURVE_DH_RD) DM = dq_hermite(T, zq);
      if (code == CF_CURVE_DV_RD || code == CF_CURVE_DH_RD || code == CF_CURVE_FAP)
        DH = d.bao_dh_exact ? d.c / dq_H(d, wc, zq) : dq_pchip_dh(T, zq);  // bao/desi_cmb.py:54-56 / bao/desi_cmb_des5y.py:88
      switch (code) {
        case CF_CURVE_H: v = dq_H(d, wc, zq); break;
        case CF_CURVE_DM: v = DM; break;
        case CF_CURVE_DV_RD: v = pow(zq * DH * (DM * DM), 1.0 / 3) / rd; break;  // bao/desi_cmb.py:68-72
        case CF_CURVE_DM_RD: v = DM / rd; break;
        case CF_CURVE_DH_RD: v = DH / rd; break;
        case CF_CURVE_FAP: v = DM / DH; break;
        default: v = 25 + 5 * log10((1 + zq) * DM); break;  // sn/pantheon.py:52-54
      }
    }
    o[k] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// Launchers (arguments are validated by the entry points below)
// ------------------------------------------------------------------------------------------------
static int cf_derived_launch(const cf_dev_desc& d, const cf_derived_kargs& a, const double* d_theta, int64_t S, double* d_out,
                      hipStream_t st) {
  const int64_t blocks = (S + DQ_TPB - 1) / DQ_TPB;
  hipLaunchKernelGGL(derived_kernel, dim3((unsigned)blocks), dim3(DQ_TPB), 0, st, d, a, d_theta, S, d_out);
  return cf_launch_status("cf_derived_device");
}

static int cf_curves_launch(const cf_dev_desc& d, const double* d_theta, int64_t S, int code, const double* d_z, int nz, double* d_out,
                     hipStream_t st) {
  const int chs = chunk_shift<DQ_TPB>(d.n_grid);
  const size_t lds = table_slots(d.n_grid, chs) * sizeof(d2) + (DQ_TPB + 2) * sizeof(double);
  // 4000 nodes are 64 KB of table: at the 64 KiB a launch may take by default.  The first launch on a device raises the kernel's
  // allowance, once, to the largest table cf_create accepts (8192 nodes).
  static std::atomic<bool> raised[DQ_MAX_DEVICES];
  const int max_lds = (int)(table_slots(8192, chunk_shift<DQ_TPB>(8192)) * sizeof(d2) + (DQ_TPB + 2) * sizeof(double));
  if (lds > 32 * 1024) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return cf_set_error(CF_ERR_HIP, "cf_curves_device: hipGetDevice failed");
    if (dev >= DQ_MAX_DEVICES || !raised[dev].load(std::memory_order_acquire)) {
      if (hipFuncSetAttribute((const void*)&curves_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds) != hipSuccess)
        return cf_set_error(CF_ERR_HIP, "cf_curves_device: " + std::to_string(max_lds) + " bytes of dynamic LDS refused on device " +
                                            std::to_string(dev));
      if (dev < DQ_MAX_DEVICES) raised[dev].store(true, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(curves_kernel, dim3((unsigned)S), dim3(DQ_TPB), lds, st, d, d_theta, S, code, chs, d_z, nz, d_out);
  return cf_launch_status("cf_curves_device");
}

// ------------------------------------------------------------------------------------------------
// Entry points: what each quantity and curve needs of the handle, the device paths and their host-buffer twins
// ------------------------------------------------------------------------------------------------

static const char* dq_name(int code) {
  switch (code) {
    case CF_DQ_H0: return "H0";
    case CF_DQ_H: return "h";
    case CF_DQ_OM: return "Om";
    case CF_DQ_OMH2: return "omh2";
    case CF_DQ_OBH2: return "obh2";
    case CF_DQ_OCH2: return "och2";
    case CF_DQ_W0: return "w0";
    case CF_DQ_WA: return "wa";
    case CF_DQ_Q0: return "q0";
    case CF_DQ_J0: return "j0";
    case CF_DQ_S8: return "S8";
    case CF_DQ_RD: return "rd";
    case CF_DQ_Z_STAR: return "z_star";
    case CF_DQ_R_DRAG: return "r_drag";
    case CF_DQ_Z_DRAG: return "z_drag";
    case CF_DQ_Z_EQ: return "z_eq";
    case CF_DQ_H_AT: return "H@z";
    case CF_DQ_RS_STAR: return "rs_star";
    case CF_DQ_DM_STAR: return "DM_star";
    case CF_DQ_THETA_STAR100: return "theta_star100";
    case CF_DQ_R: return "R";
    case CF_DQ_LA: return "lA";
    default: return nullptr;
  }
}
static const char* curve_name(int code) {
  static const char* names[] = {"H", "DM", "DV_rd", "DM_rd", "DH_rd", "F_AP", "mu"};
  return code >= CF_CURVE_H && code <= CF_CURVE_MU ? names[code] : nullptr;
}

// a slot the descriptor filled: a theta index, or a non-zero constant (an unused slot is {idx -1, fixed 0})
static bool slot_present(const cf_dev_desc& d, int s) { return d.slot[s].idx >= 0 || d.slot[s].fixed != 0.0; }

// What a quantity reads of the handle; the first thing that is missing, or nullptr.
static const char* missing_h0(const cf_dev_desc& d) { return slot_present(d, CF_P_H0) ? nullptr : "an H0 slot"; }
static const char* missing_wb_wc(const cf_dev_desc& d) {
  if (!slot_present(d, CF_P_OBH2)) return "an obh2 slot";
  if (!slot_present(d, CF_P_OCH2)) return "an och2 slot";
  return nullptr;
}
static const char* missing_om(const cf_dev_desc& d) {
  if (d.ez_model == CF_EZ_PHYSICAL) {
    if (const char* m = missing_h0(d)) return m;
    return missing_wb_wc(d);
  }
  if (!slot_present(d, CF_P_OM)) return "an Om slot";
  return d.om_mode ? missing_h0(d) : nullptr;
}
static const char* missing_wm_drag(const cf_dev_desc& d) {  // wb and the matter density of the r_drag / z_drag fits
  if (!slot_present(d, CF_P_OBH2)) return "an obh2 slot";
  if (d.rd_wm_late) {
    if (const char* m = missing_h0(d)) return m;
    return slot_present(d, CF_P_OM) ? nullptr : "an Om slot";
  }
  return slot_present(d, CF_P_OCH2) ? nullptr : "an och2 slot";
}
static const char* missing_rd(const cf_dev_desc& d) {
  if (d.rd_from_fit) return missing_wm_drag(d);
  return slot_present(d, CF_P_RD) ? nullptr : "an r_d slot or the r_drag fit (CF_RD_FIT)";
}

static int derived_prepare(cf_handle* h, const int32_t* codes, const double* args, int32_t n_q, const cf_derived_consts* consts,
                           cf_derived_kargs& a, const char* fn) {
  const std::string F = std::string(fn) + ": ";
  if (h->qsr) return cf_set_error(CF_ERR_UNSUPPORTED, F + "a quasar handle has no derived quantities");
  if (!h->peers.empty()) return cf_set_error(CF_ERR_INVALID, F + "this handle spans several devices; use one handle per device");
  if (!codes) return cf_set_error(CF_ERR_INVALID, F + "null argument");
  if (n_q < 1 || n_q > CF_DQ_MAX) return cf_set_error(CF_ERR_INVALID, F + "n_q must be in 1.." + std::to_string(CF_DQ_MAX));
  if (consts && consts->struct_size != (int32_t)sizeof(cf_derived_consts)) return cf_set_error(CF_ERR_INVALID, F + "cf_derived_consts.struct_size mismatch");
  const cf_dev_desc& d = h->d;
  memset(&a, 0, sizeof(a));
  a.n_q = n_q;
  for (int q = 0; q < n_q; ++q) {
    const int code = codes[q];
    const char* name = dq_name(code);
    if (!name) return cf_set_error(CF_ERR_INVALID, F + "unknown quantity code " + std::to_string(code));
    const char* miss = nullptr;
    double arg = args ? args[q] : 0.0;
    switch (code) {
      case CF_DQ_H0: case CF_DQ_H: miss = missing_h0(d); break;
      case CF_DQ_OM: case CF_DQ_Q0: case CF_DQ_J0: miss = missing_om(d); break;
      case CF_DQ_OMH2:
        miss = d.ez_model == CF_EZ_PHYSICAL ? missing_wb_wc(d) : (missing_h0(d) ? missing_h0(d) : missing_om(d));
        break;
      case CF_DQ_OBH2: miss = slot_present(d, CF_P_OBH2) ? nullptr : "an obh2 slot"; break;
      case CF_DQ_OCH2: miss = slot_present(d, CF_P_OCH2) ? nullptr : "an och2 slot"; break;
      case CF_DQ_W0: case CF_DQ_WA: break;
      case CF_DQ_S8: miss = slot_present(d, CF_P_S8) ? missing_om(d) : "a sigma8 slot"; break;
      case CF_DQ_RD:
        miss = missing_rd(d);
        if (d.rd_from_fit) a.need |= CF_DQ_NEED_RDFIT;
        break;
      case CF_DQ_Z_STAR:
        miss = d.cmb_mode == CF_CMB_NONE ? "a compressed-CMB block (z_star coefficients)" : missing_wb_wc(d);
        a.need |= CF_DQ_NEED_ZSTAR;
        break;
      case CF_DQ_R_DRAG:
        miss = (d.rd_from_fit || (consts && consts->has_rdrag_fit)) ? missing_wm_drag(d) : "r_drag coefficients (CF_RD_FIT or cf_derived_consts.rdrag_fit)";
        a.need |= CF_DQ_NEED_RDFIT;
        break;
      case CF_DQ_Z_DRAG:
        miss = consts ? missing_wm_drag(d) : "cf_derived_consts.zdrag_fit";
        a.need |= CF_DQ_NEED_ZDRAG;
        break;
      case CF_DQ_Z_EQ:
        miss = missing_wb_wc(d);
        if (!(arg > 0.0)) arg = consts ? consts->zeq_or_h2 : 0.0;
        if (!miss && !(arg > 0.0 && std::isfinite(arg))) miss = "Omega_r h^2 > 0 (arg or cf_derived_consts.zeq_or_h2)";
        break;
      case CF_DQ_H_AT:
        miss = missing_h0(d) ? missing_h0(d) : (std::isfinite(arg) ? nullptr : "a finite redshift");
        break;
      default:  // the Gauss-Legendre quantities
        miss = (d.n_gl < 1 || !d.gl_x || !d.gl_w) ? "Gauss-Legendre nodes (a compressed-CMB block)"
                                                  : (missing_h0(d) ? missing_h0(d) : missing_wb_wc(d));
        a.need |= CF_DQ_NEED_GL | CF_DQ_NEED_ZSTAR;
        break;
    }
    if (miss) return cf_set_error(CF_ERR_INVALID, F + name + " needs " + miss + ", which this handle lacks");
    a.codes[q] = code;
    a.args[q] = arg;
  }
  if (consts)
    for (int i = 0; i < 10; ++i) a.zdrag_fit[i] = consts->zdrag_fit[i];
  for (int i = 0; i < 11; ++i) a.rdrag_fit[i] = d.rd_from_fit ? d.rd_fit[i] : (consts && consts->has_rdrag_fit ? consts->rdrag_fit[i] : 0.0);
  return CF_OK;
}

static int curves_check(cf_handle* h, int32_t code, int32_t nz, const char* fn) {
  const std::string F = std::string(fn) + ": ";
  if (h->qsr) return cf_set_error(CF_ERR_UNSUPPORTED, F + "a quasar handle has no prediction curves; use cf_qsr_eval_parts");
  if (!h->peers.empty()) return cf_set_error(CF_ERR_INVALID, F + "this handle spans several devices; use one handle per device");
  const char* name = curve_name(code);
  if (!name) return cf_set_error(CF_ERR_INVALID, F + "unknown curve code " + std::to_string(code));
  if (nz < 1 || nz > CF_CURVE_MAX_NZ) return cf_set_error(CF_ERR_INVALID, F + "nz must be in 1.." + std::to_string(CF_CURVE_MAX_NZ));
  const cf_dev_desc& d = h->d;
  const char* miss = missing_h0(d);
  if (!miss && d.ez_model == CF_EZ_PHYSICAL) miss = missing_wb_wc(d);
  if (!miss && d.ez_model != CF_EZ_PHYSICAL) miss = missing_om(d);
  if (!miss && (code == CF_CURVE_DV_RD || code == CF_CURVE_DM_RD || code == CF_CURVE_DH_RD)) miss = missing_rd(d);
  if (!miss && !d.bao_dh_exact && d.n_grid < 3 && (code == CF_CURVE_DV_RD || code == CF_CURVE_DH_RD || code == CF_CURVE_FAP))
    miss = "n_grid >= 3 (PCHIP D_H)";
  if (miss) return cf_set_error(CF_ERR_INVALID, F + name + " needs " + miss + ", which this handle lacks");
  return CF_OK;
}

#define CF_DQ_MAX_ROWS (((int64_t)1 << 31) - 1)

extern "C" int cf_derived_device(cf_handle* h, const double* d_theta, int64_t S, const int32_t* codes, const double* args, int32_t n_q,
                                 const cf_derived_consts* consts, double* d_out, void* hip_stream) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_derived_device: null argument");
  cf_derived_kargs a;
  int rc = derived_prepare(h, codes, args, n_q, consts, a, "cf_derived_device");
  if (rc) return rc;
  if (S < 0 || S > CF_DQ_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, "cf_derived_device: S out of range");
  if (S == 0) return CF_OK;
  if (!d_theta || !d_out) return cf_set_error(CF_ERR_INVALID, "cf_derived_device: null argument");
  HandleScope hs(h);
  HIP_TRY(hs.err);
  return cf_derived_launch(h->d, a, d_theta, S, d_out, (hipStream_t)hip_stream);
}

extern "C" int cf_curves_device(cf_handle* h, const double* d_theta, int64_t S, int32_t code, const double* d_z, int32_t nz,
                                double* d_out, void* hip_stream) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_curves_device: null argument");
  int rc = curves_check(h, code, nz, "cf_curves_device");
  if (rc) return rc;
  if (S < 0 || S > CF_DQ_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, "cf_curves_device: S out of range");
  if (S == 0) return CF_OK;
  if (!d_theta || !d_z || !d_out) return cf_set_error(CF_ERR_INVALID, "cf_curves_device: null argument");
  HandleScope hs(h);
  HIP_TRY(hs.err);
  return cf_curves_launch(h->d, d_theta, S, code, d_z, nz, d_out, (hipStream_t)hip_stream);
}

// Host-buffer twins: rows in chunks through temporary device buffers on the handle's own stream.
#define CF_DQ_HOST_CHUNK 65536

extern "C" int cf_derived(cf_handle* h, const double* theta, int64_t S, const int32_t* codes, const double* args, int32_t n_q,
                          const cf_derived_consts* consts, double* out) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_derived: null argument");
  cf_derived_kargs a;
  int rc = derived_prepare(h, codes, args, n_q, consts, a, "cf_derived");
  if (rc) return rc;
  if (S < 0 || S > CF_DQ_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, "cf_derived: S out of range");
  if (S == 0) return CF_OK;
  if (!theta || !out) return cf_set_error(CF_ERR_INVALID, "cf_derived: null argument");
  HandleScope hs(h);
  HIP_TRY(hs.err);
  RowStage rows(h->stream, std::min<int64_t>(S, CF_DQ_HOST_CHUNK));
  const double* dth = rows.in(theta, (size_t)h->d.ndim * 8);
  double* dout = rows.out(out, (size_t)n_q * 8);
  return rows.run(S, [&](int64_t, int64_t m) { return cf_derived_launch(h->d, a, dth, m, dout, h->stream); });
}

extern "C" int cf_curves(cf_handle* h, const double* theta, int64_t S, int32_t code, const double* z, int32_t nz, double* out) {
  if (!h) return cf_set_error(CF_ERR_INVALID, "cf_curves: null argument");
  int rc = curves_check(h, code, nz, "cf_curves");
  if (rc) return rc;
  if (S < 0 || S > CF_DQ_MAX_ROWS) return cf_set_error(CF_ERR_INVALID, "cf_curves: S out of range");
  if (S == 0) return CF_OK;
  if (!theta || !z || !out) return cf_set_error(CF_ERR_INVALID, "cf_curves: null argument");
  HandleScope hs(h);
  HIP_TRY(hs.err);
  RowStage rows(h->stream, std::min<int64_t>(S, std::max<int64_t>(1, CF_DQ_HOST_CHUNK * 16 / nz)));
  const double* dth = rows.in(theta, (size_t)h->d.ndim * 8);
  double* dout = rows.out(out, (size_t)nz * 8);
  DevBuf dz;
  if (dz.ensure((size_t)nz * 8)) return CF_ERR_HIP;
  HIP_TRY(hipMemcpyAsync(dz.p, z, (size_t)nz * 8, hipMemcpyHostToDevice, h->stream));
  return rows.run(S, [&](int64_t, int64_t m) {
    return cf_curves_launch(h->d, dth, m, code, dz.as<const double>(), nz, dout, h->stream);
  });
}
