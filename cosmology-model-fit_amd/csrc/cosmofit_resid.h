// cosmofit_resid.h -- what the three loops over chunks of residual rows share (fit report: cosmofit_resid.hip, its owner; mocks:
// cosmofit_mock.hip; attribution: cosmofit_infl.hip), and the fit report's share of cf_create (cosmofit_api.hip).
#ifndef COSMOFIT_RESID_H
#define COSMOFIT_RESID_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/cosmofit.h"
#include "cf_host.h"

// Where the residuals of a chunk lie.  SN block: r = delta[s][i] (row pitch n_ld), y = obs[i] - mu_corr[s][i] (the
// `corrected_mags` of sn/pantheon.py:154).  BAO block: r = val[i] - theory[s][i], y = val[i] (bao/desi_fs_lya.py:96-141).
struct cf_resid_src {
  const double* rows;   // SN: the workspace's residual rows; BAO: bao_theory rows
  const double* data;   // SN: obs; BAO: val
  const double* mu_corr;  // SN only, [rows][n]
  const double* sigma;  // [n] sqrt(C_ii)
  int64_t pitch;        // doubles between rows of `rows`
  int32_t n, bao;
};

struct cf_resid_thr {
  double t[CF_RESID_MAX_THR];
  int32_t n_thr, pad;
};

// the per-row outputs of the likelihood's kernels, assembled into the ten chi2_blocks columns of cf_eval_parts
struct cf_resid_blocks {
  const double* sn;    // [rows] chi2 of the SN block
  const double* b8;    // [rows][8] small_blocks_kernel's (bao, cmb, cmb vector[3], cc, z*, r_d)
  const double* fs8;   // [rows] chi2 of the growth-rate block
  double* out;         // [rows][10] or null
};

// One chunk of `rows` rows whose residuals lie at `src`: kernel A when d_sample or blk.out is set, kernel B when acc is.
int cf_resid_launch(const cf_resid_src& src, int64_t rows, double* d_sample, const cf_resid_blocks& blk, const double* d_w,
                    const double* thresholds, int32_t n_thr, const cf_resid_acc* acc, hipStream_t st);

#define CF_RESID_MAX_ROWS (((int64_t)1 << 31) - 1)
#define CF_RESID_MAX_CHUNK 65536
#define CF_RESID_HOST_PIECE 65536  // rows per piece of the host-buffer twins

// What cf_resid and cf_infl check alike (F: "<entry point>: ").
int check_block(const std::string& F, int64_t n_sn, int32_t n_bao, int32_t block);
int check_rows_thresholds(const std::string& F, int64_t S, const double* thresholds, int32_t n_thr);
bool acc_lacks_an_array(const cf_resid_acc* acc, int32_t n_thr);
// The chunk buffers of the accessor path's outputs for `rows` rows, and the device copy of sigma.
struct HandleScope;
int resid_prepare(const HandleScope& hs, int64_t rows);
// cf_create's work for the fit report: sqrt(C_ii) of the SN data from the factor L, of the BAO data from their inverse covariance.
void resid_sn_sigma(const double* L, int64_t n, int64_t ld, std::vector<double>& out);
void resid_bao_sigma(const double* inv_cov, int n, std::vector<double>& out);

// The device twin of a host cf_resid_acc: up once, continued piece by piece on the device, down at the end.
struct HostAccTwin {
  DevBuf w, mean, m2, ex, used, skip;
  cf_resid_acc dev{};
  cf_resid_acc* host = nullptr;
  int up(cf_resid_acc* acc, hipStream_t st) {
    host = acc;
    if (!acc) return 0;
    const size_t nb = (size_t)acc->n * 8, ne = nb * (size_t)acc->n_thr;
    dev = *acc;
    if (w.ensure(nb) || mean.ensure(nb) || m2.ensure(nb) || used.ensure(nb) || skip.ensure(nb) || (ne && ex.ensure(ne))) return CF_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(w.p, acc->w_sum, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(mean.p, acc->mean, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m2.p, acc->m2, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(used.p, acc->n_used, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(skip.p, acc->n_skipped, nb, hipMemcpyHostToDevice, st));
    if (ne) HIP_TRY(hipMemcpyAsync(ex.p, acc->exceed, ne, hipMemcpyHostToDevice, st));
    dev.w_sum = w.as<double>(); dev.mean = mean.as<double>(); dev.m2 = m2.as<double>(); dev.exceed = ex.as<double>();
    dev.n_used = used.as<int64_t>(); dev.n_skipped = skip.as<int64_t>();
    return 0;
  }
  int down() {
    if (!host) return 0;
    const size_t nb = (size_t)host->n * 8, ne = nb * (size_t)host->n_thr;
    HIP_TRY(hipMemcpy(host->w_sum, w.p, nb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host->mean, mean.p, nb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host->m2, m2.p, nb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host->n_used, used.p, nb, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host->n_skipped, skip.p, nb, hipMemcpyDeviceToHost));
    if (ne) HIP_TRY(hipMemcpy(host->exceed, ex.p, ne, hipMemcpyDeviceToHost));
    return 0;
  }
  const cf_resid_acc* ptr() const { return host ? &dev : nullptr; }
};

#endif
