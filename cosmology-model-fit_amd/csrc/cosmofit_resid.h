// cosmofit_resid.h -- what cosmofit_api.hip (the launcher of cf_resid_device) and cosmofit_resid.hip (the kernels) share.
#ifndef COSMOFIT_RESID_H
#define COSMOFIT_RESID_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cosmofit.h"

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

#endif
