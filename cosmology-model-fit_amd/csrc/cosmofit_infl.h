// cosmofit_infl.h -- what cosmofit_api.hip (the launcher of cf_infl_device / cf_prec_apply_device) and cosmofit_infl.hip (the
// kernels) share.
#ifndef COSMOFIT_INFL_H
#define COSMOFIT_INFL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cosmofit.h"

// Where the residuals of a chunk lie, as in cf_resid_src.  SN block (and caller-supplied rows): r = rows[s][i] (row pitch
// `pitch`, columns >= n are never read).  BAO block: r = data[i] - rows[s][i], formed where it is read.
struct cf_infl_src {
  const double* rows;
  const double* data;  // BAO: val; else unused
  int64_t pitch;       // doubles between rows of `rows`
  int32_t n, bao;
};

// what infl_row_kernel reads beside the residuals and writes: g at pitch g_pitch, the row arrays at pitch n (any may be null)
struct cf_infl_rows {
  const double* g;
  int64_t g_pitch;
  const double* kdiag;           // [n] K_ii
  const double* inv_sqrt_kdiag;  // [n] 1 / sqrt(K_ii), 0 where K_ii = 0
  double* contrib;
  double* z;
  double* loo;
  double* sample;                // [rows][CF_INFL_NCOL] or null
};

// G[rows, n] = R[rows, n] K[n, n]; K row-major at pitch kp = n rounded up to 16, zero in the padding.
int cf_prec_gemm_launch(const cf_infl_src& src, int64_t rows, const double* K, int64_t kp, double* g, int64_t g_pitch,
                        hipStream_t st);
int cf_infl_row_launch(const cf_infl_src& src, int64_t rows, const cf_infl_rows& a, hipStream_t st);

#endif
