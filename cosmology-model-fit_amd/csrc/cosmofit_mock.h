// cosmofit_mock.h -- what cosmofit_api.hip (the launcher of cf_mock_eval_device) and cosmofit_mock.hip (the kernels) share.
#ifndef COSMOFIT_MOCK_H
#define COSMOFIT_MOCK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cosmofit.h"

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

// One chunk of `rows` rows: d_out[s] and d_cross[3 s + b] (null: not wanted) for the mocks d_mock[s].
int cf_mock_launch(const cf_mock_args& a, int64_t rows, const int32_t* d_mock, double* d_out, double* d_cross, hipStream_t st);

#endif
