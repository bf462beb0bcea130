// cosmofit_group.h -- what cosmofit_infl.hip (the owner of cf_prec) and cosmofit_group.hip (the group object, its kernels and the
// importance summary) share.
#ifndef COSMOFIT_GROUP_H
#define COSMOFIT_GROUP_H
#include <stdint.h>

#include "../../include/cosmofit.h"

// A read-only look at a cf_prec: K on its device (row-major at pitch kp = n rounded up to 16, zero in the padding) and the
// host copy of its diagonal.  Valid while the cf_prec lives.
struct cf_prec_view {
  int64_t n, kp;
  int device;
  const double* d_K;
  const double* kdiag_host;
};
int cf_prec_look(const cf_prec* p, cf_prec_view* out);  // cosmofit_infl.hip; CF_ERR_INVALID for a null cf_prec

#endif
