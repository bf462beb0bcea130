// cf_wave.h — what the kernels do across the 64 lanes of a wave: the inclusive scan on DPP row operations (the distance-table
// builds of cosmofit_kernels.hip, cosmofit_quasar.hip and cosmofit_field.hip), and the butterfly sum and argmax of the
// one-wave-per-row kernels (cosmofit_resid.hip, cosmofit_infl.hip, cosmofit_mock.hip, cosmofit_cscale.hip).
#ifndef CF_WAVE_H
#define CF_WAVE_H

#include <hip/hip_runtime.h>

// Inclusive scan across the 64 lanes of a wave on DPP row operations (no LDS round trips, unlike
// ds_bpermute-based shuffles): Hillis-Steele inside each row of 16 lanes (row_shr 1, 2, 4, 8), then
// lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast:15) and lane 31 into rows 2-3 (row_bcast:31).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
  return __hiloint2double(hi, lo);  // lanes without a source (or outside ROW_MASK) get 0
}

__device__ __forceinline__ double wave_inclusive_scan(double v) {
  v += dpp_move<0x111, 0xF>(v);  // row_shr:1
  v += dpp_move<0x112, 0xF>(v);  // row_shr:2
  v += dpp_move<0x114, 0xF>(v);  // row_shr:4
  v += dpp_move<0x118, 0xF>(v);  // row_shr:8
  v += dpp_move<0x142, 0xA>(v);  // row_bcast:15 -> rows 1 and 3
  v += dpp_move<0x143, 0xC>(v);  // row_bcast:31 -> rows 2 and 3
  return v;
}

// The sum over the 64 lanes, in every lane: the xor butterfly 32, 16, .., 1.  The order is part of the results' bits (the host
// twins of the kernels add in the same tree), so every whole-wave sum goes through here.
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

// np.argmax's order on (value, index): a NaN beats every number, among equals the lower index wins
__device__ __forceinline__ bool argmax_before(double a, int ia, double b, int ib) {
  const bool an = a != a, bn = b != b;
  if (an != bn) return an;
  if (an || a == b) return ia < ib;
  return a > b;
}

// (v, idx) of the lane that comes first in that order, in every lane
__device__ __forceinline__ void wave_argmax(double& v, int& idx) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double vo = __shfl_xor(v, m);
    const int io = __shfl_xor(idx, m);
    if (argmax_before(vo, io, v, idx)) { v = vo; idx = io; }
  }
}

#endif
