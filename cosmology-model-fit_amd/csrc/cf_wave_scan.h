// cf_wave_scan.h — the wave64 inclusive scan on DPP row operations, shared by the distance-table builds of
// cosmofit_kernels.hip and cosmofit_quasar.hip.
#ifndef CF_WAVE_SCAN_H
#define CF_WAVE_SCAN_H

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

#endif
