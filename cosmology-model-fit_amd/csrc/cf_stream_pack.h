// cf_stream_pack.h — create-time packing for the streaming per-walker kernel (walker_stream_kernel, cosmofit_kernels.hip).
// Plain host C++ (no HIP): tools/stream_pack_check.cpp runs it under the sanitizers.
//
// The kernel builds the distance table CF_STREAM_SEG nodes at a time and keeps one segment plus a halo of CF_STREAM_HALO nodes
// of the segment before in LDS.  An SN is evaluated right after the segment whose window holds the interval of its z_cmb at
// least CF_STREAM_HALO / 2 nodes from either edge, so that the peculiar-velocity shift of z_cosmo (a few nodes inside any prior
// box) cannot leave the window; the kernel checks that per walker (cf_stream_shift_bound against CF_STREAM_GUARD_NODES).
#ifndef CF_STREAM_PACK_H
#define CF_STREAM_PACK_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "cosmofit_device.h"

struct cf_stream_plan {
  std::vector<int32_t> row;  // row[j]: index of the SN evaluated j-th (sorted by the node of z_cmb, ties in input order)
  int32_t seg_off[CF_STREAM_MAX_SEGS + 1];
  int32_t n_seg;
  double max_step, zp1_max;
};

// step: the step weights or null (no velocity step: max_step = 0).  Returns false when the grid does not fit the kernel.
static inline bool cf_stream_assign(const double* z_cmb, const double* step, int64_t n_sn, int n_grid, double inv_step, double z_max,
                                    cf_stream_plan& plan) {
  if (n_grid < 2 || n_grid > CF_STREAM_SEG * CF_STREAM_MAX_SEGS || n_sn < 0 || n_sn > INT32_MAX - CF_STREAM_REC_SLACK) return false;
  plan.n_seg = (n_grid + CF_STREAM_SEG - 1) / CF_STREAM_SEG;
  std::vector<int32_t> node((size_t)n_sn);
  plan.max_step = 0.0;
  plan.zp1_max = 1.0;
  for (int64_t i = 0; i < n_sn; ++i) {
    // a non-finite redshift or weight has no window it stays in: such data keep the workgroup form
    if (!std::isfinite(z_cmb[i]) || (step && !std::isfinite(step[i]))) return false;
    node[(size_t)i] = cf_stream_node(z_cmb[i], n_grid, inv_step, z_max);
    if (step) plan.max_step = std::max(plan.max_step, std::fabs(step[i]));
    plan.zp1_max = std::max(plan.zp1_max, 1.0 + z_cmb[i]);
  }
  plan.row.resize((size_t)n_sn);
  std::iota(plan.row.begin(), plan.row.end(), 0);
  std::stable_sort(plan.row.begin(), plan.row.end(), [&](int32_t a, int32_t b) { return node[(size_t)a] < node[(size_t)b]; });
  for (int s = 0; s <= CF_STREAM_MAX_SEGS; ++s) plan.seg_off[s] = (int32_t)n_sn;
  // the segment is monotone in the node: offsets by one pass over the sorted order
  int s = 0;
  plan.seg_off[0] = 0;
  for (int64_t j = 0; j < n_sn; ++j) {
    const int sj = cf_stream_segment(node[(size_t)plan.row[(size_t)j]], plan.n_seg);
    while (s < sj) plan.seg_off[++s] = (int32_t)j;
  }
  while (s < CF_STREAM_MAX_SEGS) plan.seg_off[++s] = (int32_t)n_sn;
  return true;
}

// The wave priority (s_setprio level, 0 .. 3) a walker's wave takes at the top of segment s: it falls 3 -> 0 as the share of the
// walker's work already done rises, so that of the four waves of a SIMD the one that is behind outranks the one that is ahead
// (the hardware arbitrates by priority, then age: at equal priority the oldest wave runs ahead and the four finish one after
// another).  Cost of a segment in vector instructions, from the compiled kernel (profiles/NOTES_walker_stream.md section 2): the
// table build, and one trip of the SN loop per 64 records.  A function of seg_off and n_seg alone.  One segment: nothing to
// level, 0.  Segments past n_seg: 0.
#define CF_STREAM_COST_BUILD 230
#define CF_STREAM_COST_TRIP 60
static inline void cf_stream_levels(const int32_t* seg_off, int n_seg, int32_t level[CF_STREAM_MAX_SEGS]) {
  int64_t cost[CF_STREAM_MAX_SEGS], total = 0;
  for (int s = 0; s < CF_STREAM_MAX_SEGS; ++s) {
    level[s] = 0;
    cost[s] = 0;
    if (s >= n_seg) continue;
    const int64_t n = (int64_t)seg_off[s + 1] - (int64_t)seg_off[s];
    cost[s] = CF_STREAM_COST_BUILD + CF_STREAM_COST_TRIP * ((std::max<int64_t>(n, 0) + 63) / 64);
    total += cost[s];
  }
  if (n_seg < 2) return;
  int64_t before = 0;
  for (int s = 0; s < n_seg && s < CF_STREAM_MAX_SEGS; ++s) {
    level[s] = (int32_t)std::min<int64_t>(3, std::max<int64_t>(0, 3 - 4 * before / total));
    before += cost[s];
  }
}
// the table as the kernel takes it: four bits per segment
static inline uint32_t cf_stream_levels_packed(const int32_t level[CF_STREAM_MAX_SEGS]) {
  uint32_t p = 0;
  for (int s = 0; s < CF_STREAM_MAX_SEGS; ++s) p |= (uint32_t)(level[s] & 3) << (4 * s);
  return p;
}

#endif
