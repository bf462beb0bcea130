// stream_pack_check.cpp — stand-alone check of the create-time packing of the streaming per-walker kernel (csrc/cf_stream_pack.h),
// meant to be built with -fsanitize=address,undefined (tests/test_stream_pack_cpu.py):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/stream_pack_check.cpp -o stream_pack_check && ./stream_pack_check
// For sorted, unsorted and duplicate redshifts, 1 .. 1701 SNe and grids of 520 / 1000 / 4000 / 4096 nodes it checks that every SN
// is evaluated exactly once, that the interval of its z_cmb (node and node + 1) lies at least HALO / 2 - 1 nodes inside the window
// of its segment (the grid's own ends excepted: there is nothing beyond them), that the offsets are monotone and end at n_sn, and
// that the guard admits |v| = 300 km/s (the prior box of sn/pantheon.py) for the Pantheon+ shape.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../cosmology-model-fit_amd/csrc/cf_stream_pack.h"

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
    }                                    \
  } while (0)

static void check_plan(const std::vector<double>& z, const std::vector<double>* step, int G, double z_max, const char* what) {
  const int64_t n = (int64_t)z.size();
  const double inv_step = 1.0 / (z_max / (double)(G - 1));
  cf_stream_plan plan;
  const bool ok = cf_stream_assign(z.data(), step ? step->data() : nullptr, n, G, inv_step, z_max, plan);
  CHECK(ok, "%s n=%lld G=%d: refused", what, (long long)n, G);
  if (!ok) return;
  CHECK(plan.n_seg == (G + CF_STREAM_SEG - 1) / CF_STREAM_SEG, "%s: n_seg %d", what, plan.n_seg);
  CHECK(plan.seg_off[0] == 0, "%s: seg_off[0] = %d", what, plan.seg_off[0]);
  for (int s = 0; s < CF_STREAM_MAX_SEGS; ++s)
    CHECK(plan.seg_off[s] <= plan.seg_off[s + 1], "%s n=%lld G=%d: offsets not monotone at %d", what, (long long)n, G, s);
  CHECK(plan.seg_off[plan.n_seg] == n && plan.seg_off[CF_STREAM_MAX_SEGS] == n, "%s: offsets end at %d / %d, n = %lld", what,
        plan.seg_off[plan.n_seg], plan.seg_off[CF_STREAM_MAX_SEGS], (long long)n);
  std::vector<int> seen((size_t)n, 0);
  CHECK((int64_t)plan.row.size() == n, "%s: %zu rows for %lld SNe", what, plan.row.size(), (long long)n);
  for (int s = 0; s < plan.n_seg; ++s) {
    // the window of segment s: its own nodes and the halo in front; the grid's ends bound it too
    const int w_lo = s == 0 ? 0 : CF_STREAM_SEG * s - CF_STREAM_HALO;
    const int w_hi = std::min(CF_STREAM_SEG * s + CF_STREAM_SEG - 1, G - 1);
    for (int j = plan.seg_off[s]; j < plan.seg_off[s + 1]; ++j) {
      const int32_t r = plan.row[(size_t)j];
      CHECK(r >= 0 && r < n, "%s: row %d out of range", what, r);
      if (r < 0 || r >= n) continue;
      ++seen[(size_t)r];
      const int node = cf_stream_node(z[(size_t)r], G, inv_step, z_max);
      CHECK(node >= 0 && node + 1 <= G - 1, "%s: node %d of z = %g outside the grid", what, node, z[(size_t)r]);
      const int margin = CF_STREAM_HALO / 2 - 1;
      CHECK(w_lo == 0 || node - w_lo >= margin, "%s n=%lld G=%d: node %d only %d above the window's start %d (segment %d)", what,
            (long long)n, G, node, node - w_lo, w_lo, s);
      CHECK(w_hi == G - 1 || w_hi - (node + 1) >= margin, "%s n=%lld G=%d: node %d + 1 only %d below the window's end %d (segment %d)",
            what, (long long)n, G, node, w_hi - (node + 1), w_hi, s);
      CHECK(node + 1 <= w_hi && node >= w_lo, "%s: node %d outside the window [%d, %d]", what, node, w_lo, w_hi);
    }
  }
  for (int64_t i = 0; i < n; ++i) CHECK(seen[(size_t)i] == 1, "%s n=%lld G=%d: SN %lld evaluated %d times", what, (long long)n, G, (long long)i, seen[(size_t)i]);
  double ms = 0.0, zm = 1.0;
  for (int64_t i = 0; i < n; ++i) {
    if (step) ms = std::max(ms, std::fabs((*step)[(size_t)i]));
    zm = std::max(zm, 1.0 + z[(size_t)i]);
  }
  CHECK(plan.max_step == ms && plan.zp1_max == zm, "%s: max_step %g (%g), zp1_max %g (%g)", what, plan.max_step, ms, plan.zp1_max, zm);
}

int main() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  const int grids[4] = {520, 1000, 4000, 4096};
  const int sizes[] = {1, 2, 3, 63, 64, 65, 70, 200, 511, 512, 513, 1024, 1700, 1701};
  int plans = 0;
  for (int G : grids)
    for (int n : sizes) {
      // the Pantheon+ shape: 45 % in [0.01, 0.15], the rest out to 2.26; the grid ends 0.1 above the highest redshift
      std::vector<double> z((size_t)n), step((size_t)n);
      for (int i = 0; i < n; ++i) z[(size_t)i] = uni(rng) < 0.45 ? 0.01 + 0.14 * uni(rng) : 0.15 + 2.11 * uni(rng);
      double top = 0.0;
      for (double v : z) top = std::max(top, v);
      const double z_max = top + 0.1;
      for (int i = 0; i < n; ++i) step[(size_t)i] = z[(size_t)i] <= 0.15 ? 1.0 : -1.0;
      check_plan(z, &step, G, z_max, "unsorted");
      std::vector<double> zs = z;
      std::sort(zs.begin(), zs.end());
      check_plan(zs, nullptr, G, z_max, "sorted");
      std::vector<double> zd = z;
      for (int i = 1; i < n; i += 2) zd[(size_t)i] = zd[(size_t)i - 1];  // pairs of equal redshifts
      for (int i = 0; i < n; ++i) step[(size_t)i] = 1.9 * uni(rng) - 0.95;
      check_plan(zd, &step, G, z_max, "duplicates");
      // on and next to every segment and packing boundary, below the first node, at and above the last
      const double h = z_max / (double)(G - 1);
      std::vector<double> zb;
      for (int b = 0; b <= G; b += CF_STREAM_SEG)
        for (int o : {-CF_STREAM_HALO / 2 - 1, -CF_STREAM_HALO / 2, -CF_STREAM_HALO / 2 + 1, -1, 0, 1})
          for (double f : {0.0, 0.5, 0.999999})
            if (b + o >= 0) zb.push_back(((double)(b + o) + f) * h);
      zb.push_back(0.3 * h);
      zb.push_back(0.0);
      zb.push_back(z_max);
      zb.push_back(1.5 * z_max);
      check_plan(zb, nullptr, G, z_max, "boundaries");
      plans += 4;
    }
  // a redshift that is not finite has no window: the plan is refused (such data keep the workgroup form)
  {
    std::vector<double> z = {0.1, std::nan(""), 0.3};
    cf_stream_plan plan;
    CHECK(!cf_stream_assign(z.data(), nullptr, 3, 4000, 3999.0 / 2.36, 2.36, plan), "a NaN redshift was accepted");
    CHECK(!cf_stream_assign(z.data(), nullptr, 1, 5000, 4999.0 / 2.36, 2.36, plan), "a grid of 5000 nodes was accepted");
  }
  // the guard, for the Pantheon+ shape (z up to 2.26, grid of 4000 nodes to 2.36, +-1 step weights): the prior box's
  // |v| = 300 km/s must pass, and the bound must really bound the shift of z_cosmo in nodes
  {
    const double c = 299792.458, z_top = 2.26, z_max = 2.36, inv_step = 3999.0 / z_max;
    double a;
    const double at300 = cf_stream_shift_bound(300.0, 1.0, 1.0 + z_top, c, inv_step, &a);
    CHECK(a < 0.5 && at300 <= (double)CF_STREAM_GUARD_NODES, "guard refuses 300 km/s: bound %g nodes, limit %d", at300, CF_STREAM_GUARD_NODES);
    std::printf("guard: 300 km/s moves an SN by at most %.2f nodes (limit %d)\n", at300, CF_STREAM_GUARD_NODES);
    double v_lim = 300.0;
    while (cf_stream_shift_bound(v_lim + 1.0, 1.0, 1.0 + z_top, c, inv_step, &a) <= (double)CF_STREAM_GUARD_NODES) v_lim += 1.0;
    std::printf("guard: passes up to %.0f km/s\n", v_lim);
    for (double v : {-v_lim, -300.0, 300.0, v_lim})
      for (double z = 0.001; z <= z_top; z += 0.0007) {
        const double bound = cf_stream_shift_bound(v, 1.0, 1.0 + z_top, c, inv_step, &a);
        for (double st : {1.0, -1.0}) {
          const double z_cosmo = -1.0 + (1.0 + z) / (1.0 + v * st / c);
          CHECK(std::fabs(z_cosmo - z) * inv_step <= bound, "shift %g nodes above the bound %g at z = %g, v = %g", std::fabs(z_cosmo - z) * inv_step, bound, z, v);
          const int moved = std::abs(cf_stream_node(z_cosmo, 4000, inv_step, z_max) - cf_stream_node(z, 4000, inv_step, z_max));
          CHECK(moved <= CF_STREAM_HALO / 2 - 2, "node moved by %d at z = %g, v = %g", moved, z, v);
        }
      }
    CHECK(!(cf_stream_shift_bound(std::nan(""), 1.0, 1.0 + z_top, c, inv_step, &a) <= (double)CF_STREAM_GUARD_NODES), "NaN passes the guard");
  }
  std::printf("stream pack: %d plans checked, %d failures\n", plans, failures);
  return failures ? 1 : 0;
}
