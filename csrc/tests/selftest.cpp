// Host-only self-test of the native engine's CPU components (topology,
// decomposition, layouts, pass boxes and ghost bookkeeping, the TB launch
// planners, prtdat formatting, initial condition, CPU stencil, deep-halo
// invariance).  Built twice: plain
// (`make selftest`) and under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make selftest-asan`); the reference's latent OOB/UB bugs (SURVEY Q2, Q6,
// Q7) are the kind of thing the sanitizer build guards against here.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "heat/cpu_backend.hpp"
#include "heat/init_fn.hpp"
#include "heat/io.hpp"
#include "heat/plan.hpp"
#include "heat/tb_plan.hpp"
#include "heat/topology.hpp"

using namespace heat;

static int failures = 0;
#define EXPECT(c)                                                      \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static void test_dims() {
  const int want[][3] = {{1, 1, 1}, {2, 2, 1}, {6, 3, 2}, {8, 4, 2}, {10, 5, 2}, {12, 4, 3},
                         {16, 4, 4}, {7, 7, 1}, {36, 6, 6}};
  for (auto& w : want) {
    auto d = dims_create(w[0], 2);
    EXPECT(d[0] == w[1] && d[1] == w[2]);
  }
  auto d3 = dims_create(24, 3);
  EXPECT(d3[0] * d3[1] * d3[2] == 24 && d3[0] >= d3[1] && d3[1] >= d3[2]);
}

static void test_blocks() {
  for (int world : {1, 2, 3, 4, 6, 8}) {
    Cart c(world, DecompKind::Auto, 0, 0, 37, 53);
    int64_t cells = 0;
    for (int r = 0; r < world; ++r) {
      Block b = make_block(c, r, 37, 53);
      cells += b.lx * b.ly;
      auto n = c.neighbors(r);
      if (n[South] >= 0) EXPECT(make_block(c, n[South], 37, 53).ox == b.ox + b.lx);
      if (n[East] >= 0) EXPECT(make_block(c, n[East], 37, 53).oy == b.oy + b.ly);
    }
    EXPECT(cells == 37 * 53);
  }
  Layout L = Layout::make(7, 5, 3);
  EXPECT(L.pitch % 64 == 0 && L.hy == 4 && L.rows == 13 && L.origin() == 3 * L.pitch + 4);
}

static void test_format() {
  struct {
    float v;
    const char* s;
  } cases[] = {{0.f, "   0.0"}, {-0.f, "  -0.0"}, {0.25f, "   0.2"}, {0.75f, "   0.8"},
               {2.5f, "   2.5"}, {-12.34f, " -12.3"}, {123456.78f, "123456.8"},
               {-2147483648.f, "-2147483648.0"}};
  for (auto& c : cases) {
    std::string s;
    format_6_1f(c.v, s);
    EXPECT(s == c.s);
    char buf[64];
    std::snprintf(buf, sizeof buf, "%6.1f", double(c.v));
    EXPECT(s == buf);
  }
}

static void test_init_wrap() {
  // n = 1000 overflows int32: compare with explicit wrap-around arithmetic.
  const int64_t n = 1000;
  for (int64_t ix : {0L, 1L, 499L, 500L, 998L})
    for (int64_t iy : {0L, 3L, 500L, 997L}) {
      int64_t a = int32_t(uint32_t(ix * (n - ix - 1)));
      a = int32_t(uint32_t(a * iy));
      a = int32_t(uint32_t(a * (n - iy - 1)));
      EXPECT(init_ref_wrap(ix, iy, n, n) == float(int32_t(a)));
    }
  EXPECT(init_value(0, -1, 5, n, n, 0) == 0.f);
}

static void test_cpu_step_and_halo_invariance() {
  const int64_t nx = 29, ny = 31;
  // Reference: 12 single steps on a halo-1 layout.
  auto run = [&](int halo, int steps) {
    Layout L = Layout::make(nx, ny, halo);
    std::vector<float> a(size_t(L.elems())), b(size_t(L.elems()));
    cpu::init_field(a.data() + L.origin(), L, 0, 0, nx, ny, 2, 3);
    cpu::init_field(b.data() + L.origin(), L, 0, 0, nx, ny, 2, 3);
    cpu::Geom g;
    g.pitch = L.pitch;
    g.nx = nx;
    g.ny = ny;
    float* s = a.data() + L.origin();
    float* d = b.data() + L.origin();
    for (int k = 0; k < steps; ++k) {
      cpu::step(s, d, g, Box{0, nx, 0, ny}, false);
      std::swap(s, d);
    }
    std::vector<float> out(size_t(nx * ny));
    for (int64_t r = 0; r < nx; ++r) std::memcpy(&out[size_t(r * ny)], s + r * L.pitch, size_t(ny) * 4);
    return out;
  };
  auto x = run(1, 12), y = run(4, 12);
  EXPECT(x == y);
  // boundary ring unchanged
  EXPECT(x[0] == init_random(0, 0, 3) && x[size_t(nx * ny - 1)] == init_random(nx - 1, ny - 1, 3));
}

static bool same_box(const Box& b, int64_t r0, int64_t r1, int64_t c0, int64_t c1) {
  return b.r0 == r0 && b.r1 == r1 && b.c0 == c0 && b.c1 == c1;
}

// Span boxes worked out by hand (plan.hpp: Sides, GhostState, grown_box).
static void test_span_box_literals() {
  {  // 8192^2 on 8 x 1 at depth 12, m = 7: 1024-row slabs grown by 6 * 12 rows.
    Cart c(8, DecompKind::Auto, 8, 1, 8192, 8192);
    EXPECT(same_box(span_box(c, make_block(c, 3, 8192, 8192), 12, 7), -72, 1096, 0, 8192));
    EXPECT(span_box(c, make_block(c, 3, 8192, 8192), 12, 7).rows() == 1168);
    EXPECT(same_box(span_box(c, make_block(c, 0, 8192, 8192), 12, 7), 0, 1096, 0, 8192));
    EXPECT(same_box(span_box(c, make_block(c, 7, 8192, 8192), 12, 7), -72, 1024, 0, 8192));
  }
  {  // 2 x 2 at m = 5: 4096 + 4 * 12 = 4144 square; at depth 6, m = 4 the 18
     // columns round down to 16.
    Cart c(4, DecompKind::Auto, 2, 2, 8192, 8192);
    EXPECT(same_box(span_box(c, make_block(c, 0, 8192, 8192), 12, 5), 0, 4144, 0, 4144));
    EXPECT(same_box(span_box(c, make_block(c, 3, 8192, 8192), 12, 5), -48, 4096, -48, 4096));
    EXPECT(same_box(span_box(c, make_block(c, 1, 8192, 8192), 6, 4), 0, 4114, -16, 4096));
  }
  Cart one(1, DecompKind::Auto, 1, 1, 100, 200);
  const Block b = make_block(one, 0, 100, 200);
  // Insulated north and east (1 | 8) at depth 8, m = 3: both axes count, only
  // those two sides grow.
  EXPECT(same_box(span_box(one, b, 8, 3, 1 | 8, 0), -16, 100, 0, 216));
  // Periodic in y: west and east grow, the rows do not.
  EXPECT(same_box(span_box(one, b, 8, 3, 0, kPeriodicY), 0, 100, -16, 216));
  EXPECT(same_box(span_box(one, b, 8, 3), 0, 100, 0, 200));
}

// Sides, GhostState and grown_box against the rule restated naively, over m + 1
// passes from stale ghosts, on every rank of small grids.
static void test_pass_geometry_sweep() {
  const int64_t nx = 37, ny = 53;
  const int grids[][2] = {{1, 1}, {2, 1}, {1, 2}, {2, 2}, {3, 2}};
  int unrounded = 0;  // column growths off a float4 column: without tb only
  for (auto& pg : grids)
    for (unsigned ins = 0; ins < 16; ++ins)
      for (unsigned per = 0; per < 4; ++per) {
        if (((per & 1) && (ins & 3)) || ((per & 2) && (ins & 12))) continue;  // rejected up front
        Cart c(pg[0] * pg[1], DecompKind::Auto, pg[0], pg[1], nx, ny);
        const int64_t limit = halo_extent_limit(c, nx, ny, ins, per);
        for (int r = 0; r < c.world; ++r) {
          const Block b = make_block(c, r, nx, ny, per);
          const Sides s = make_sides(c, b, ins, per);
          // The naive rule: axis 0 = rows (sides 0, 1), axis 1 = columns (2, 3).
          const int64_t len[2] = {b.lx, b.ly};
          bool act[2], open[4];
          for (int a = 0; a < 2; ++a) {
            act[a] = (a == 0 ? c.px : c.py) > 1 || ((per >> a) & 1) != 0;
            for (int d = 2 * a; d < 2 * a + 2; ++d) {
              if ((ins >> d) & 1) act[a] = true;
              open[d] = b.nbr[size_t(d)] >= 0 || ((ins >> d) & 1) != 0 || ((per >> a) & 1) != 0;
            }
          }
          EXPECT(s.ns == act[0] && s.ew == act[1]);
          for (int d = 0; d < 4; ++d) EXPECT(s.open[d] == open[d]);
          for (int depth : {1, 2, 3, 8, 12})
            for (int m = 1; m <= 4 && int64_t(m) * depth <= limit; ++m)
              for (int tb = 0; tb < 2; ++tb) {
                const int64_t H = int64_t(m) * depth;
                GhostState g;
                int64_t valid[2] = {0, 0};
                for (int pass = 0; pass <= m; ++pass) {
                  bool need = false;
                  for (int a = 0; a < 2; ++a)
                    if (act[a] && valid[a] < depth) need = true;
                  EXPECT(g.needs_exchange(s, depth) == need);
                  if (pass == 0) EXPECT(need == (act[0] || act[1]));
                  if (need) {
                    g.refill(H);
                    valid[0] = valid[1] = H;
                  }
                  for (int a = 0; a < 2; ++a) valid[a] = act[a] ? valid[a] - depth : 0;
                  if (tb) valid[1] -= valid[1] % 4;
                  const auto e = g.advance(s, depth, tb != 0);
                  EXPECT(e.first == valid[0] && e.second == valid[1]);
                  EXPECT(g.gr == valid[0] && g.gc == valid[1]);
                  EXPECT(e.first >= 0 && e.second >= 0 && e.first <= H - depth);
                  if (tb) EXPECT(e.second % 4 == 0);
                  else if (e.second % 4 != 0) ++unrounded;
                  int64_t lo[2], hi[2];
                  for (int a = 0; a < 2; ++a) {
                    lo[a] = open[2 * a] ? -valid[a] : 0;
                    hi[a] = len[a] + (open[2 * a + 1] ? valid[a] : 0);
                  }
                  const Box box = grown_box(b.lx, b.ly, s, e.first, e.second);
                  EXPECT(same_box(box, lo[0], hi[0], lo[1], hi[1]));
                  if (pass == 0 && tb) {
                    const Box sb = span_box(c, b, depth, m, ins, per);
                    EXPECT(same_box(sb, box.r0, box.r1, box.c0, box.c1));
                  }
                }
              }
        }
      }
  EXPECT(unrounded > 0);
}

// The launches of a pass, walked as the solver walks them.
static std::vector<SubPass> sub_passes(int k, int rl, int group_max) {
  std::vector<SubPass> v;
  for (int j = 0; j < k; j += v.back().n) v.push_back(sub_pass(k, rl, group_max, j));
  return v;
}
// The same for the replay of a check's first rl steps: grow = the steps left.
template <class F>
static std::vector<SubPass> replay_sub_passes(int rl, F supported) {
  std::vector<SubPass> v;
  for (int left = rl; left > 0;) {
    const int d = replay_depth(left, supported(left));
    left -= d;
    v.push_back({d, left, false});
  }
  return v;
}

static void test_sub_passes() {
  for (int k = 1; k <= 12; ++k)
    for (int rl = 0; rl <= k; ++rl)
      for (int gmax : {1, 8}) {
        const auto v = sub_passes(k, rl, gmax);
        int j = 0, takers = 0;
        for (size_t i = 0; i < v.size(); ++i) {
          EXPECT(v[i].n >= 1 && v[i].n <= gmax);
          EXPECT(!(j < rl && j + v[i].n > rl));  // no group straddles rl
          EXPECT(v[i].takes_resid == (rl > 0 && j + v[i].n == rl));
          takers += v[i].takes_resid ? 1 : 0;
          j += v[i].n;
          EXPECT(v[i].grow == k - j);
          if (i > 0) EXPECT(v[i].grow < v[i - 1].grow);
        }
        EXPECT(j == k && takers == (rl > 0 ? 1 : 0));
        EXPECT(!v.empty() && v.front().grow == k - v.front().n && v.back().grow == 0);
        if (gmax == 1) EXPECT(int(v.size()) == k);
      }
  // A depth-12 source pass with a check after step 9, fused: 8 + 1 | 3.
  const auto v = sub_passes(12, 9, 8);
  EXPECT(v.size() == 3 && v[0].n == 8 && v[1].n == 1 && v[2].n == 3 && v[1].takes_resid);
  EXPECT(v[0].grow == 4 && v[1].grow == 3 && v[2].grow == 0);
  // The replay of a check's first rl steps: depths the kernel takes (1..8 and
  // 12, the TB kernels' set), the remainder first.
  auto supported = [](int d) { return (d >= 1 && d <= 8) || d == 12; };
  for (int rl = 1; rl <= 12; ++rl) {
    const auto w = replay_sub_passes(rl, supported);
    int sum = 0;
    for (size_t i = 0; i < w.size(); ++i) {
      EXPECT(supported(w[i].n) && !w[i].takes_resid);
      sum += w[i].n;
      EXPECT(w[i].grow == rl - sum);
      if (i > 0) EXPECT(w[i].n == 8);
    }
    EXPECT(sum == rl);
    if (supported(rl)) EXPECT(w.size() == 1);
    else EXPECT(w.size() == 2 && w[0].n == rl % 8);
  }
  // Without depth 12 in the set, and past it: 12 = 4 + 8, 24 = 8 + 8 + 8.
  auto upto8 = [](int d) { return d >= 1 && d <= 8; };
  const auto w12 = replay_sub_passes(12, upto8), w24 = replay_sub_passes(24, upto8);
  EXPECT(w12.size() == 2 && w12[0].n == 4 && w12[1].n == 8 && w12[0].grow == 8);
  EXPECT(w24.size() == 3 && w24[0].n == 8 && w24[2].grow == 0);
}

// The interior and its four bands tile the owned block exactly once.
static void test_interior_split() {
  const int64_t lx = 37, ly = 53;
  for (int mask = 0; mask < 16; ++mask)
    for (int64_t band : {1, 4, 12, 20, 28}) {
      std::array<int, 4> nbr;
      for (int d = 0; d < 4; ++d) nbr[size_t(d)] = (mask >> d) & 1 ? 5 : kNoNeighbor;
      const InteriorSplit sp = interior_split(lx, ly, nbr, band);
      const Box& in = sp.interior;
      EXPECT(in.r0 == (nbr[North] >= 0 ? band : 0) && in.r1 == (nbr[South] >= 0 ? lx - band : lx));
      EXPECT(in.c0 % 4 == 0 && in.c0 >= (nbr[West] >= 0 ? band : 0) && in.c0 < band + 4);
      if (nbr[East] >= 0) EXPECT(in.c1 % 4 == 0 && in.c1 <= ly - band && in.c1 > ly - band - 4);
      else EXPECT(in.c1 == ly);
      if (nbr[West] < 0) EXPECT(in.c0 == 0);
      std::vector<unsigned char> grid(size_t(lx * ly), 0);
      auto paint = [&](const Box& b) {
        int64_t n = 0;
        for (int64_t r = b.r0; r < b.r1; ++r)
          for (int64_t cc = b.c0; cc < b.c1; ++cc) {
            EXPECT(r >= 0 && r < lx && cc >= 0 && cc < ly);
            if (r < 0 || r >= lx || cc < 0 || cc >= ly) continue;
            ++grid[size_t(r * ly + cc)];
            ++n;
          }
        return n;
      };
      const int64_t inside = paint(in);
      EXPECT(in.empty() == (inside == 0));
      if (band <= 12) EXPECT(!in.empty());
      if (in.empty()) continue;  // the schedules then do not split the pass
      for (const Box& b : sp.bands) paint(b);
      int64_t once = 0;
      for (unsigned char v : grid) once += v == 1;
      EXPECT(once == lx * ly);
    }
}

// --------------------------------------------------------------------------
// TB launch planners (heat/tb_plan.hpp)
// --------------------------------------------------------------------------
namespace tbp_test {
using namespace heat::gpu;
using tbdetail::TbBox;

// The device facts the golden lines were recorded with (MI355X, 256 CUs):
// resident waves of the streaming builds, and resident workgroups per CU of
// the per-pass tile shapes (kTileShapes' order, mixed lane shifts); the
// resident tiles' are kResidentOccGfx950.
constexpr int kSimds = 1024, kCus = 256;
int resident_waves(int depth, int variant) {
  if (depth == 12) return 2048;
  if (depth == 8) return tb_variant_split(variant) ? 2560 : 3072;
  if (depth == 7) return 3072;
  return depth == 4 ? 5120 : 3072;  // other depths: sweeps only
}
constexpr int kTileOccMixed[] = {2, 2, 2, 2, 2, 1, 1, 1, 1, 1};

std::string stream_line(int requested, int depth, const std::vector<Box>& boxes, int64_t nx,
                        int64_t pitch, const TbTuning& tune, int* resolved = nullptr) {
  const int v = tb_choose_variant(requested, depth, boxes.data(), int(boxes.size()), kSimds, tune);
  if (resolved) *resolved = v;
  if (v & tbv::kTile) return "tile";
  const TbPlan p = tb_plan_launch(v, depth, boxes.data(), int(boxes.size()), 0, nx, pitch, 0,
                                  resident_waves(depth, v), kSimds, tune);
  char line[320];
  tb_plan_trace_line(line, depth, p);
  return line;
}

std::string tile_line(int depth, const Box& box) {
  const tbw::TilePlan pl = tbw::tile_shape_search(
      &box, 1, depth, kCus, tbw::kTileShapes, [](int i) { return kTileOccMixed[i]; }, 0, 0, false);
  TbBox t{};
  const int64_t units = tbw::tile_fill_box(t, box, depth, pl, 0);
  char line[200];
  tbw::tile_trace_line(line, depth, pl, 2, 1, units, t);
  return line;
}

std::string resident_line(int depth, int passes, const Box& box) {
  const tbw::TilePlan pl =
      tbw::resident_tile_plan(box, depth, kCus, [](int i) { return tbw::kResidentOccGfx950[i]; });
  char line[200];
  tbw::resident_trace_line(line, depth, passes, pl, 0);
  return line;
}

#define EXPECT_LINE(got, want)                                                         \
  do {                                                                                 \
    const std::string g_ = (got);                                                      \
    if (g_ != (want)) {                                                                \
      std::fprintf(stderr, "FAIL %s:%d:\n  got  %s  want %s", __FILE__, __LINE__, g_.c_str(), want); \
      ++failures;                                                                      \
    }                                                                                  \
  } while (0)

// HEAT_TB_TRACE lines of the parent build on an MI355X, case by case (the
// plate, the environment and the pass are in the comments), against the pure
// planners fed the facts above.
void test_golden_plans() {
  const TbTuning def;
  const std::vector<Box> p8192{{0, 8192, 0, 8192}}, p1024{{0, 1024, 0, 8192}}, p2048{{0, 2048, 0, 4096}};
  const int64_t pitch8192 = Layout::make(8192, 8192, 12).pitch;
  // 8192^2, 1000 steps: the depth-12 passes and the depth-8 remainder.
  EXPECT_LINE(stream_line(-1, 12, p8192, 8192, pitch8192, def),
              "[heat tb] depth 12 variant 2071 boxes 1 strip_rows 294912 waves_target 2048 bpc 4 linear 0 "
              "units 2016 age_groups 2 cum 645,1024,0,0 chunk0 147 nchunks0 28 nt 1\n");
  EXPECT_LINE(stream_line(-1, 8, p8192, 8192, pitch8192, def),
              "[heat tb] depth 8 variant 2071 boxes 1 strip_rows 286720 waves_target 2048 bpc 4 linear 0 "
              "units 2030 age_groups 2 cum 645,1024,0,0 chunk0 144 nchunks0 29 nt 1\n");
  // 1024 x 8192 with HEAT_TB_TILE_MAX=0: one wave per chunk at depth 12.
  TbTuning no_tiles;
  no_tiles.tile_max_srps = 0;
  EXPECT_LINE(stream_line(-1, 12, p1024, 1024, Layout::make(1024, 8192, 12).pitch, no_tiles),
              "[heat tb] depth 12 variant 23 boxes 1 strip_rows 36864 waves_target 1024 bpc 1 linear 0 "
              "units 1008 age_groups 0 cum 0,0,0,0 chunk0 37 nchunks0 28 nt 0\n");
  // 1024 x 8192 per pass (HEAT_TB_RESIDENT=0): tiles at depth 12 and 8.
  int v = 0;
  EXPECT(stream_line(-1, 12, p1024, 1024, 0, def, &v) == "tile" && v == (tbv::kTile | tbv::kXcdGroups));
  EXPECT_LINE(tile_line(12, p1024[0]),
              "[heat tb] tile depth 12 rows 12 waves 16 bpermute 2 boxes 1 units 252 tiles0 7 len0 147\n");
  EXPECT_LINE(tile_line(8, p1024[0]),
              "[heat tb] tile depth 8 rows 12 waves 8 bpermute 2 boxes 1 units 455 tiles0 13 len0 79\n");
  EXPECT_LINE(tile_line(6, p1024[0]),
              "[heat tb] tile depth 6 rows 20 waves 8 bpermute 2 boxes 1 units 245 tiles0 7 len0 147\n");
  // An odd pass on the same block: HEAT_TB_VARIANT = kTile | kXcdGroups falls
  // back to kDefault, which is also the automatic choice.
  const char* odd =
      "[heat tb] depth 7 variant 23 boxes 1 strip_rows 35840 waves_target 1024 bpc 1 linear 0 "
      "units 1015 age_groups 0 cum 0,0,0,0 chunk0 36 nchunks0 29 nt 0\n";
  TbTuning forced_tile;
  forced_tile.variant = tbv::kTile | tbv::kXcdGroups;
  EXPECT_LINE(stream_line(-1, 7, p1024, 1024, Layout::make(1024, 8192, 12).pitch, forced_tile), odd);
  EXPECT_LINE(stream_line(-1, 7, p1024, 1024, Layout::make(1024, 8192, 7).pitch, def), odd);
  EXPECT(tb_choose_variant(tbv::kTile | tbv::kTileDpp | tbv::kAltDirection, 7, p1024.data(), 1, kSimds,
                           def) == (tbv::kDefault | tbv::kAltDirection));
  // Even depths the streaming builds lack stay on tiles whatever the size.
  EXPECT(tb_choose_variant(-1, 10, p8192.data(), 1, kSimds, def) == (tbv::kTile | tbv::kXcdGroups));
  // Resident spans: 1024 x 8192 and 2048 x 4096, depths 12, 8 and 10.
  EXPECT_LINE(resident_line(12, 82, p1024[0]),
              "[heat tb] resident depth 12 passes 82 rows 12 waves 16 xl 0 tiles 252\n");
  EXPECT_LINE(resident_line(8, 2, p1024[0]),
              "[heat tb] resident depth 8 passes 2 rows 12 waves 8 xl 0 tiles 455\n");
  EXPECT_LINE(resident_line(12, 82, p2048[0]),
              "[heat tb] resident depth 12 passes 82 rows 12 waves 16 xl 0 tiles 234\n");
  EXPECT_LINE(resident_line(8, 2, p2048[0]),
              "[heat tb] resident depth 8 passes 2 rows 12 waves 8 xl 0 tiles 468\n");
  EXPECT_LINE(resident_line(10, 10, p1024[0]),
              "[heat tb] resident depth 10 passes 10 rows 12 waves 8 xl 0 tiles 504\n");
  // HEAT_TB_VARIANT = kDefaultDeep | kLinear at 8192^2.
  TbTuning lin;
  lin.variant = tbv::kDefaultDeep | tbv::kLinear;
  EXPECT_LINE(stream_line(-1, 12, p8192, 8192, pitch8192, lin),
              "[heat tb] depth 12 variant 34839 boxes 1 strip_rows 294912 waves_target 2048 bpc 4 linear 1 "
              "units 2048 age_groups 4 cum 336,663,856,1024 chunk0 8192 nchunks0 1 nt 1\n");
  // A classic plan that fills < 9/10 of the launch: 1400 x 131072 switches by itself.
  EXPECT_LINE(stream_line(-1, 12, {{0, 1400, 0, 131072}}, 1400, Layout::make(1400, 131072, 12).pitch, def),
              "[heat tb] depth 12 variant 2071 boxes 1 strip_rows 791000 waves_target 2048 bpc 4 linear 1 "
              "units 2048 age_groups 4 cum 336,663,856,1024 chunk0 1400 nchunks0 1 nt 1\n");
  // HEAT_TB_EDGE_FRAC=0.75 at 8192^2: the box owns both plate edges.
  TbTuning edge;
  edge.edge_frac = 0.75;
  EXPECT_LINE(stream_line(-1, 12, p8192, 8192, pitch8192, edge),
              "[heat tb] depth 12 variant 2071 boxes 3 strip_rows 294912 waves_target 2048 bpc 4 linear 0 "
              "units 2016 age_groups 2 cum 645,1024,0,0 chunk0 58 nchunks0 1 nt 1\n");
  // HEAT_TB_VARIANT = kDefault | kForceAgePairs, HEAT_TB_AGE_WEIGHTS=1,1 at 4096^2.
  TbTuning even;
  even.variant = tbv::kDefault | tbv::kForceAgePairs;
  even.age_weights = {1.0, 1.0};
  EXPECT_LINE(stream_line(-1, 12, {{0, 4096, 0, 4096}}, 4096, Layout::make(4096, 4096, 12).pitch, even),
              "[heat tb] depth 12 variant 279 boxes 1 strip_rows 73728 waves_target 2048 bpc 2 linear 0 "
              "units 2016 age_groups 2 cum 512,1024,0,0 chunk0 37 nchunks0 56 nt 0\n");
  // HEAT_TB_AGE_WEIGHTS=1 at 8192^2: no age groups.
  TbTuning off;
  off.age_weights = {1.0};
  EXPECT_LINE(stream_line(-1, 12, p8192, 8192, pitch8192, off), "[heat tb] depth 12 variant 2071 boxes 1 strip_rows 294912 waves_target 2048 bpc 4 linear 0 "
              "units 2016 age_groups 0 cum 0,0,0,0 chunk0 147 nchunks0 56 nt 1\n");
  // Five boxes, as the overlap schedules make: the interior and four bands
  // of 8192^2 at depth 12, and of 4096^2 at depth 8 with kDefault.
  EXPECT_LINE(stream_line(-1, 12,
                          {{12, 8180, 12, 8180}, {0, 12, 0, 8192}, {8180, 8192, 0, 8192}, {12, 8180, 0, 12},
                           {12, 8180, 8180, 8192}},
                          8192, pitch8192, def),
              "[heat tb] depth 12 variant 2071 boxes 5 strip_rows 311248 waves_target 2048 bpc 4 linear 0 "
              "units 2044 age_groups 2 cum 645,1024,0,0 chunk0 169 nchunks0 25 nt 1\n");
  EXPECT_LINE(stream_line(tbv::kDefault, 8,
                          {{8, 4088, 8, 4088}, {0, 8, 0, 4096}, {4088, 4096, 0, 4096}, {8, 4088, 0, 8},
                           {8, 4088, 4088, 4096}},
                          4096, Layout::make(4096, 4096, 8).pitch, def),
              "[heat tb] depth 8 variant 23 boxes 5 strip_rows 77808 waves_target 2048 bpc 2 linear 0 "
              "units 2031 age_groups 0 cum 0,0,0,0 chunk0 39 nchunks0 105 nt 0\n");
}

// Units of the classic plan with chunks of L rows, restated from the
// planner's rules: per sub-box strips x chunks (x G with age groups).
int64_t classic_units(int64_t L, int64_t min_len, double edge_frac, int G, int W, int depth,
                      const std::vector<Box>& boxes, int64_t gx0, int64_t nx) {
  const int64_t edge_len = std::max<int64_t>(std::min<int64_t>(min_len, L), int64_t(double(L) * edge_frac));
  int64_t units = 0;
  auto add = [&](int64_t rows, int64_t cols, int64_t clen) {
    if (rows <= 0) return;
    const int64_t strips = ceil_div(cols, W);
    if (G == 0) {
      units += strips * ceil_div(rows, std::min(clen, rows));
    } else {
      const int64_t len = std::max<int64_t>(1, ceil_div(std::min(G * clen, rows), G));
      units += strips * ceil_div(rows, G * len) * G;
    }
  };
  for (const Box& B : boxes) {
    if (B.empty()) continue;
    int64_t r0 = B.r0, r1 = B.r1, top = 0, bot = 0;
    if (edge_len < L && B.rows() > 2 * L) {
      const int64_t top_end = 1 - gx0 + depth, bot_begin = nx - 2 - gx0 - depth;
      if (B.r0 < top_end) {
        top = std::min(B.r1, std::max(top_end, B.r0 + edge_len)) - B.r0;
        r0 += top;
      }
      if (B.r1 - 1 > bot_begin && r1 > r0) {
        bot = B.r1 - std::max(r0, std::min(bot_begin + 1, B.r1 - edge_len));
        r1 -= bot;
      }
    }
    add(top, B.cols(), edge_len);
    add(r1 - r0, B.cols(), L);
    add(bot, B.cols(), edge_len);
  }
  return units;
}

void check_plan(const TbPlan& p, int variant, int depth, const std::vector<Box>& boxes, int64_t gx0,
                int64_t nx, int waves_target, const TbTuning& tune, int* near_switch = nullptr) {
  const int W = tb_strip_width(depth, 4);
  const int G = p.age_groups > 0 ? p.age_groups : 1;
  EXPECT(((p.flags & tbdetail::kTbAgePairs) != 0) == (p.age_groups > 0));
  EXPECT(p.waves_target == waves_target && p.units == p.total_waves * G);
  if (p.age_groups > 0) {
    EXPECT(p.age_groups >= 2 && p.age_groups <= 4 && p.age_cum[0] == 0 && p.age_cum[p.age_groups] == 1024);
    for (int a = 0; a < p.age_groups; ++a) EXPECT(p.age_cum[a] < p.age_cum[a + 1]);
  }
  int64_t total_rows = 0;
  for (const Box& B : boxes)
    if (!B.empty()) total_rows += ceil_div(B.cols(), W) * B.rows();
  EXPECT(p.total_strip_rows == total_rows);
  // The classic plan first, restated: the shrink loop stays within
  // waves_target unless eight steps of its recurrence do not get there.
  const bool is_linear = (p.flags & tbdetail::kTbLinear) != 0;
  const int64_t min_len = tune.min_len > 0 ? tune.min_len : std::max(depth, 8);
  // Linear plans of split pipelines may regroup (kTbLinearAgeWeights): their classic plan had two.
  const int Gc = is_linear && p.age_groups == 4 && tune.age_weights.empty() ? 2 : p.age_groups;
  int64_t len = std::max(min_len, ceil_div(total_rows, int64_t(waves_target)));
  int64_t units = classic_units(len, min_len, tune.edge_frac, Gc, W, depth, boxes, gx0, nx);
  int64_t max_rows = 1;  // a longer chunk length plans the same
  for (const Box& B : boxes) max_rows = std::max(max_rows, B.rows());
  for (int it = 0; it < 8 && units > waves_target; ++it) {
    len = std::min(max_rows, std::max(len + 1, ceil_div(len * units, int64_t(waves_target))));
    units = classic_units(len, min_len, tune.edge_frac, Gc, W, depth, boxes, gx0, nx);
  }
  // The linear switch: forced, or a classic plan that fills < 9/10 of a large launch.
  const bool large = total_rows >= 32 * int64_t(depth) * waves_target;
  EXPECT(is_linear == ((variant & tbv::kLinear) ||
                       (!(variant & tbv::kNoLinear) && units < 9 * int64_t(waves_target) / 10 && large)));
  if (near_switch && !(variant & (tbv::kLinear | tbv::kNoLinear)) && large &&
      units >= 9 * int64_t(waves_target) / 10 && units < waves_target)
    ++*near_switch;
  if (p.flags & tbdetail::kTbLinear) {
    int b = 0;
    int64_t lin = 0;
    for (const Box& B : boxes) {
      if (B.empty()) continue;
      const TbBox& t = p.box[b++];
      EXPECT(t.r0 == B.r0 && t.r1 == B.r1 && t.c0 == B.c0 && t.c1 == B.c1);
      EXPECT(t.nstrips == ceil_div(B.cols(), W) && t.lin0 == lin && t.nchunks == 1 && t.wave_begin == 0);
      lin += int64_t(t.nstrips) * B.rows();
    }
    EXPECT(b == p.nbox && p.lin_total == lin && p.lin_slack == 2 * depth);
    EXPECT(p.units % G == 0 && p.units >= G && p.units <= std::max(waves_target, G));
    return;
  }
  // Classic: the sub-boxes of a box partition its rows in plate order.
  int b = 0, begin = 0;
  for (const Box& B : boxes) {
    if (B.empty()) continue;
    int64_t r = B.r0;
    while (r < B.r1 && b < p.nbox) {
      const TbBox& t = p.box[b++];
      EXPECT(t.r0 == r && t.r1 > t.r0 && t.r1 <= B.r1 && t.c0 == B.c0 && t.c1 == B.c1);
      const int64_t rows = t.r1 - t.r0;
      EXPECT(t.nstrips == ceil_div(B.cols(), W) && t.chunk_len >= 1);
      EXPECT(int64_t(t.nchunks - 1) * G * t.chunk_len < rows && rows <= int64_t(t.nchunks) * G * t.chunk_len);
      EXPECT(t.wave_begin == begin);
      begin += t.nstrips * t.nchunks;
      r = t.r1;
    }
    EXPECT(r == B.r1);
  }
  EXPECT(b == p.nbox && p.total_waves == begin);
  EXPECT(p.units == units);
}

void test_plan_sweep() {
  // Box sets with c0 % 4 == 0: one to five boxes, plate edges owned or not.
  const std::vector<std::vector<Box>> sets = {
      {{0, 8192, 0, 8192}},
      {{0, 1000, 0, 777}},
      {{-12, 2060, -12, 4108}},
      {{0, 37, 0, 5000}, {37, 3000, 0, 5000}},
      {{0, 700, 4, 3001}, {0, 0, 0, 8}, {700, 701, 0, 3001}},
      {{16, 4080, 16, 4080}, {0, 16, 0, 4096}, {4080, 4096, 0, 4096}, {16, 4080, 0, 16}},
      {{12, 8180, 12, 8180}, {0, 12, 0, 8192}, {8180, 8192, 0, 8192}, {12, 8180, 0, 12}, {12, 8180, 8180, 8192}},
      {{0, 1400, 0, 131072}},
      {{0, 131072, 0, 131072}},
  };
  const int variants[] = {tbv::kDefault, tbv::kDefaultDeep, tbv::kDefault | tbv::kForceAgePairs,
                          tbv::kDefaultDeep | tbv::kLinear, tbv::kDefaultDeep | tbv::kNoLinear,
                          tbv::kDefault | tbv::kNoAgePairs};
  int plans = 0, linear = 0, over = 0, grouped = 0, edged = 0, near_switch = 0;
  for (const auto& boxes : sets)
    for (int depth : {1, 2, 3, 4, 5, 6, 7, 8, 12})
      for (int variant : variants)
        for (int wt : {0, -1, -2, 64, 100, 333, 1000, 2048, 4096})
          for (int min_len : {0, 4, 64})
            for (double edge_frac : {1.0, 0.75, 0.3})
              for (int w = 0; w < 3; ++w) {
                if (tb_variant_split(variant) && depth != 8 && depth != 12) continue;
                TbTuning tune;
                tune.min_len = min_len;
                tune.edge_frac = edge_frac;
                if (w == 1) tune.age_weights = {3.0, 2.0, 1.0};
                if (w == 2) tune.age_weights = {1.0};
                const int64_t nx = boxes[0].r1 + (boxes.size() == 1 && boxes[0].r0 < 0 ? 500 : 0);
                const int resident = resident_waves(depth, variant);
                const TbPlan p = tb_plan_launch(variant, depth, boxes.data(), int(boxes.size()), 0, nx,
                                                8192, wt, resident, kSimds, tune);
                int target = wt;
                if (wt < 0) target = -wt * resident;
                if (wt == 0) target = p.waves_target;  // from the work per SIMD: checked by the goldens
                EXPECT(p.nbox > 0 && p.variant == variant);
                check_plan(p, variant, depth, boxes, 0, nx, target, tune, &near_switch);
                ++plans;
                linear += (p.flags & tbdetail::kTbLinear) != 0;
                over += p.units > p.waves_target;
                grouped += p.age_groups > 0;
                edged += p.nbox > int(boxes.size());
              }
  // The sweep reaches every path, and plans on both sides of the linear switch.
  EXPECT(plans > 10000 && linear > 100 && over > 10 && grouped > 1000 && edged > 100);
  EXPECT(near_switch > 100);
  if (failures) std::fprintf(stderr, "sweep: %d plans, %d linear, %d over target, %d grouped, %d with edge sub-boxes, %d near the switch\n", plans, linear, over, grouped, edged, near_switch);
  // No boxes, or only empty ones: nothing to launch.
  const Box none[2] = {{0, 0, 0, 8}, {4, 4, 0, 0}};
  EXPECT(tb_plan_launch(tbv::kDefault, 8, none, 2, 0, 100, 512, 0, 3072, kSimds, TbTuning{}).nbox == 0);
  EXPECT(tb_plan_launch(tbv::kDefault | tbv::kLinear, 8, none, 0, 0, 100, 512, 0, 3072, kSimds,
                        TbTuning{}).nbox == 0);
}

// resident_shape_static as it stood before the shared search, restated.
int naive_resident_shape(const Box& box, int depth, int cus) {
  static constexpr int kShapes[][3] = {{12, 8, 2}, {13, 8, 2}, {14, 8, 2}, {16, 8, 2},
                                       {20, 8, 1}, {24, 8, 1}, {12, 16, 1}, {20, 16, 1}};
  if (box.empty() || depth < 4 || depth % 2 != 0 || box.c0 % 4 != 0) return 0;
  const int64_t W = 256 - 2 * round_up(int64_t(depth), 4);
  auto estimate = [&](int64_t units, int occ, int rows, int waves) {
    const int64_t cap = int64_t(cus) * occ, full = (units - 1) / cap;
    const int64_t busiest = (units - full * cap + cus - 1) / cus;
    auto cost = [&](int64_t tiles) {
      const double wps = double(tiles * waves) / 4.0;
      return wps * rows * (wps >= 4.0 ? 2.7 : 3.1);
    };
    return double(full) * cost(occ) + cost(busiest);
  };
  int best = 0;
  double best_est = 0.0;
  int64_t best_hmax = 0;
  for (const auto& s : kShapes) {
    const int64_t hmax = int64_t(s[0]) * s[1] - 2 * int64_t(depth);
    if (hmax < std::max(depth, 4)) continue;
    const int64_t units = ceil_div(box.cols(), W) * ceil_div(box.rows(), hmax);
    if (units > int64_t(cus) * s[2]) continue;
    const double est = estimate(units, s[2], s[0], s[1]);
    if (best == 0 || est < best_est) {
      best = res_shape(s[0], s[1]);
      best_est = est;
      best_hmax = hmax;
    }
  }
  if (best != 0 && ceil_div(box.rows(), ceil_div(box.rows(), best_hmax)) < depth) return 0;
  return best;
}

void test_tile_search() {
  auto occ = [](int i) { return tbw::kResidentOccGfx950[i]; };
  int shapes_seen = 0, none = 0, differ = 0;
  for (int depth : {2, 4, 6, 7, 8, 10, 12, 16}) {
    // Every row count (every hmax boundary of every shape) against columns
    // around every strip boundary.
    const int W = tb_strip_width(depth, 4);
    std::vector<int64_t> cols;
    for (int64_t c = W; c <= 5000 + W; c += W)
      for (int64_t d = -1; d <= 1; ++d)
        if (c + d >= 1 && c + d <= 5000) cols.push_back(c + d);
    cols.push_back(1);
    cols.push_back(5000);
    for (int64_t rows = 1; rows <= 5000; ++rows)
      for (int64_t c : cols) {
        const Box box{0, rows, 0, c};
        const int want = naive_resident_shape(box, depth, kCus);
        EXPECT(resident_shape_static(box, depth, kCus) == want);
        shapes_seen += want != 0;
        none += want == 0;
        if (depth < 4 || depth % 2 != 0 || c % 7 != 0) continue;
        // One dispatch round is the only difference between the tile and the
        // resident answer on the common shapes.
        const tbw::TilePlan any = tbw::tile_shape_search(&box, 1, depth, kCus, tbw::kResidentShapes, occ, 0, 0, false);
        const tbw::TilePlan one = tbw::tile_shape_search(&box, 1, depth, kCus, tbw::kResidentShapes, occ, 0, 0, true);
        int occ_any = 0;
        for (int i = 0; i < 8; ++i)
          if (tbw::kResidentShapes[i].rows == any.rows && tbw::kResidentShapes[i].waves == any.waves) occ_any = occ(i);
        if (any.units <= int64_t(kCus) * occ_any)
          EXPECT(one.rows == any.rows && one.waves == any.waves && one.units == any.units);
        else
          EXPECT(one.rows == 0 || (one.est >= any.est && (one.rows != any.rows || one.waves != any.waves)));
        differ += one.rows != any.rows || one.waves != any.waves;
      }
  }
  EXPECT(shapes_seen > 100000 && none > 100000 && differ > 100);
  EXPECT(resident_shape_static(Box{0, 1024, 2, 8192}, 12) == 0);  // c0 % 4
  // The tuning's filters: that value only.
  const Box b{0, 1024, 0, 8192};
  const tbw::TilePlan f = tbw::tile_shape_search(&b, 1, 12, kCus, tbw::kTileShapes,
                                                 [](int i) { return kTileOccMixed[i]; }, 20, 16, false);
  EXPECT(f.rows == 20 && f.waves == 16);
  EXPECT(tbw::tile_shape_search(&b, 1, 12, kCus, tbw::kTileShapes, [](int) { return 0; }, 0, 0, false).rows == 0);
}
}  // namespace tbp_test

int main() {
  tbp_test::test_golden_plans();
  tbp_test::test_plan_sweep();
  tbp_test::test_tile_search();
  test_span_box_literals();
  test_pass_geometry_sweep();
  test_sub_passes();
  test_interior_split();
  test_dims();
  test_blocks();
  test_format();
  test_init_wrap();
  test_cpu_step_and_halo_invariance();
  if (failures) {
    std::fprintf(stderr, "selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("selftest: ok\n");
  return 0;
}
