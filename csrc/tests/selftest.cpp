// Host-only self-test of the native engine's CPU components (topology,
// decomposition, layouts, pass boxes and ghost bookkeeping, prtdat formatting,
// initial condition, CPU stencil, deep-halo invariance).  Built twice: plain
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

int main() {
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
