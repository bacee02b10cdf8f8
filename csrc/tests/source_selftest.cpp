// Host-only self-test of the heat source: the host twin of the source step
// (heat::cpu::step_source, cpu_backend.hpp) and the extended-table builder that
// gives the source field its ghost cells (heat::ghost_axis_index /
// refine_axis_ext, io.hpp).  Stand-alone, so that it also runs under
// ASan/UBSan (make source-selftest-asan).  No GPU, no Python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "heat/common.hpp"
#include "heat/cpu_backend.hpp"
#include "heat/init_fn.hpp"
#include "heat/io.hpp"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);    \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

float value(uint64_t k) {  // signed, magnitudes 2^-20 .. 2^20
  const uint64_t h = heat::mix64(k);
  const float m = float(h >> 40) * (1.0f / 16777216.0f) + 0.5f;
  return std::ldexp((h & 1) ? -m : m, int((h >> 1) % 41) - 20);
}

// A field of exactly (lx + 2) x (ly + 2) floats: any access beyond the 1-cell
// frame of the block is out of the allocation (ASan).
struct Tight {
  int64_t lx, ly, pitch;
  std::vector<float> v;
  Tight(int64_t lx_, int64_t ly_, float fill)
      : lx(lx_), ly(ly_), pitch(ly_ + 2), v(size_t((lx_ + 2) * (ly_ + 2)), fill) {}
  float* origin() { return v.data() + pitch + 1; }
  float& at(int64_t r, int64_t c) { return origin()[r * pitch + c]; }
};

void test_step(int64_t nx, int64_t ny, int64_t gx0, int64_t gy0, int64_t lx, int64_t ly,
               heat::Box box, float cx, float cy) {
  const float nan = std::numeric_limits<float>::quiet_NaN(), sentinel = -777.25f;
  Tight src(lx, ly, nan), dst(lx, ly, sentinel), q(lx, ly, nan), plain(lx, ly, sentinel);
  for (int64_t r = -1; r <= lx; ++r)
    for (int64_t c = -1; c <= ly; ++c) {
      const int64_t gx = gx0 + r, gy = gy0 + c;
      if (gx >= 0 && gx < nx && gy >= 0 && gy < ny) src.at(r, c) = value(uint64_t(gx * ny + gy));
    }
  for (int64_t r = box.r0; r < box.r1; ++r)
    for (int64_t c = box.c0; c < box.c1; ++c) q.at(r, c) = value(uint64_t(7919 + r * ly + c));
  heat::cpu::Geom g;
  g.pitch = src.pitch;
  g.gx0 = gx0;
  g.gy0 = gy0;
  g.nx = nx;
  g.ny = ny;
  g.cx = cx;
  g.cy = cy;
  const float res = heat::cpu::step_source(src.origin(), dst.origin(), q.origin(), g, box, true);
  heat::cpu::step(src.origin(), plain.origin(), g, box, false);
  float want_res = 0.f;
  for (int64_t r = -1; r <= lx; ++r)
    for (int64_t c = -1; c <= ly; ++c) {
      const bool in = r >= box.r0 && r < box.r1 && c >= box.c0 && c < box.c1;
      if (!in) {
        CHECK(bits(dst.at(r, c)) == bits(sentinel), "cell (%lld, %lld) outside the box written",
              (long long)r, (long long)c);
        continue;
      }
      const int64_t gx = gx0 + r, gy = gy0 + c;
      const bool upd = gx >= 1 && gx <= nx - 2 && gy >= 1 && gy <= ny - 2;
      // The plain step's value plus q in one rounded add; a fixed cell keeps its value.
      volatile float sum = plain.at(r, c) + q.at(r, c);
      const float want = upd ? float(sum) : src.at(r, c);
      CHECK(bits(dst.at(r, c)) == bits(want), "cell (%lld, %lld): %a != %a", (long long)r,
            (long long)c, double(dst.at(r, c)), double(want));
      if (upd) want_res = std::fmax(want_res, std::fabs(want - src.at(r, c)));
    }
  CHECK(bits(res) == bits(want_res), "residual %a != %a", double(res), double(want_res));
}

void test_steps() {
  const float coef[2][2] = {{0.05f, 0.2f}, {0.1f, 0.1f}};
  for (const auto& k : coef) {
    // Whole plates (no or one interior cell, wider ones), the block is the plate.
    const int64_t plates[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 2}, {3, 3}, {13, 37}, {70, 21}};
    for (const auto& p : plates)
      test_step(p[0], p[1], 0, 0, p[0], p[1], heat::Box{0, p[0], 0, p[1]}, k[0], k[1]);
    // Blocks inside a plate, 1, 2, 3 and 5 columns from its east edge, and a sub-box.
    for (int64_t d : {1, 2, 3, 5})
      test_step(30, 40, 7, 40 - d - 11, 12, 11, heat::Box{0, 12, 0, 11}, k[0], k[1]);
    test_step(30, 40, 0, 0, 30, 40, heat::Box{3, 17, 5, 22}, k[0], k[1]);
  }
  // q = +0: the plain step, except that a -0 result becomes +0.
  {
    Tight src(3, 3, 0.f), dst(3, 3, 1.f), q(3, 3, 0.f);
    // A -0 result: c = -0 and neighbour sums so small and negative that both
    // products underflow to -0 (0.1 * 2^-149 is below half an ulp of zero).
    for (auto& x : src.v) x = -0.f;
    src.at(0, 1) = src.at(1, 2) = -std::numeric_limits<float>::denorm_min();
    heat::cpu::Geom g;
    g.pitch = src.pitch;
    g.nx = g.ny = 3;
    heat::cpu::step(src.origin(), dst.origin(), g, heat::Box{0, 3, 0, 3}, false);
    CHECK(bits(dst.at(1, 1)) == bits(-0.f), "plain step of an all -0 field: %a",
          double(dst.at(1, 1)));
    heat::cpu::step_source(src.origin(), dst.origin(), q.origin(), g, heat::Box{0, 3, 0, 3}, false);
    CHECK(bits(dst.at(1, 1)) == bits(0.f), "source step with q = +0 of an all -0 field: %a",
          double(dst.at(1, 1)));
    CHECK(bits(dst.at(0, 0)) == bits(-0.f), "a fixed cell keeps its -0");
  }
  // A NaN in q inside the box makes the residual NaN; outside it does not.
  {
    Tight src(5, 5, 1.f), dst(5, 5, 0.f), q(5, 5, 0.f);
    heat::cpu::Geom g;
    g.pitch = src.pitch;
    g.nx = g.ny = 5;
    q.at(1, 3) = std::numeric_limits<float>::quiet_NaN();
    float r = heat::cpu::step_source(src.origin(), dst.origin(), q.origin(), g,
                                     heat::Box{1, 4, 1, 3}, true);
    CHECK(r == 0.f, "NaN next to the box: residual %a", double(r));
    r = heat::cpu::step_source(src.origin(), dst.origin(), q.origin(), g, heat::Box{1, 4, 1, 4},
                               true);
    CHECK(std::isnan(r), "NaN in the box: residual %a", double(r));
  }
}

void test_ghost_index() {
  // identity, wrap (several periods out), mirrors, clamp
  for (int64_t n : {1, 2, 5, 9})
    for (int64_t i = -3 * n - 2; i < 4 * n + 2; ++i) {
      const int64_t w = heat::ghost_axis_index(i, n, true, false, false);
      CHECK(w >= 0 && w < n && (w - i) % n == 0, "wrap %lld of %lld -> %lld", (long long)i,
            (long long)n, (long long)w);
      const int64_t c = heat::ghost_axis_index(i, n, false, false, false);
      CHECK(c == (i < 0 ? 0 : i >= n ? n - 1 : i), "clamp %lld of %lld -> %lld", (long long)i,
            (long long)n, (long long)c);
    }
  const int64_t n = 9;
  for (int64_t d = 1; d < n; ++d) {
    CHECK(heat::ghost_axis_index(-d, n, false, true, false) == d, "mirror lo %lld", (long long)d);
    CHECK(heat::ghost_axis_index(-d, n, false, false, true) == 0, "fixed lo %lld", (long long)d);
    CHECK(heat::ghost_axis_index(n - 1 + d, n, false, false, true) == n - 1 - d, "mirror hi %lld",
          (long long)d);
    CHECK(heat::ghost_axis_index(n - 1 + d, n, false, true, false) == n - 1, "fixed hi %lld",
          (long long)d);
  }
}

void test_axis_ext() {
  // Entry q of the extended table is the plate table's entry at the mapped index.
  struct Mode { bool wrap, lo, hi; };
  const Mode modes[] = {{false, false, false}, {true, false, false}, {false, true, false},
                        {false, false, true}, {false, true, true}};
  for (int64_t n : {9, 37})
    for (int64_t f : {1, 4, 5})
      for (int order : {0, 1})
        for (const Mode& m : modes) {
          std::vector<int32_t> p0(size_t(n), 0), p1(size_t(n), 0);
          std::vector<float> pw(size_t(n), 0.f);
          heat::refine_axis(n, f, order, m.wrap, 0, n, p0.data(), p1.data(), pw.data());
          const int64_t H = 8, begin = 3 - H, count = n - 3 + 2 * H;  // a block [3, n) plus H each side
          std::vector<int32_t> e0(size_t(count), -1), e1(size_t(count), -1);
          std::vector<float> ew(size_t(count), -1.f);
          heat::refine_axis_ext(n, f, order, m.wrap, m.lo, m.hi, begin, count, e0.data(),
                                e1.data(), ew.data());
          for (int64_t k = 0; k < count; ++k) {
            const size_t j = size_t(heat::ghost_axis_index(begin + k, n, m.wrap, m.lo, m.hi));
            CHECK(e0[size_t(k)] == p0[j] && e1[size_t(k)] == p1[j] &&
                      bits(ew[size_t(k)]) == bits(pw[j]),
                  "n %lld f %lld order %d: entry %lld", (long long)n, (long long)f, order,
                  (long long)(begin + k));
          }
        }
  // The extended block of a refined field: ghost cells equal the plate cells they stand for.
  const int64_t nx = 11, ny = 13, fx = 4, fy = 3, H = 3;
  const int64_t cr = (nx + fx - 1) / fx, cc = (ny + fy - 1) / fy;
  std::vector<float> S(size_t(cr * cc));
  for (size_t k = 0; k < S.size(); ++k) S[k] = value(k + 100);
  auto fill = [&](int64_t ox, int64_t lx, int64_t oy, int64_t ly, int64_t h, bool wx, bool mn,
                  bool ms, bool wy, bool mw, bool me, std::vector<float>& out) {
    const int64_t ex = lx + 2 * h, ey = ly + 2 * h;
    std::vector<int32_t> i0(size_t(ex + ey)), i1(size_t(ex + ey));
    std::vector<float> w(size_t(ex + ey));
    heat::refine_axis_ext(nx, fx, 1, wx, mn, ms, ox - h, ex, i0.data(), i1.data(), w.data());
    heat::refine_axis_ext(ny, fy, 1, wy, mw, me, oy - h, ey, i0.data() + ex, i1.data() + ex,
                          w.data() + ex);
    out.assign(size_t(ex * ey), 0.f);
    heat::refine_block(out.data(), ey, ex, ey, S.data(), cc,
                       heat::RefineTable{i0.data(), i1.data(), w.data()},
                       heat::RefineTable{i0.data() + ex, i1.data() + ex, w.data() + ex});
  };
  std::vector<float> plate, ext;
  // wrap x, mirror west, fixed east: a block in the plate's north-west corner.
  fill(0, nx, 0, ny, 0, true, false, false, false, true, false, plate);
  fill(0, 5, 0, 6, H, true, false, false, false, true, false, ext);
  const int64_t ey = 6 + 2 * H;
  for (int64_t r = -H; r < 5 + H; ++r)
    for (int64_t c = -H; c < 6 + H; ++c) {
      const int64_t pr = heat::ghost_axis_index(r, nx, true, false, false);
      const int64_t pc = heat::ghost_axis_index(c, ny, false, true, false);
      CHECK(bits(ext[size_t((r + H) * ey + c + H)]) == bits(plate[size_t(pr * ny + pc)]),
            "extended block cell (%lld, %lld)", (long long)r, (long long)c);
    }
}

}  // namespace

int main() {
  test_steps();
  test_ghost_index();
  test_axis_ext();
  if (g_fail) {
    std::printf("source selftest: %d FAILED\n", g_fail);
    return 1;
  }
  std::printf("source selftest: ok\n");
  return 0;
}
