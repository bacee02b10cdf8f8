// Host-only self-test of the refinement (heat::refine_axis and the host twin
// heat::refine_block, io.hpp): stand-alone, so that it also runs under
// ASan/UBSan (make refine-selftest-asan).  No GPU, no Python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "heat/common.hpp"
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

struct Axis {
  std::vector<int32_t> i0, i1;
  std::vector<float> w;
  Axis(int64_t n, int64_t f, int order, bool wrap, int64_t begin, int64_t count)
      : i0(size_t(count)), i1(size_t(count)), w(size_t(count)) {
    heat::refine_axis(n, f, order, wrap, begin, count, i0.data(), i1.data(), w.data());
  }
  heat::RefineTable table() const { return heat::RefineTable{i0.data(), i1.data(), w.data()}; }
};

// The definition, index by index, with a linear search for k.
void slow_entry(int64_t n, int64_t f, int order, bool wrap, int64_t i, int32_t* a, int32_t* b,
                float* w) {
  const int64_t C = (n + f - 1) / f;
  auto c2 = [&](int64_t I) { return I * f + (((I + 1) * f < n) ? (I + 1) * f : n) - 1; };
  *w = 0.f;
  if (order == 0) {
    *a = *b = int32_t(i / f);
    return;
  }
  const int64_t t = 2 * i;
  int64_t k = -1;
  for (int64_t I = 0; I < C; ++I)
    if (c2(I) <= t) k = I;
  if (k >= 0 && k < C - 1) {
    *a = int32_t(k);
    *b = int32_t(k + 1);
    *w = float(double(t - c2(k)) / double(c2(k + 1) - c2(k)));
  } else if (!wrap || C == 1) {
    *a = *b = int32_t(k < 0 ? 0 : C - 1);
  } else {
    *a = int32_t(C - 1);
    *b = 0;
    *w = float(double(t - c2(C - 1) + (k < 0 ? 2 * n : 0)) / double(c2(0) + 2 * n - c2(C - 1)));
  }
}

void test_axis() {
  {  // the documented example: n = 10, f = 4, order 1
    const Axis a(10, 4, 1, false, 0, 10);
    const int32_t e0[10] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 2}, e1[10] = {0, 0, 1, 1, 1, 1, 2, 2, 2, 2};
    const float ew[10] = {0.f,    0.f,         .125f, .375f,       .625f,
                          .875f, float(1. / 6), .5f,   float(5. / 6), 0.f};
    for (int i = 0; i < 10; ++i)
      CHECK(a.i0[size_t(i)] == e0[i] && a.i1[size_t(i)] == e1[i] &&
                bits(a.w[size_t(i)]) == bits(ew[i]),
            "example entry %d", i);
    const Axis p(10, 4, 1, true, 0, 10);
    CHECK(p.i0[0] == 2 && p.i1[0] == 0 && p.w[0] == .5f, "wrap entry 0");
    CHECK(p.i0[1] == 2 && p.i1[1] == 0 && bits(p.w[1]) == bits(float(5. / 6)), "wrap entry 1");
    CHECK(p.i0[9] == 2 && p.i1[9] == 0 && bits(p.w[9]) == bits(float(1. / 6)), "wrap entry 9");
  }
  const int64_t factors[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 64};
  for (int64_t n = 1; n <= 40; ++n)
    for (int64_t f : factors)
      for (int order = 0; order < 2; ++order)
        for (int wrap = 0; wrap < 2; ++wrap) {
          const Axis a(n, f, order, wrap != 0, 0, n);
          const int64_t C = (n + f - 1) / f;
          for (int64_t i = 0; i < n; ++i) {
            int32_t s0, s1;
            float sw;
            slow_entry(n, f, order, wrap != 0, i, &s0, &s1, &sw);
            const size_t q = size_t(i);
            CHECK(a.i0[q] == s0 && a.i1[q] == s1 && bits(a.w[q]) == bits(sw),
                  "n %lld f %lld order %d wrap %d i %lld", (long long)n, (long long)f, order, wrap,
                  (long long)i);
            CHECK(a.i0[q] >= 0 && a.i0[q] < C && a.i1[q] >= 0 && a.i1[q] < C, "index range");
            CHECK(a.w[q] >= 0.f && a.w[q] < 1.f && (a.i0[q] != a.i1[q] || a.w[q] == 0.f),
                  "weight n %lld f %lld i %lld", (long long)n, (long long)f, (long long)i);
          }
          // A sub-range is the same entries.
          if (n >= 3) {
            const Axis s(n, f, order, wrap != 0, 1, n - 2);
            for (int64_t i = 0; i < n - 2; ++i)
              CHECK(s.i0[size_t(i)] == a.i0[size_t(i + 1)] && s.i1[size_t(i)] == a.i1[size_t(i + 1)] &&
                        bits(s.w[size_t(i)]) == bits(a.w[size_t(i + 1)]),
                    "sub-range");
          }
        }
}

float lerp(float a, float b, float w) { return w == 0.f ? a : std::fmaf(w, b - a, a); }

void test_block(int64_t nx, int64_t ny, int64_t fx, int64_t fy, int order, int wrap) {
  int64_t cr = 0, cc = 0;
  heat::coarse_dims(nx, ny, fx, fy, &cr, &cc);
  heat::refine_check(nx, ny, cr, cc, fx, fy, order);
  std::vector<float> S(size_t(cr * cc));
  uint32_t seed = uint32_t(nx * 131 + ny * 17 + fx * 7 + fy);
  for (auto& v : S) {
    seed = seed * 1664525u + 1013904223u;
    v = float(int32_t(seed >> 8) % 4096 - 2048) * 0.25f;
  }
  if (S.size() > 2) {
    S[1] = std::numeric_limits<float>::infinity();
    uint32_t payload = 0x7fc12345u;  // a NaN with a payload
    std::memcpy(&S[2], &payload, 4);
  }
  const Axis rows(nx, fx, order, (wrap & 1) != 0, 0, nx), cols(ny, fy, order, (wrap & 2) != 0, 0, ny);
  // The whole plate inside a NaN-free sentinel frame (ring 2, pitch ny + 7).
  const int64_t pitch = ny + 7, H = 2;
  const float kSent = -12345.f;
  std::vector<float> buf(size_t((nx + 2 * H) * pitch), kSent);
  float* origin = buf.data() + H * pitch + H;
  heat::refine_block(origin, pitch, nx, ny, S.data(), cc, rows.table(), cols.table());
  for (int64_t r = 0; r < nx + 2 * H; ++r)
    for (int64_t c = 0; c < pitch; ++c) {
      const bool owned = r >= H && r < H + nx && c >= H && c < H + ny;
      const float got = buf[size_t(r * pitch + c)];
      if (!owned) {
        CHECK(bits(got) == bits(kSent), "frame cell (%lld, %lld) written", (long long)r, (long long)c);
        continue;
      }
      const size_t i = size_t(r - H), j = size_t(c - H);
      const float* sa = S.data() + int64_t(rows.i0[i]) * cc;
      const float* sb = S.data() + int64_t(rows.i1[i]) * cc;
      const float top = lerp(sa[cols.i0[j]], sa[cols.i1[j]], cols.w[j]);
      const float bot = lerp(sb[cols.i0[j]], sb[cols.i1[j]], cols.w[j]);
      const float want = lerp(top, bot, rows.w[i]);
      const bool same = bits(got) == bits(want) || (got != got && want != want);
      CHECK(same, "cell (%zu, %zu) of %lldx%lld f %lldx%lld order %d wrap %d", i, j, (long long)nx,
            (long long)ny, (long long)fx, (long long)fy, order, wrap);
      if (order == 0)
        CHECK(bits(got) == bits(S[size_t((int64_t(i) / fx) * cc + int64_t(j) / fy)]), "order 0 copy");
    }
  // Blocks refined at their offsets are the same cells.
  const int64_t ox = nx / 3, oy = ny / 2, lx = nx - ox, ly = ny - oy;
  const Axis br(nx, fx, order, (wrap & 1) != 0, ox, lx), bc(ny, fy, order, (wrap & 2) != 0, oy, ly);
  std::vector<float> blk(size_t(lx * ly), kSent);
  heat::refine_block(blk.data(), ly, lx, ly, S.data(), cc, br.table(), bc.table());
  for (int64_t r = 0; r < lx; ++r)
    for (int64_t c = 0; c < ly; ++c) {
      const float a = blk[size_t(r * ly + c)], b = origin[(ox + r) * pitch + oy + c];
      CHECK(bits(a) == bits(b) || (a != a && b != b), "block cell (%lld, %lld)", (long long)r, (long long)c);
    }
}

void test_refusals() {
  bool threw = false;
  try {
    heat::refine_check(70, 519, 18, 65, 5, 8, 1);
  } catch (const std::exception& e) {
    threw = std::strstr(e.what(), "18x65") && std::strstr(e.what(), "5x8") &&
            std::strstr(e.what(), "70x519") && std::strstr(e.what(), "14x65");
  }
  CHECK(threw, "refine_check names the numbers");
  threw = false;
  try {
    heat::refine_check(70, 519, 18, 65, 4, 8, 2);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "refine_check refuses order 2");
}

}  // namespace

int main() {
  test_axis();
  const int64_t cases[][4] = {{37, 53, 4, 8}, {9, 519, 1, 3}, {130, 70, 64, 300}, {5, 5, 7, 2},
                              {64, 256, 8, 8}, {1, 1, 1, 1}};
  for (const auto& c : cases)
    for (int order = 0; order < 2; ++order)
      for (int wrap = 0; wrap < 4; ++wrap) test_block(c[0], c[1], c[2], c[3], order, wrap);
  test_refusals();
  if (g_fail) {
    std::printf("refine selftest: %d FAILED\n", g_fail);
    return 1;
  }
  std::printf("refine selftest: ok\n");
  return 0;
}
