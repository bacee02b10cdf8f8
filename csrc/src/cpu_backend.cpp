// CPU reference backend (see cpu_backend.hpp).
#include "heat/cpu_backend.hpp"

#include <omp.h>

#include <cmath>
#include <cstring>

#include "heat/common.hpp"
#include "heat/init_fn.hpp"

namespace heat::cpu {

void set_threads(int n) {
  if (n > 0) omp_set_num_threads(n);
}
int get_threads() { return omp_get_max_threads(); }

void init_field(float* origin, const Layout& L, int64_t gx0, int64_t gy0, int64_t nx, int64_t ny,
                int mode, uint64_t seed) {
  float* base = origin - L.origin();
#pragma omp parallel for schedule(static)
  for (int64_t r = 0; r < L.rows; ++r)
    for (int64_t c = 0; c < L.pitch; ++c)
      base[r * L.pitch + c] = init_value(mode, gx0 + r - L.hx, gy0 + c - L.hy, nx, ny, seed);
}

static inline bool interior(int64_t g, int64_t n) { return g >= 1 && g <= n - 2; }

namespace {
// Q: the step adds the source q (same layout) to every cell it updates.
template <bool Q>
float step_impl(const float* src, float* dst, const float* q, const Geom& g, const Box& box,
                bool want_resid) {
  if (box.empty()) return 0.0f;
  uint32_t mbits = 0;
  // Only the global-interior part of each row is updated; boundary cells are
  // copied so dst holds a complete field for the box.
  const int64_t cl = std::max(box.c0, 1 - g.gy0), ch = std::min(box.c1, g.ny - 1 - g.gy0);
#pragma omp parallel for schedule(static) reduction(max : mbits)
  for (int64_t r = box.r0; r < box.r1; ++r) {
    const float* s = src + r * g.pitch;
    float* d = dst + r * g.pitch;
    if (!interior(g.gx0 + r, g.nx) || cl >= ch) {
      std::memcpy(d + box.c0, s + box.c0, size_t(box.cols()) * 4);
      continue;
    }
    const float* n = s - g.pitch;
    const float* so = s + g.pitch;
    for (int64_t c = box.c0; c < cl; ++c) d[c] = s[c];
    uint32_t rm = 0;
    auto row = [&](auto update) {
      for (int64_t c = cl; c < ch; ++c) {
        float v = update(s[c], n[c], so[c], s[c - 1], s[c + 1], g.cx, g.cy);
        if constexpr (Q) v = v + q[r * g.pitch + c];  // one rounded add, nothing fused into it
        d[c] = v;
        if (want_resid) {
          float diff = std::fabs(v - s[c]);
          uint32_t bits;
          std::memcpy(&bits, &diff, 4);
          rm = bits > rm ? bits : rm;
        }
      }
    };
    if (g.numerics == 1)
      row([](float c, float n, float s, float w, float e, float cx, float cy) {
        return stencil_mpi(c, n, s, w, e, cx, cy);
      });
    else
      row([](float c, float n, float s, float w, float e, float cx, float cy) {
        return stencil(c, n, s, w, e, cx, cy);
      });
    for (int64_t c = ch; c < box.c1; ++c) d[c] = s[c];
    mbits = rm > mbits ? rm : mbits;
  }
  float m;
  std::memcpy(&m, &mbits, 4);
  return want_resid ? m : 0.0f;
}
}  // namespace

float step(const float* src, float* dst, const Geom& g, const Box& box, bool want_resid) {
  return step_impl<false>(src, dst, nullptr, g, box, want_resid);
}

float step_source(const float* src, float* dst, const float* q, const Geom& g, const Box& box,
                  bool want_resid) {
  HEAT_CHECK(q != nullptr, "source step without a source field");
  HEAT_CHECK(g.numerics == 0, "the source step evaluates the canonical fp32 expression only");
  return step_impl<true>(src, dst, q, g, box, want_resid);
}

void fill_edge_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int insulated_sides,
                      int periodic_axes, int depth) {
  HEAT_CHECK((insulated_sides & ~15) == 0 && (periodic_axes & ~3) == 0 && depth >= 1,
             "fill_edge_ghosts: sides %d axes %d depth %d", insulated_sides, periodic_axes, depth);
  const bool wx = periodic_axes & kPeriodicX, wy = periodic_axes & kPeriodicY;
  HEAT_CHECK(!(wx && (insulated_sides & 3)), "fill_edge_ghosts: axis x both wrapped and mirrored");
  HEAT_CHECK(!(wy && (insulated_sides & 12)), "fill_edge_ghosts: axis y both wrapped and mirrored");
  const bool n = insulated_sides & (1 << North), s = insulated_sides & (1 << South),
             w = insulated_sides & (1 << West), e = insulated_sides & (1 << East);
  HEAT_CHECK(!(n || s) || lx > depth, "fill_insulated_ghosts: %lld rows, depth %d", (long long)lx,
             depth);
  HEAT_CHECK(!(w || e) || ly > depth, "fill_insulated_ghosts: %lld columns, depth %d",
             (long long)ly, depth);
  HEAT_CHECK(!wx || lx >= depth, "fill_edge_ghosts: %lld rows wrapped, depth %d", (long long)lx,
             depth);
  HEAT_CHECK(!wy || ly >= depth, "fill_edge_ghosts: %lld columns wrapped, depth %d", (long long)ly,
             depth);
  const int64_t d = depth;
  // Every cell of the frame beyond a filled side takes its per-axis source
  // (reflected beyond an insulated side, shifted by the extent along a
  // periodic axis); the sources lie beyond no filled side, so none is written.
  auto mr = [&](int64_t r) {
    if (r < 0) return n ? -r : wx ? r + lx : r;
    if (r >= lx) return s ? 2 * (lx - 1) - r : wx ? r - lx : r;
    return r;
  };
  auto mc = [&](int64_t c) {
    if (c < 0) return w ? -c : wy ? c + ly : c;
    if (c >= ly) return e ? 2 * (ly - 1) - c : wy ? c - ly : c;
    return c;
  };
  for (int64_t r = -d; r < lx + d; ++r) {
    const int64_t sr = mr(r);
    float* dst = origin + r * pitch;
    const float* src = origin + sr * pitch;
    if (sr != r) {
      for (int64_t c = -d; c < ly + d; ++c) dst[c] = src[mc(c)];
    } else {
      if (w || wy)
        for (int64_t c = -d; c < 0; ++c) dst[c] = src[mc(c)];
      if (e || wy)
        for (int64_t c = ly; c < ly + d; ++c) dst[c] = src[mc(c)];
    }
  }
}

void fill_insulated_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int sides,
                           int depth) {
  HEAT_CHECK((sides & ~15) == 0 && depth >= 1, "fill_insulated_ghosts: sides %d depth %d", sides,
             depth);
  fill_edge_ghosts(origin, pitch, lx, ly, sides, 0, depth);
}

void copy_box(const float* src, int64_t src_pitch, float* dst, int64_t dst_pitch, const Box& box) {
  if (box.empty()) return;
#pragma omp parallel for schedule(static) if (box.rows() > 64)
  for (int64_t r = box.r0; r < box.r1; ++r)
    std::memcpy(dst + r * dst_pitch + box.c0, src + r * src_pitch + box.c0,
                size_t(box.cols()) * 4);
}

}  // namespace heat::cpu
