// Insulated and periodic plate edges: the ghost fill (see kernels.hpp).
//
// The stencil kernels know fixed-temperature edges only.  An insulated edge
// reaches them as a plate extended into the ghost ring whose ghost cells hold
// the plate's mirror image across the edge row / column (the second-order
// mirror scheme u[-1] := u[1]): every real cell next to the edge is then an
// interior cell, and its missing neighbour is its own mirror image.  A
// periodic axis that one rank spans alone is the same with another source:
// the ghost cells hold the field's opposite edge (u[-1] := u[lx-1]).  This
// unit keeps those ghost cells filled, one launch per halo exchange.
//
// Every side has a mode: none, mirror or wrap (both sides of an axis wrap, or
// neither).  A frame cell's source is the per-axis composition of the maps
//   mirror:  r < 0 -> -r        r >= lx -> 2 (lx - 1) - r
//   wrap:    r < 0 -> r + lx    r >= lx -> r - lx
// (columns alike), the identity on an axis whose side has no mode.
//
// Work split of the one launch (blockIdx.x):
//   * one workgroup per ghost row beyond a filled N/S side: the row is a copy
//     of its source row (rows are 256-B pitched and owned column 0 is 16-B
//     aligned, so columns [0, ly & ~3) move as float4 lanes, a wrapped source
//     row being as aligned as a mirrored one; the tail and the 2 x depth ghost
//     columns -- mapped where W/E is filled, copied where a neighbour's halo
//     or nothing fills them -- as scalars: a wrapped column source ly - d ..
//     is not 16-B aligned when ly % 4 != 0);
//   * the remaining workgroups grid-stride over the <= 2 x depth ghost columns
//     beyond filled W/E sides of every other row of the frame.
// A source lies beyond no filled side, so it is never a target and the launch
// has no ordering hazard.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "heat/common.hpp"
#include "heat/kernels.hpp"

namespace heat::gpu {
namespace {

struct GhostFill {
  int64_t pitch, lx, ly;
  int d;           // frame depth
  int n, s, w, e;  // mode of each side: kNone, kMirror, kWrap
  int vec;         // float4 lanes allowed (aligned origin and pitch)
  int ns_rows;     // ghost rows beyond filled N/S sides: ((n != 0) + (s != 0)) * d
  int64_t side_r0, side_rows;  // the other rows of the frame
  int side_blocks;
};

enum Mode : int { kNone = 0, kMirror = 1, kWrap = 2 };

// The source of index i of an axis of extent n whose low / high sides have the
// modes lo / hi: reflected across cell 0 / n - 1, or shifted by the extent,
// where it lies beyond a filled side.
__device__ __forceinline__ int64_t source(int64_t i, int64_t n, int lo, int hi) {
  if (i < 0) return lo == kMirror ? -i : lo == kWrap ? i + n : i;
  if (i >= n) return hi == kMirror ? 2 * (n - 1) - i : hi == kWrap ? i - n : i;
  return i;
}

__global__ __launch_bounds__(256) void ghost_fill_kernel(float* origin, GhostFill a) {
  const int tid = int(threadIdx.x);
  if (int(blockIdx.x) < a.ns_rows) {
    const int i = int(blockIdx.x);
    const int64_t r = (a.n && i < a.d) ? int64_t(i) - a.d : a.lx + (i - (a.n ? a.d : 0));
    const float* src = origin + source(r, a.lx, a.n, a.s) * a.pitch;
    float* dst = origin + r * a.pitch;
    const int64_t ly4 = a.vec ? (a.ly & ~int64_t(3)) : 0;
    for (int64_t j = tid; j < ly4 / 4; j += 256)
      reinterpret_cast<float4*>(dst)[j] = reinterpret_cast<const float4*>(src)[j];
    for (int64_t c = ly4 + tid; c < a.ly; c += 256) dst[c] = src[c];
    for (int j = tid; j < 2 * a.d; j += 256) {
      const int64_t c = j < a.d ? int64_t(j) - a.d : a.ly + (j - a.d);
      dst[c] = src[source(c, a.ly, a.w, a.e)];
    }
    return;
  }
  const int64_t wc = int64_t((a.w != 0) + (a.e != 0)) * a.d, total = a.side_rows * wc;
  for (int64_t k = (int64_t(blockIdx.x) - a.ns_rows) * 256 + tid; k < total;
       k += int64_t(a.side_blocks) * 256) {
    const int64_t r = a.side_r0 + k / wc, j = k % wc;
    const int64_t c = (a.w && j < a.d) ? j - a.d : a.ly + (j - (a.w ? a.d : 0));
    float* row = origin + r * a.pitch;
    row[c] = row[source(c, a.ly, a.w, a.e)];
  }
}

}  // namespace

void fill_edge_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int insulated_sides,
                      int periodic_axes, int depth, hipStream_t st) {
  HEAT_CHECK((insulated_sides & ~15) == 0 && (periodic_axes & ~3) == 0 && depth >= 1,
             "fill_edge_ghosts: sides %d axes %d depth %d", insulated_sides, periodic_axes, depth);
  const bool wx = (periodic_axes & kPeriodicX) != 0, wy = (periodic_axes & kPeriodicY) != 0;
  HEAT_CHECK(!(wx && (insulated_sides & 3)), "fill_edge_ghosts: axis x both wrapped and mirrored");
  HEAT_CHECK(!(wy && (insulated_sides & 12)), "fill_edge_ghosts: axis y both wrapped and mirrored");
  if (insulated_sides == 0 && periodic_axes == 0) return;
  GhostFill a{};
  a.pitch = pitch;
  a.lx = lx;
  a.ly = ly;
  a.d = depth;
  a.n = wx ? kWrap : (insulated_sides >> North) & 1;
  a.s = wx ? kWrap : (insulated_sides >> South) & 1;
  a.w = wy ? kWrap : (insulated_sides >> West) & 1;
  a.e = wy ? kWrap : (insulated_sides >> East) & 1;
  // Mirror sources are rows (columns) 1..depth and their images at the far
  // edge; wrap sources the last and the first `depth` rows (columns).
  HEAT_CHECK(!(a.n == kMirror || a.s == kMirror) || lx > depth,
             "fill_insulated_ghosts: %lld rows, depth %d", (long long)lx, depth);
  HEAT_CHECK(!(a.w == kMirror || a.e == kMirror) || ly > depth,
             "fill_insulated_ghosts: %lld columns, depth %d", (long long)ly, depth);
  HEAT_CHECK(!wx || lx >= depth, "fill_edge_ghosts: %lld rows wrapped, depth %d", (long long)lx,
             depth);
  HEAT_CHECK(!wy || ly >= depth, "fill_edge_ghosts: %lld columns wrapped, depth %d", (long long)ly,
             depth);
  a.vec = (reinterpret_cast<uintptr_t>(origin) % 16 == 0 && pitch % 4 == 0) ? 1 : 0;
  const int fn = a.n != 0, fs = a.s != 0, fw = a.w != 0, fe = a.e != 0;
  a.ns_rows = (fn + fs) * depth;
  a.side_r0 = fn ? 0 : -int64_t(depth);
  a.side_rows = (fs ? lx : lx + depth) - a.side_r0;
  const int64_t side_cells = a.side_rows * int64_t(fw + fe) * depth;
  a.side_blocks = int(std::min<int64_t>(ceil_div(side_cells, 256), 2048));
  const unsigned blocks = unsigned(a.ns_rows + a.side_blocks);
  if (blocks == 0) return;
  hipLaunchKernelGGL(ghost_fill_kernel, dim3(blocks), dim3(256), 0, st, origin, a);
  HIP_CHECK(hipGetLastError());
}

void fill_insulated_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int sides,
                           int depth, hipStream_t st) {
  HEAT_CHECK((sides & ~15) == 0 && depth >= 1, "fill_insulated_ghosts: sides %d depth %d", sides,
             depth);
  fill_edge_ghosts(origin, pitch, lx, ly, sides, 0, depth, st);
}

}  // namespace heat::gpu
