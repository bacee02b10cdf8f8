// Insulated (zero-flux) plate edges: the ghost fill (see kernels.hpp).
//
// The stencil kernels know fixed-temperature edges only.  An insulated edge
// reaches them as a plate extended into the ghost ring whose ghost cells hold
// the plate's mirror image across the edge row / column (the second-order
// mirror scheme u[-1] := u[1]): every real cell next to the edge is then an
// interior cell, and its missing neighbour is its own mirror image.  This
// unit keeps those ghost cells filled, one launch per halo exchange.
//
// Work split of the one launch (blockIdx.x):
//   * one workgroup per ghost row beyond an insulated N/S side: the row is a
//     copy of its mirror row (rows are 256-B pitched and owned column 0 is
//     16-B aligned, so columns [0, ly & ~3) move as float4 lanes; the tail and
//     the 2 x depth ghost columns -- reflected where W/E is insulated, copied
//     where a neighbour's halo or nothing fills them -- as scalars);
//   * the remaining workgroups grid-stride over the <= 2 x depth ghost columns
//     beyond insulated W/E sides of every other row of the frame.
// A source is never a target, so the launch has no ordering hazard.
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
  int n, s, w, e;  // insulated sides (0 / 1)
  int vec;         // float4 lanes allowed (aligned origin and pitch)
  int ns_rows;     // ghost rows beyond insulated N/S sides: (n + s) * d
  int64_t side_r0, side_rows;  // the other rows of the frame
  int side_blocks;
};

// Index i of an axis of extent n, reflected across cell 0 (lo) / n - 1 (hi)
// where it lies beyond an insulated side.
__device__ __forceinline__ int64_t mirror(int64_t i, int64_t n, int lo, int hi) {
  return (lo && i < 0) ? -i : (hi && i >= n) ? 2 * (n - 1) - i : i;
}

__global__ __launch_bounds__(256) void ghost_fill_kernel(float* origin, GhostFill a) {
  const int tid = int(threadIdx.x);
  if (int(blockIdx.x) < a.ns_rows) {
    const int i = int(blockIdx.x);
    const int64_t r = (a.n && i < a.d) ? int64_t(i) - a.d : a.lx + (i - (a.n ? a.d : 0));
    const float* src = origin + mirror(r, a.lx, a.n, a.s) * a.pitch;
    float* dst = origin + r * a.pitch;
    const int64_t ly4 = a.vec ? (a.ly & ~int64_t(3)) : 0;
    for (int64_t j = tid; j < ly4 / 4; j += 256)
      reinterpret_cast<float4*>(dst)[j] = reinterpret_cast<const float4*>(src)[j];
    for (int64_t c = ly4 + tid; c < a.ly; c += 256) dst[c] = src[c];
    for (int j = tid; j < 2 * a.d; j += 256) {
      const int64_t c = j < a.d ? int64_t(j) - a.d : a.ly + (j - a.d);
      dst[c] = src[mirror(c, a.ly, a.w, a.e)];
    }
    return;
  }
  const int64_t wc = int64_t(a.w + a.e) * a.d, total = a.side_rows * wc;
  for (int64_t k = (int64_t(blockIdx.x) - a.ns_rows) * 256 + tid; k < total;
       k += int64_t(a.side_blocks) * 256) {
    const int64_t r = a.side_r0 + k / wc, j = k % wc;
    const int64_t c = (a.w && j < a.d) ? j - a.d : a.ly + (j - (a.w ? a.d : 0));
    float* row = origin + r * a.pitch;
    row[c] = row[mirror(c, a.ly, a.w, a.e)];
  }
}

}  // namespace

void fill_insulated_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int sides,
                           int depth, hipStream_t st) {
  HEAT_CHECK((sides & ~15) == 0 && depth >= 1, "fill_insulated_ghosts: sides %d depth %d", sides,
             depth);
  if (sides == 0) return;
  GhostFill a{};
  a.pitch = pitch;
  a.lx = lx;
  a.ly = ly;
  a.d = depth;
  a.n = (sides >> North) & 1;
  a.s = (sides >> South) & 1;
  a.w = (sides >> West) & 1;
  a.e = (sides >> East) & 1;
  // Mirror sources are rows (columns) 1..depth and their images at the far edge.
  HEAT_CHECK(!(a.n || a.s) || lx > depth, "fill_insulated_ghosts: %lld rows, depth %d",
             (long long)lx, depth);
  HEAT_CHECK(!(a.w || a.e) || ly > depth, "fill_insulated_ghosts: %lld columns, depth %d",
             (long long)ly, depth);
  a.vec = (reinterpret_cast<uintptr_t>(origin) % 16 == 0 && pitch % 4 == 0) ? 1 : 0;
  a.ns_rows = (a.n + a.s) * depth;
  a.side_r0 = a.n ? 0 : -int64_t(depth);
  a.side_rows = (a.s ? lx : lx + depth) - a.side_r0;
  const int64_t side_cells = a.side_rows * int64_t(a.w + a.e) * depth;
  a.side_blocks = int(std::min<int64_t>(ceil_div(side_cells, 256), 2048));
  const unsigned blocks = unsigned(a.ns_rows + a.side_blocks);
  if (blocks == 0) return;
  hipLaunchKernelGGL(ghost_fill_kernel, dim3(blocks), dim3(256), 0, st, origin, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace heat::gpu
