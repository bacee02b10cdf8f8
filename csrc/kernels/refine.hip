// gfx950 (CDNA4) refinement: fill a block of a field from a small source grid
// S and two axis tables, piecewise constant or cell-centred bilinear
// (io.hpp: the definition; kernels.hpp: the interface).
//
// Design (one streaming write of the block, nothing else on the hot path):
//  * A unit is one wave's share of the block: a strip of 256 columns times a
//    chunk of rows.  Lane l owns columns 4l..4l+3 of the strip and loads their
//    table entries (j0, j1, wy) once per unit.  Lane 0 of strip 0 starts on
//    the 16-byte boundary at or below the origin, so a whole lane's four cells
//    are one aligned dwordx4 store and a wave's row one coalesced 1 KiB write.
//  * The row table is wave-uniform: the unit index comes from blockIdx and the
//    wave id made uniform, so its entries arrive through scalar loads.
//  * S is gathered only when the source row pair (i0, i1) differs from the
//    previous row's: there the lane forms top[4] and bot[4], the column pass
//    of the pair.  A pair that moves on by one row keeps its lower row (the
//    old bot is the new top) and a pair of one row twice (order 0, a clamped
//    edge) gathers once: 8 loads per lane instead of 16.  S is at most 16 MB
//    and stays in cache.  Every other row is one lerp per cell and the store.
//  * Lanes cut by the block's edge (the first lane of an unaligned origin, the
//    ragged last lane) and every lane of a pitch that is no multiple of 4
//    store their cells dword by dword: no ghost or padding cell is written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "heat/common.hpp"
#include "heat/kernels.hpp"

namespace heat::gpu {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct RefineArgs {
  int64_t pitch, lx, ly, cc;
  int64_t strips, units;
  int chunk_rows, align, vector_rows;
};

__device__ __forceinline__ float lerp1(float a, float b, float w) {
  return w == 0.f ? a : __builtin_fmaf(w, b - a, a);
}

// The pointers are kernel arguments of their own, each __restrict__: only so
// can the compiler tell that the block's stores never touch the tables, and
// read the wave-uniform row table through scalar loads.
__global__ __launch_bounds__(256) void refine_kernel(
    RefineArgs a, float* __restrict__ origin, const float* __restrict__ S,
    const int32_t* __restrict__ ri0, const int32_t* __restrict__ ri1,
    const float* __restrict__ rw, const int32_t* __restrict__ cj0,
    const int32_t* __restrict__ cj1, const float* __restrict__ cw) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t nwaves = int64_t(gridDim.x) * 4;
  for (int64_t u = int64_t(blockIdx.x) * 4 + wv; u < a.units; u += nwaves) {
    const int64_t strip = u % a.strips, chunk = u / a.strips;
    const int64_t ra = chunk * a.chunk_rows;
    const int64_t rb = ra + a.chunk_rows < a.lx ? ra + a.chunk_rows : a.lx;
    // Local column of this lane's first cell (>= -3) and which of its four
    // cells lie in the block.
    const int64_t c0 = strip * kRefineStripCols - a.align + 4 * lane;
    unsigned emask = 0;
    int j0[4], j1[4];
    float wy[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = c0 + e >= 0 && c0 + e < a.ly;
      emask |= unsigned(in) << e;
      const int64_t c = in ? c0 + e : 0;  // a cell outside reads column 0's entry, stores nothing
      j0[e] = cj0[c];
      j1[e] = cj1[c];
      wy[e] = cw[c];
    }
    const bool vec = a.vector_rows != 0 && emask == 15u;
    float top[4] = {0.f, 0.f, 0.f, 0.f}, bot[4] = {0.f, 0.f, 0.f, 0.f};
    int pa = -1, pb = -1;
    float* p = origin + ra * a.pitch + c0;
    for (int64_t r = ra; r < rb; ++r, p += a.pitch) {
      const int ia = ri0[r], ib = ri1[r];
      const float wx = rw[r];
      if (ia != pa || ib != pb) {
        if (ia == pb) {  // the same expression of the same row: the same bits
#pragma unroll
          for (int e = 0; e < 4; ++e) top[e] = bot[e];
        } else {
          const float* sa = S + int64_t(ia) * a.cc;
#pragma unroll
          for (int e = 0; e < 4; ++e) top[e] = lerp1(sa[j0[e]], sa[j1[e]], wy[e]);
        }
        if (ib == ia) {
#pragma unroll
          for (int e = 0; e < 4; ++e) bot[e] = top[e];
        } else {
          const float* sb = S + int64_t(ib) * a.cc;
#pragma unroll
          for (int e = 0; e < 4; ++e) bot[e] = lerp1(sb[j0[e]], sb[j1[e]], wy[e]);
        }
        pa = ia;
        pb = ib;
      }
      v4f v;
      v.x = lerp1(top[0], bot[0], wx);
      v.y = lerp1(top[1], bot[1], wx);
      v.z = lerp1(top[2], bot[2], wx);
      v.w = lerp1(top[3], bot[3], wx);
      if (vec) {
        *reinterpret_cast<v4f*>(p) = v;
      } else {
        if (emask & 1u) p[0] = v.x;
        if (emask & 2u) p[1] = v.y;
        if (emask & 4u) p[2] = v.z;
        if (emask & 8u) p[3] = v.w;
      }
    }
  }
}

std::atomic<int> g_max_waves{0};

int device_cus() {
  static std::atomic<int> cus[64] = {};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const int slot = dev & 63;
  int n = cus[slot].load(std::memory_order_relaxed);
  if (n <= 0) {
    HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    n = std::max(n, 1);
    cus[slot].store(n, std::memory_order_relaxed);
  }
  return n;
}

}  // namespace

void refine_set_max_waves(int waves) { g_max_waves.store(std::max(waves, 0)); }

RefinePlan refine_plan(const float* origin, int64_t pitch, int64_t lx, int64_t ly) {
  RefinePlan pl;
  HEAT_CHECK(lx >= 1 && ly >= 1 && pitch >= ly, "refine plan of a %lldx%lld block, pitch %lld",
             (long long)lx, (long long)ly, (long long)pitch);
  const uintptr_t addr = reinterpret_cast<uintptr_t>(origin);
  HEAT_CHECK(addr % 4 == 0, "field not 4-byte aligned");
  pl.vector_rows = pitch % 4 == 0;
  pl.align = pl.vector_rows ? int((addr >> 2) & 3) : 0;
  pl.strips = ceil_div(ly + pl.align, kRefineStripCols);
  int cap = g_max_waves.load();
  if (cap <= 0) cap = device_cus() * kRefineWavesPerCu;
  // Chunks: the longest that still give every wave of the launch a unit.
  for (int R = kRefineMaxChunkRows;; R /= 2) {
    pl.chunk_rows = R;
    pl.chunks = ceil_div(lx, R);
    pl.units = pl.strips * pl.chunks;
    if (pl.units >= cap || R <= kRefineMinChunkRows) break;
  }
  pl.waves = int(std::min<int64_t>(pl.units, cap));
  return pl;
}

void refine_block(float* origin, int64_t pitch, int64_t lx, int64_t ly, const float* S,
                  int64_t cc, const RefineTable& rows, const RefineTable& cols, hipStream_t st) {
  if (lx <= 0 || ly <= 0) return;
  HEAT_CHECK(origin && S && cc >= 1 && rows.i0 && rows.i1 && rows.w && cols.i0 && cols.i1 &&
                 cols.w,
             "refine of a %lldx%lld block", (long long)lx, (long long)ly);
  const RefinePlan pl = refine_plan(origin, pitch, lx, ly);
  RefineArgs a{};
  a.pitch = pitch;
  a.lx = lx;
  a.ly = ly;
  a.cc = cc;
  a.strips = pl.strips;
  a.units = pl.units;
  a.chunk_rows = pl.chunk_rows;
  a.align = pl.align;
  a.vector_rows = int(pl.vector_rows);
  const dim3 grid(unsigned(ceil_div(pl.waves, 4)));
  hipLaunchKernelGGL(refine_kernel, grid, dim3(256), 0, st, a, origin, S, rows.i0, rows.i1,
                     rows.w, cols.i0, cols.i1, cols.w);
  HIP_CHECK(hipGetLastError());
}

}  // namespace heat::gpu
