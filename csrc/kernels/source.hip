// gfx950 (CDNA4) one-step Jacobi update with a static per-cell heat source:
//   u' = heat::stencil(c, n, s, w, e, cx, cy) + q          (kernels.hpp: source_step)
// one rounded fp32 add after the unchanged FMA expression.
//
// Design (three streams, 12 B per cell-update, nothing else on the hot path):
//  * A unit is one wave's share of the box: a strip of 256 columns times a
//    chunk of rows.  Lane l owns columns 4l..4l+3 of the strip; lane 0 of
//    strip 0 starts on the 16-byte boundary at or below the box's first
//    column, so a whole lane's four cells are one aligned dwordx4 access and a
//    wave's row one coalesced 1 KiB access, per array.
//  * The wave streams down its chunk with a 3-row window of u in registers
//    (north, centre, south): every row of src and of q is read once per unit,
//    plus the two window rows above and below the chunk, and dst is written
//    once.  No LDS tile.
//  * East/west neighbours cross lanes with DPP wave shifts.  The strip-edge
//    lanes get theirs from two extra dword loads per row (lane 0: the column
//    left of the strip, lane 63: the one right of it), folded into the shift's
//    `old` operand; a one-lane overlap would recompute 4 of every 256 columns
//    and break the aligned 1 KiB rows.  The neighbour strip's wave of the same
//    chunk reads those lines anyway (adjacent units run on adjacent waves).
//  * Lanes cut by the box's edge, and every lane when the pitch is no multiple
//    of 4 or the three arrays do not share their 16-byte phase, use dword
//    accesses under per-cell masks: no cell outside rows [r0-1, r1] x columns
//    [c0-1, c1] is read, no cell outside the box is written.
//  * Residual: the wave keeps max |new - old| over its updated cells as float
//    bits (a NaN sorts on top); with a residual the workgroup folds its four
//    waves through two LDS words into ONE global atomic (tb_common.hpp).
//    That is the kernel's only LDS; scratch is zero.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "heat/common.hpp"
#include "heat/init_fn.hpp"
#include "heat/kernels.hpp"
#include "tb_common.hpp"

namespace heat::gpu {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct SourceArgs {
  int64_t cs;  // column of lane 0 of strip 0: box.c0 - align
  int64_t strips, units;
  int chunk_rows, vector_rows;
};

// Lane l <- lane l-1 (wave_shr:1); lane 0 keeps `edge` (bound_ctrl off).  The
// edge value rides in the DPP `old` operand: a lane select could become an
// EXEC mask that disables the very lane the shift reads from (lds.hip).
__device__ __forceinline__ float src_from_left(float v, float edge) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
// Lane l <- lane l+1 (wave_shl:1); lane 63 keeps `edge`.
__device__ __forceinline__ float src_from_right(float v, float edge) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130, 0xf, 0xf, false));
}

// Four cells of a row: one dwordx4 access for a whole aligned lane, else the
// cells in `mask` dword by dword (the others read as 0 and are never used).
template <bool NT>
__device__ __forceinline__ v4f load4(const float* p, bool vec, unsigned mask) {
  v4f v = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if constexpr (NT)
      v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    else
      v = *reinterpret_cast<const v4f*>(p);
  } else {
    if (mask & 1u) v.x = p[0];
    if (mask & 2u) v.y = p[1];
    if (mask & 4u) v.z = p[2];
    if (mask & 8u) v.w = p[3];
  }
  return v;
}

// NT: q is read and dst written non-temporally (each is touched once per
// step); src, whose rows the neighbour chunk and strip re-read, stays plain.
template <bool NT>
__global__ __launch_bounds__(256) void source_kernel(const float* __restrict__ src,
                                                     float* __restrict__ dst,
                                                     const float* __restrict__ q, StencilGeom g,
                                                     Box box, SourceArgs a, unsigned* resid) {
  __shared__ unsigned wg[2];
  if (tbdetail::gated(g.gate)) return;  // uniform: before the barrier
  if (resid) {
    if (threadIdx.x < 2) wg[threadIdx.x] = 0u;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int64_t nwaves = int64_t(gridDim.x) * 4;
  unsigned m = 0;
  for (int64_t u = int64_t(blockIdx.x) * 4 + wv; u < a.units; u += nwaves) {
    const int64_t strip = u % a.strips, chunk = u / a.strips;
    const int64_t ra = box.r0 + chunk * a.chunk_rows;
    const int64_t rb = ra + a.chunk_rows < box.r1 ? ra + a.chunk_rows : box.r1;
    const int64_t col = a.cs + strip * kSourceStripCols + 4 * lane;
    // in: the cell is in the box (written); ld: its u is read, the box and one
    // column each side; upd: in the box and no cell of a fixed edge column.
    unsigned in = 0, ld = 0, upd = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t c = col + e;
      const bool i = c >= box.c0 && c < box.c1;
      in |= unsigned(i) << e;
      ld |= unsigned(c >= box.c0 - 1 && c <= box.c1) << e;
      upd |= unsigned(i && tbdetail::in_interior(g.gy0 + c, g.ny)) << e;
    }
    const bool vec_ld = a.vector_rows != 0 && ld == 15u;
    const bool vec_in = a.vector_rows != 0 && in == 15u;
    // Strip-edge lanes: lane 0 reads the cell left of its first, lane 63 the
    // cell right of its last, where that cell of theirs is in the box.
    const bool has_edge = (lane == 0 && (in & 1u)) || (lane == 63 && (in & 8u));
    const int eoff = lane == 0 ? -1 : 4;
    const float* ps = src + (ra - 1) * g.pitch + col;
    v4f n = load4<false>(ps, vec_ld, ld);
    ps += g.pitch;
    v4f c = load4<false>(ps, vec_ld, ld);
    float ec = has_edge ? ps[eoff] : 0.f;
    ps += g.pitch;
    const float* pq = q + ra * g.pitch + col;
    float* pd = dst + ra * g.pitch + col;
    for (int64_t r = ra; r < rb; ++r, ps += g.pitch, pq += g.pitch, pd += g.pitch) {
      const v4f s = load4<false>(ps, vec_ld, ld);
      const float es = has_edge ? ps[eoff] : 0.f;
      const v4f qq = load4<NT>(pq, vec_in, in);
      const float w = src_from_left(c.w, ec);
      const float e = src_from_right(c.x, ec);
      const unsigned um = tbdetail::in_interior(g.gx0 + r, g.nx) ? upd : 0u;
      v4f o;
      o.x = (um & 1u) ? stencil(c.x, n.x, s.x, w, c.y, g.cx, g.cy) + qq.x : c.x;
      o.y = (um & 2u) ? stencil(c.y, n.y, s.y, c.x, c.z, g.cx, g.cy) + qq.y : c.y;
      o.z = (um & 4u) ? stencil(c.z, n.z, s.z, c.y, c.w, g.cx, g.cy) + qq.z : c.z;
      o.w = (um & 8u) ? stencil(c.w, n.w, s.w, c.z, e, g.cx, g.cy) + qq.w : c.w;
      if (vec_in) {
        if constexpr (NT)
          __builtin_nontemporal_store(o, reinterpret_cast<v4f*>(pd));
        else
          *reinterpret_cast<v4f*>(pd) = o;
      } else {
        if (in & 1u) pd[0] = o.x;
        if (in & 2u) pd[1] = o.y;
        if (in & 4u) pd[2] = o.z;
        if (in & 8u) pd[3] = o.w;
      }
      if (resid) {
        m = max(m, (um & 1u) ? __float_as_uint(fabsf(o.x - c.x)) : 0u);
        m = max(m, (um & 2u) ? __float_as_uint(fabsf(o.y - c.y)) : 0u);
        m = max(m, (um & 4u) ? __float_as_uint(fabsf(o.z - c.z)) : 0u);
        m = max(m, (um & 8u) ? __float_as_uint(fabsf(o.w - c.w)) : 0u);
      }
      n = c;
      c = s;
      ec = es;
    }
  }
  if (resid) tbdetail::group_max_atomic(m, resid, wg, 4);
}

std::atomic<int> g_max_waves{0};
std::atomic<int> g_nontemporal{-1};
// A step that sweeps more than the Infinity Cache holds (256 MiB) streams q and
// dst non-temporally; a smaller one keeps them plain, so that the next step
// finds them on die.  Measured both ways (profiles/source.md): 8192^2 (805 MB a
// step) 1.14x faster non-temporal, 1024 x 8192 (101 MB) 1.11x faster plain;
// in between plain still leads by 1.14x at 252 MB, the two are even at 302 MB
// (plain 2 % ahead) and non-temporal leads by 1.17x at 403 MB.
constexpr int64_t kSourceStreamBytes = int64_t(256) << 20;

// Waves of a full launch on the current device: what is resident at once (the
// kernel's occupancy, at most kSourceWavesPerCu per CU).
int device_waves() {
  static std::atomic<int> waves[64] = {};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const int slot = dev & 63;
  int n = waves[slot].load(std::memory_order_relaxed);
  if (n <= 0) {
    int cus = 0, blocks = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, source_kernel<false>, 256, 0));
    n = std::max(cus, 1) * std::min(std::max(blocks, 1) * 4, kSourceWavesPerCu);
    waves[slot].store(n, std::memory_order_relaxed);
  }
  return n;
}

}  // namespace

void source_set_max_waves(int waves) { g_max_waves.store(std::max(waves, 0)); }
void source_set_nontemporal(int mode) { g_nontemporal.store(mode); }

SourcePlan source_plan(const float* src, const float* dst, const float* q, int64_t pitch,
                       const Box& box) {
  SourcePlan pl;
  HEAT_CHECK(!box.empty() && pitch >= box.cols(), "source plan of a %lldx%lld box, pitch %lld",
             (long long)box.rows(), (long long)box.cols(), (long long)pitch);
  const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst),
                  aq = reinterpret_cast<uintptr_t>(q);
  HEAT_CHECK(as % 4 == 0 && ad % 4 == 0 && aq % 4 == 0, "field not 4-byte aligned");
  // One lane layout serves the three arrays: they must share their phase.
  pl.vector_rows = pitch % 4 == 0 && (as & 15) == (ad & 15) && (as & 15) == (aq & 15);
  pl.align = pl.vector_rows ? int((int64_t(as >> 2) + box.c0) & 3) : 0;
  pl.strips = ceil_div(box.cols() + pl.align, kSourceStripCols);
  int cap = g_max_waves.load();
  if (cap <= 0) cap = device_waves();
  // Chunks: the longest (at most kSourceMaxChunkRows) that still give every
  // wave of the launch a unit.  A box too small for that at the longest chunk
  // takes as many chunks as one round of the launch holds, not the next power
  // of two: every wave then has exactly one unit, and no second, part-filled
  // round trails the first.
  int64_t chunks = ceil_div(box.rows(), kSourceMaxChunkRows);
  if (pl.strips * chunks < cap)
    chunks = std::max(chunks, std::min<int64_t>(cap / pl.strips,
                                                ceil_div(box.rows(), kSourceMinChunkRows)));
  pl.chunk_rows = int(ceil_div(box.rows(), chunks));
  pl.chunks = ceil_div(box.rows(), pl.chunk_rows);
  pl.units = pl.strips * pl.chunks;
  pl.waves = int(std::min<int64_t>(pl.units, cap));
  return pl;
}

void source_step(const float* src, float* dst, const float* q, const StencilGeom& g,
                 const Box& box, unsigned* resid, hipStream_t st) {
  if (box.empty()) return;
  HEAT_CHECK(src && dst && q, "source step of a %lldx%lld box: null field", (long long)box.rows(),
             (long long)box.cols());
  HEAT_CHECK(g.numerics == 0, "the source step evaluates the canonical fp32 expression only");
  const SourcePlan pl = source_plan(src, dst, q, g.pitch, box);
  SourceArgs a{};
  a.cs = box.c0 - pl.align;
  a.strips = pl.strips;
  a.units = pl.units;
  a.chunk_rows = pl.chunk_rows;
  a.vector_rows = int(pl.vector_rows);
  const dim3 grid(unsigned(ceil_div(pl.waves, 4)));
  const int mode = g_nontemporal.load();
  const bool nt = mode >= 0 ? mode != 0 : box.rows() * box.cols() * 12 > kSourceStreamBytes;
  if (nt)
    hipLaunchKernelGGL(source_kernel<true>, grid, dim3(256), 0, st, src, dst, q, g, box, a, resid);
  else
    hipLaunchKernelGGL(source_kernel<false>, grid, dim3(256), 0, st, src, dst, q, g, box, a,
                       resid);
  HIP_CHECK(hipGetLastError());
}

}  // namespace heat::gpu
