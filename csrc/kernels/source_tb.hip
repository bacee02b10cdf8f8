// gfx950 (CDNA4) K fused Jacobi steps with a static per-cell heat source in one
// launch (kernels.hpp: source_tb_step), K = 2 .. kSourceTbMaxDepth:
//   u_j = heat::stencil(c, n, s, w, e, cx, cy) + q      on level j = 1 .. K
// bit for bit what K calls of source_step over the shrinking boxes give (call
// j over the box grown by K-1-j and clipped to the plate).  src and q are read
// once and dst written once per K steps instead of once per step.
//
// Design (one wave per unit, everything in VGPRs, no LDS tile):
//  * A unit is a strip of 256 columns times a chunk of rows.  Lane l owns four
//    adjacent columns as a float4; lane 0 of strip 0 starts OV = round_up(K, 4)
//    columns left of the 16-byte boundary at or below the box's first column.
//    Neighbouring strips overlap by OV columns on each side (a strip advances
//    by 256 - 2 OV columns): a strip-edge lane has no east (west) neighbour and
//    level j is wrong in the j outermost columns of the strip, which after K
//    levels is still inside the 2 x OV columns the strip does not store.  No
//    edge-lane extra loads, and every row is an aligned 1 KiB access.
//  * The wave streams down its chunk.  Iteration i loads row R = ra - K + i of
//    src; level j then produces its row R - j from the two rows it kept of
//    level j-1 (north, centre) and the row level j-1 produced just now
//    (south).  Level K's row R - K is stored once it lies in the chunk.  The
//    windows start as zeros: the rows a level produces before its first valid
//    one (ra - K + j) are never read by a valid row of the next level, so one
//    uniform loop body serves the ramp too.  Chunks overlap by K rows per side.
//  * q: level j adds the q row R - j, the row loaded j - 1 iterations earlier.
//    A ring of K float4 slots holds them; the loop is unrolled lcm(K, 2) times
//    so that every ring slot and window slot is a compile-time register.
//  * East/west neighbours cross lanes with DPP wave shifts (wave_shr/shl:1).
//  * A cell that no level updates (a fixed edge of the plate, or off it) keeps
//    its centre value at every level, so nothing wrong crosses the plate's
//    edge; cells outside the allowed read regions (src: box grown by K, q: box
//    grown by K-1, both clipped to the plate) are never loaded and count as 0:
//    they cannot reach an output cell in K levels.
//  * Lanes cut by a region's edge, and every lane when the pitch is no
//    multiple of 4 or the three arrays do not share their 16-byte phase, use
//    dword accesses under per-cell masks.  dst is written on the box alone.
//  * Residual (its own instantiation): max |u_K - u_{K-1}| over the updated
//    cells the wave stores, as float bits (a NaN sorts on top), folded through
//    two LDS words into one global atomic per workgroup (tb_common.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "heat/common.hpp"
#include "heat/init_fn.hpp"
#include "heat/kernels.hpp"
#include "tb_common.hpp"

namespace heat::gpu {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

// Everything the kernel needs, relative to the box's first cell and in 32
// bits, so that the scalar registers hold it all: with 64-bit boxes and the
// plate's geometry they ran out, and two instantiations went to scratch.
struct SourceTbArgs {
  const float* src;  // cell (box.r0, box.c0) of each array
  float* dst;
  const float* q;
  unsigned* resid;
  const unsigned* gate;
  int64_t pitch;
  float cx, cy;
  int rows, cols;  // of the box
  int strips, units, chunk_rows;
  int lead;             // columns from lane 0 of strip 0 to the box: align + overlap
  int vector_rows;
  int en, es, ew, ee;   // rows / columns of src that may be read beyond the box, 0 .. k
  int ir0, ir1, ic0, ic1;  // the plate's interior: rows [ir0, ir1), columns [ic0, ic1)
};

// Lane l <- lane l-1 (wave_shr:1); lane 0 reads 0 (bound_ctrl on, so the
// shift needs no `old` operand and can fold into the add that consumes it):
// the strip's outermost columns are never stored.
__device__ __forceinline__ float tb_from_left(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
// Lane l <- lane l+1 (wave_shl:1); lane 63 reads 0.
__device__ __forceinline__ float tb_from_right(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}

// Four cells of a row: one dwordx4 access for a whole aligned lane, else the
// cells in `mask` dword by dword; the others, and every cell of a row that is
// not `live` (wave-uniform), read as 0.
__device__ __forceinline__ v4f tb_load4(const float* p, bool live, bool vec, unsigned mask) {
  v4f v = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    if (vec) {
      v = *reinterpret_cast<const v4f*>(p);
    } else {
      if (mask & 1u) v.x = p[0];
      if (mask & 2u) v.y = p[1];
      if (mask & 4u) v.z = p[2];
      if (mask & 8u) v.w = p[3];
    }
  }
  return v;
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

template <int K, bool RES>
__global__ __launch_bounds__(256) void source_tb_kernel(SourceTbArgs a) {
  constexpr int OV = (K + 3) / 4 * 4;
  constexpr int STRIDE = kSourceTbStripCols - 2 * OV;
  constexpr int U = K % 2 == 0 ? K : 2 * K;  // ring (K) and window (2) slots repeat
  __shared__ unsigned wg[2];
  if (tbdetail::gated(a.gate)) return;  // uniform: before the barrier
  if constexpr (RES) {
    if (threadIdx.x < 2) wg[threadIdx.x] = 0u;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int nwaves = int(gridDim.x) * 4;
  unsigned m = 0;
  for (int u = int(blockIdx.x) * 4 + wv; u < a.units; u += nwaves) {
    const int strip = u % a.strips, chunk = u / a.strips;
    const int ra = chunk * a.chunk_rows;
    const int rb = min(ra + a.chunk_rows, a.rows);
    const int col = strip * STRIDE - a.lead + 4 * lane;
    // ld / lq: the cell's u / q may be read; in: the cell is stored (in the box
    // and in the columns this strip owns); upd: no cell of a fixed column.
    const bool own = 4 * lane >= OV && 4 * lane < kSourceTbStripCols - OV;
    unsigned ld = 0, lq = 0, in = 0, upd = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = col + e;
      ld |= unsigned(c >= -a.ew && c < a.cols + a.ee) << e;
      lq |= unsigned(c >= -min(a.ew, K - 1) && c < a.cols + min(a.ee, K - 1)) << e;
      in |= unsigned(own && c >= 0 && c < a.cols) << e;
      upd |= unsigned(c >= a.ic0 && c < a.ic1) << e;
    }
    // The four update masks as wave-wide lane masks in scalar registers: a
    // level's row flag then joins them with one scalar AND each, and every
    // cell's select is a single v_cndmask.
    const uint64_t ux = __builtin_amdgcn_ballot_w64((upd & 1u) != 0),
                   uy = __builtin_amdgcn_ballot_w64((upd & 2u) != 0),
                   uz = __builtin_amdgcn_ballot_w64((upd & 4u) != 0),
                   uw = __builtin_amdgcn_ballot_w64((upd & 8u) != 0);

    v4f win[K][2];  // level j's last two rows: [i & 1] the older (north)
    v4f qr[K];      // q rows R-1 .. R-K
#pragma unroll
    for (int j = 0; j < K; ++j) {
      win[j][0] = win[j][1] = v4f{0.f, 0.f, 0.f, 0.f};
      qr[j] = v4f{0.f, 0.f, 0.f, 0.f};
    }
    const int iters = rb - ra + 2 * K;
    // Iteration i loads row R = ra - K + i of src and row R - 1 of q; level j
    // produces row R - j.  As iteration numbers (wave-uniform): the rows of src
    // [su0, su1) and of q [sq0, sq1) that may be read, and the plate's interior
    // rows [si0, si1) by i - j.
    const int R0 = ra - K;
    const int su0 = -a.en - R0, su1 = a.rows + a.es - R0;
    const int sq0 = -min(a.en, K - 1) - R0 + 1, sq1 = a.rows + min(a.es, K - 1) - R0 + 1;
    const int si0 = a.ir0 - R0, si1 = a.ir1 - R0;
    // The row pointers may start rows above or columns left of the arrays:
    // they are only dereferenced under the row flags and cell masks.
    const float* ps = a.src + int64_t(R0) * a.pitch + col;
    const float* pq = a.q + int64_t(R0 - 1) * a.pitch + col;
    float* pd = a.dst + int64_t(ra) * a.pitch + col;
    // One iteration ahead: the rows of iteration i + 1 are in flight while i computes.
    v4f ns = tb_load4(ps, 0 >= su0 && 0 < su1, a.vector_rows != 0 && ld == 15u, ld);
    v4f nq = tb_load4(pq, 0 >= sq0 && 0 < sq1, a.vector_rows != 0 && lq == 15u, lq);
    for (int i0 = 0; i0 < iters; i0 += U) {
      static_for<0, U>([&](auto uc) __attribute__((always_inline)) {
        constexpr int uu = decltype(uc)::value;
        constexpr int P = uu & 1;
        const int i = i0 + uu;
        if (i < iters) {
          // The access masks stay in their three VGPRs: hoisted out of the
          // loop as lane masks they would take 30 scalar registers.
          asm volatile("" : "+v"(ld), "+v"(lq), "+v"(in));
          v4f x = ns;  // level 0, row R
          qr[uu % K] = nq;
          ps += a.pitch;
          pq += a.pitch;
          {
            const int i1 = i + 1;  // rows past the last iteration's are not needed
            ns = tb_load4(ps, i1 < iters && i1 >= su0 && i1 < su1,
                          a.vector_rows != 0 && ld == 15u, ld);
            nq = tb_load4(pq, i1 < iters && i1 >= sq0 && i1 < sq1,
                          a.vector_rows != 0 && lq == 15u, lq);
          }
          static_for<1, K + 1>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            const v4f n = win[j - 1][P], c = win[j - 1][P ^ 1];
            const v4f qq = qr[(uu - (j - 1) + 2 * K) % K];
            const bool ri = i - j >= si0 && i - j < si1;
            const float w = tb_from_left(c.w);
            const float e = tb_from_right(c.x);
            // Every cell is evaluated and then selected (one v_cndmask under a
            // scalar-made lane mask): a branch per cell costs more than the
            // arithmetic it skips on the plate's one fixed ring.
            const v4f t = {stencil(c.x, n.x, x.x, w, c.y, a.cx, a.cy) + qq.x,
                           stencil(c.y, n.y, x.y, c.x, c.z, a.cx, a.cy) + qq.y,
                           stencil(c.z, n.z, x.z, c.y, c.w, a.cx, a.cy) + qq.z,
                           stencil(c.w, n.w, x.w, c.z, e, a.cx, a.cy) + qq.w};
            v4f o;
            const uint64_t rm = ri ? ~uint64_t(0) : uint64_t(0);
            o.x = __builtin_amdgcn_inverse_ballot_w64(ux & rm) ? t.x : c.x;
            o.y = __builtin_amdgcn_inverse_ballot_w64(uy & rm) ? t.y : c.y;
            o.z = __builtin_amdgcn_inverse_ballot_w64(uz & rm) ? t.z : c.z;
            o.w = __builtin_amdgcn_inverse_ballot_w64(uw & rm) ? t.w : c.w;
            win[j - 1][P] = x;  // the north row's slot takes the newest
            if constexpr (j == K) {
              if (i >= 2 * K) {  // row R - K >= ra; < rb by the loop bound
                if (a.vector_rows != 0 && in == 15u) {
                  *reinterpret_cast<v4f*>(pd) = o;
                } else {
                  if (in & 1u) pd[0] = o.x;
                  if (in & 2u) pd[1] = o.y;
                  if (in & 4u) pd[2] = o.z;
                  if (in & 8u) pd[3] = o.w;
                }
                pd += a.pitch;
                if constexpr (RES) {
                  const unsigned um = ri ? (upd & in) : 0u;
                  m = max(m, (um & 1u) ? __float_as_uint(fabsf(o.x - c.x)) : 0u);
                  m = max(m, (um & 2u) ? __float_as_uint(fabsf(o.y - c.y)) : 0u);
                  m = max(m, (um & 4u) ? __float_as_uint(fabsf(o.z - c.z)) : 0u);
                  m = max(m, (um & 8u) ? __float_as_uint(fabsf(o.w - c.w)) : 0u);
                }
              }
            }
            x = o;
          });
        }
      });
    }
  }
  if constexpr (RES) tbdetail::group_max_atomic(m, a.resid, wg, 4);
}

std::atomic<int> g_max_waves{0};
std::atomic<long long> g_launches{0};

using KernelFn = void (*)(SourceTbArgs);
template <bool RES>
KernelFn kernel_of(int k) {
  switch (k) {
    case 2: return source_tb_kernel<2, RES>;
    case 3: return source_tb_kernel<3, RES>;
    case 4: return source_tb_kernel<4, RES>;
    case 5: return source_tb_kernel<5, RES>;
    case 6: return source_tb_kernel<6, RES>;
    case 7: return source_tb_kernel<7, RES>;
    case 8: return source_tb_kernel<8, RES>;
  }
  return nullptr;
}

// Waves of a full launch at depth k on the current device: what is resident
// at once, at most kSourceTbWavesPerCu per CU.
int device_waves(int k) {
  static std::atomic<int> waves[64][kSourceTbMaxDepth + 1] = {};
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::atomic<int>& slot = waves[dev & 63][k];
  int n = slot.load(std::memory_order_relaxed);
  if (n <= 0) {
    int cus = 0, blocks = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &blocks, reinterpret_cast<const void*>(kernel_of<true>(k)), 256, 0));
    n = std::max(cus, 1) * std::min(std::max(blocks, 1) * 4, kSourceTbWavesPerCu);
    slot.store(n, std::memory_order_relaxed);
  }
  return n;
}

}  // namespace

void source_tb_set_max_waves(int waves) { g_max_waves.store(std::max(waves, 0)); }
long long source_tb_launches() { return g_launches.load(); }

SourceTbPlan source_tb_plan(const float* src, const float* dst, const float* q, int64_t pitch,
                            const Box& box, int k) {
  SourceTbPlan pl;
  HEAT_CHECK(k >= 2 && k <= kSourceTbMaxDepth, "fused source pass of depth %d: 2..%d", k,
             kSourceTbMaxDepth);
  HEAT_CHECK(!box.empty() && pitch >= box.cols() && box.rows() < (1 << 28) &&
                 box.cols() < (1 << 28),
             "fused source plan of a %lldx%lld box, pitch %lld", (long long)box.rows(),
             (long long)box.cols(), (long long)pitch);
  const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst),
                  aq = reinterpret_cast<uintptr_t>(q);
  HEAT_CHECK(as % 4 == 0 && ad % 4 == 0 && aq % 4 == 0, "field not 4-byte aligned");
  // One lane layout serves the three arrays: they must share their phase.
  pl.vector_rows = pitch % 4 == 0 && (as & 15) == (ad & 15) && (as & 15) == (aq & 15);
  pl.align = pl.vector_rows ? int((int64_t(as >> 2) + box.c0) & 3) : 0;
  pl.overlap = int(round_up(k, 4));
  pl.strip_stride = kSourceTbStripCols - 2 * pl.overlap;
  pl.strips = ceil_div(box.cols() + pl.align, pl.strip_stride);
  int cap = g_max_waves.load();
  if (cap <= 0) cap = device_waves(k);
  // Chunks: long ones (every chunk recomputes 2k rows), shortened down to
  // kSourceTbMinChunkRows while the units do not fill the whole rounds of
  // resident waves that the longest chunks begin.
  const int64_t longest = ceil_div(box.rows(), kSourceTbMaxChunkRows);
  const int64_t rounds = std::max<int64_t>(1, ceil_div(pl.strips * longest, cap));
  const int64_t chunks =
      std::max(longest, std::min<int64_t>(rounds * cap / pl.strips,
                                          box.rows() / kSourceTbMinChunkRows));
  pl.chunk_rows = int(ceil_div(box.rows(), chunks));
  pl.chunks = ceil_div(box.rows(), pl.chunk_rows);
  pl.units = pl.strips * pl.chunks;
  pl.waves = int(std::min<int64_t>(pl.units, cap));
  return pl;
}

void source_tb_step(const float* src, float* dst, const float* q, const StencilGeom& g,
                    const Box& box, int k, unsigned* resid, hipStream_t st) {
  HEAT_CHECK(k >= 2 && k <= kSourceTbMaxDepth, "fused source pass of depth %d: 2..%d", k,
             kSourceTbMaxDepth);
  if (box.empty()) return;
  HEAT_CHECK(src && dst && q, "fused source pass of a %lldx%lld box: null field",
             (long long)box.rows(), (long long)box.cols());
  HEAT_CHECK(src != dst, "fused source pass in place");
  HEAT_CHECK(g.numerics == 0, "the source step evaluates the canonical fp32 expression only");
  const SourceTbPlan pl = source_tb_plan(src, dst, q, g.pitch, box, k);
  // The plate's rectangle and its interior, relative to the box's first cell
  // and clamped far outside the box (whose extents are below 2^28).
  const auto rel = [](int64_t v) { return int(std::clamp<int64_t>(v, -(1 << 29), 1 << 29)); };
  const int64_t p0r = -g.gx0 - box.r0, p0c = -g.gy0 - box.c0;  // plate cell (0, 0)
  SourceTbArgs a{};
  a.src = src + box.r0 * g.pitch + box.c0;
  a.dst = dst + box.r0 * g.pitch + box.c0;
  a.q = q + box.r0 * g.pitch + box.c0;
  a.resid = resid;
  a.gate = g.gate;
  a.pitch = g.pitch;
  a.cx = g.cx;
  a.cy = g.cy;
  a.rows = int(box.rows());
  a.cols = int(box.cols());
  a.strips = int(pl.strips);
  a.units = int(pl.units);
  a.chunk_rows = pl.chunk_rows;
  a.lead = pl.align + pl.overlap;
  a.vector_rows = int(pl.vector_rows);
  // src is read in the box grown by k, clipped to the plate (q: by k - 1).
  a.en = int(std::clamp<int64_t>(-p0r, 0, k));
  a.es = int(std::clamp<int64_t>(p0r + g.nx - box.rows(), 0, k));
  a.ew = int(std::clamp<int64_t>(-p0c, 0, k));
  a.ee = int(std::clamp<int64_t>(p0c + g.ny - box.cols(), 0, k));
  a.ir0 = rel(p0r + 1);
  a.ir1 = rel(p0r + g.nx - 1);
  a.ic0 = rel(p0c + 1);
  a.ic1 = rel(p0c + g.ny - 1);
  const dim3 grid(unsigned(ceil_div(pl.waves, 4)));
  const KernelFn fn = resid ? kernel_of<true>(k) : kernel_of<false>(k);
  hipLaunchKernelGGL(fn, grid, dim3(256), 0, st, a);
  HIP_CHECK(hipGetLastError());
  g_launches.fetch_add(1, std::memory_order_relaxed);
}

}  // namespace heat::gpu
