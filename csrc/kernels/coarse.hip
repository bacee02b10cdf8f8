// gfx950 (CDNA4) coarse view: per coarse cell of fx x fy plate cells the fp64
// sum, the min and the max of a block of a field (kernels.hpp).
//
// Design (one streaming read of the block, nothing else on the hot path):
//  * A unit is one wave's share of the block: a strip of at most 256 columns
//    times a chunk of rows.  A wave reads a row of its strip as one coalesced
//    1 KiB dwordx4 access (lane l holds columns 4l..4l+3); lanes whose float4
//    is cut by the strip's or the block's edge read their cells one by one, so
//    no ghost or padding cell is ever loaded.
//  * The rows of one coarse row accumulate in the lane's own registers
//    (fp64 sum, float min / max and a NaN bit per column): no cross-lane work
//    per row.  Only when a coarse row of the chunk ends are the columns of a
//    coarse cell combined across lanes: a segmented shuffle reduction for
//    fy >= 4 (a lane's float4 then spans at most two cells), a transposition
//    through the wave's own 4 KiB of LDS for fy < 4 (a lane holds several).
//  * Ownership before atomics: where fy allows (a strip of whole coarse
//    columns fits 256 lanes-columns) strips start and end on cell boundaries,
//    and chunks on coarse-row boundaries where fx <= the chunk length, so a
//    cell that lies whole inside the block is written by exactly one wave
//    with plain stores.  Cells wider than a strip, taller than a chunk or cut
//    by the block's edge are merged with one atomic per wave, cell and plane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "heat/common.hpp"
#include "heat/kernels.hpp"

namespace heat::gpu {
namespace {

constexpr int kKeyNan = 0x7FFFFFFF;            // above key(+inf)
constexpr int kKeyLowest = int(0x807FFFFFu);   // key(-inf): the identity of both planes

__host__ __device__ inline int coarse_key(float f) {
  if (f != f) return kKeyNan;
  int i;
  __builtin_memcpy(&i, &f, 4);
  return i >= 0 ? i : (i ^ 0x7FFFFFFF);
}
__host__ __device__ inline float coarse_unkey(int k) {
  const int i = k >= 0 ? k : (k ^ 0x7FFFFFFF);  // kKeyNan: a quiet NaN's bits
  float f;
  __builtin_memcpy(&f, &i, 4);
  return f;
}

__global__ void coarse_reset_kernel(CoarsePlanes p, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * blockDim.x) {
    p.sum[i] = 0.0;
    p.nmin_key[i] = kKeyLowest;
    p.max_key[i] = kKeyLowest;
  }
}

__global__ void coarse_encode_kernel(CoarsePlanes p, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * blockDim.x) {
    p.nmin_key[i] = coarse_key(-__int_as_float(p.nmin_key[i]));
    p.max_key[i] = coarse_key(__int_as_float(p.max_key[i]));
  }
}

__global__ void coarse_decode_kernel(CoarsePlanes p, int64_t n, int negated_min) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += int64_t(gridDim.x) * blockDim.x) {
    const float m = coarse_unkey(p.nmin_key[i]);
    p.nmin_key[i] = __float_as_int(negated_min ? m : -m);
    p.max_key[i] = __float_as_int(coarse_unkey(p.max_key[i]));
  }
}

struct CoarseArgs {
  const float* origin;
  int64_t pitch, lx, ly, ox, oy, nx, ny, fx, fy, cc;
  CoarsePlanes planes;
  int64_t strips, units;
  int64_t j0, i0;        // first coarse column / row the block touches
  int align;             // (address of origin in floats) mod 4; 0 without vector rows
  int owned, cells_per_strip;
  int chunk_rows, cells_per_chunk;  // cells_per_chunk 0: plain chunks of chunk_rows rows
  int vector_rows;
};

__device__ __forceinline__ int pmod4(int64_t v) { return int(v & 3); }
__device__ __forceinline__ int64_t lmin(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t lmax(int64_t a, int64_t b) { return a > b ? a : b; }

// A row's four columns of this lane: one dwordx4 where all four are the
// lane's to read, else only the cells that are.
__device__ __forceinline__ float4 load_cols(const float* p, unsigned emask, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec && emask == 15u) {
    v = *reinterpret_cast<const float4*>(p);
  } else {
    if (emask & 1u) v.x = p[0];
    if (emask & 2u) v.y = p[1];
    if (emask & 4u) v.z = p[2];
    if (emask & 8u) v.w = p[3];
  }
  return v;
}

struct ColAcc {
  double s[4];
  float mn[4], mx[4];
  unsigned nan;
};

__device__ __forceinline__ void acc_one(ColAcc& a, int e, float v, unsigned emask) {
  if ((emask >> e) & 1u) {
    a.s[e] += double(v);
    a.mn[e] = fminf(a.mn[e], v);  // ignore NaN: the nan bit carries it
    a.mx[e] = fmaxf(a.mx[e], v);
    a.nan |= unsigned(v != v) << e;
  }
}
__device__ __forceinline__ void acc_row(ColAcc& a, const float4& v, unsigned emask) {
  acc_one(a, 0, v.x, emask);
  acc_one(a, 1, v.y, emask);
  acc_one(a, 2, v.z, emask);
  acc_one(a, 3, v.w, emask);
}

// One cell's contribution: plain stores if this wave holds the whole cell.
__device__ __forceinline__ void emit(const CoarseArgs& a, int64_t I, int64_t J, bool rows_whole,
                                     double s, int knmin, int kmax) {
  const int64_t idx = I * a.cc + J;
  const bool whole = rows_whole && a.owned && J * a.fy >= a.oy &&
                     lmin((J + 1) * a.fy, a.ny) <= a.oy + a.ly;
  if (whole) {
    a.planes.sum[idx] = s;
    a.planes.nmin_key[idx] = knmin;
    a.planes.max_key[idx] = kmax;
  } else {
    atomicAdd(&a.planes.sum[idx], s);
    atomicMax(&a.planes.nmin_key[idx], knmin);
    atomicMax(&a.planes.max_key[idx], kmax);
  }
}

// MODE 0: fy < 4, cells gathered from the wave's LDS; MODE 1: fy >= 4,
// segmented shuffle reduction.
template <int MODE>
__global__ __launch_bounds__(256) void coarse_kernel(CoarseArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nwaves = int64_t(gridDim.x) * 4;
  for (int64_t u = int64_t(blockIdx.x) * 4 + wv; u < a.units; u += nwaves) {
    const int64_t strip = u % a.strips, chunk = u / a.strips;
    // Columns of the strip: lane 0's first column cs (local, may be < 0) and
    // the global columns [glo, ghi) the strip takes.
    int64_t cs, glo, ghi, ja = 0;
    if (a.owned) {
      ja = a.j0 + strip * a.cells_per_strip;
      const int64_t v = ja * a.fy - a.oy;
      cs = v - (a.vector_rows ? pmod4(v + a.align) : 0);
      glo = lmax(ja * a.fy, a.oy);
      ghi = lmin((ja + a.cells_per_strip) * a.fy, a.oy + a.ly);
    } else {
      cs = strip * kCoarseStripCols - a.align;
      glo = a.oy;
      ghi = a.oy + a.ly;
    }
    // Rows of the chunk (global).
    int64_t ra, rb;
    if (a.cells_per_chunk) {
      ra = (a.i0 + chunk * a.cells_per_chunk) * a.fx;
      rb = ra + int64_t(a.cells_per_chunk) * a.fx;
    } else {
      ra = a.ox + chunk * a.chunk_rows;
      rb = ra + a.chunk_rows;
    }
    ra = lmax(ra, a.ox);
    rb = lmin(rb, a.ox + a.lx);
    if (ra >= rb || glo >= ghi) continue;

    const int64_t c0 = cs + 4 * lane;  // local column of this lane's first element
    const int64_t g0 = a.oy + c0;      // global (>= -3)
    unsigned emask = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (g0 + e >= glo && g0 + e < ghi) emask |= 1u << e;

    // MODE 1: the lane's head cell jc (elements e < eb) and tail cell jc + 1
    // (e >= eb, if eb < 4), and what the segmented reduction needs.
    int64_t jc = 0;
    int eb = 4;
    unsigned same = 0;
    bool head = false, prev_tail = false, any_head = false, any_tail = false;
    if constexpr (MODE == 1) {
      const int64_t q = (g0 + a.fy) / a.fy, rem = (g0 + a.fy) - q * a.fy;
      jc = q - 1;
      eb = int(lmin(4, a.fy - rem));
      const int jr = int(jc - int64_t(__shfl((long long)jc, 0)));
      const bool has_tail = eb < 4;
      any_head = (emask & ((1u << eb) - 1u)) != 0u;
      any_tail = has_tail && (emask >> eb) != 0u;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int d = 1 << k;
        const int oj = __shfl_down(jr, d);
        if (lane + d < 64 && oj == jr) same |= 1u << k;
      }
      const int pj = __shfl_up(jr, 1);
      const int pt = __shfl_up(int(has_tail), 1);
      head = lane == 0 || pj != jr;
      prev_tail = lane > 0 && pt != 0 && pj + 1 == jr;
      int any = int(any_head);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int o = __shfl_down(any, 1 << k);
        if ((same >> k) & 1u) any |= o;
      }
      const int ptv = __shfl_up(int(any_tail), 1);
      if (prev_tail) any |= ptv;
      any_head = any != 0;
    }

    int64_t g = ra;
    while (g < rb) {
      const int64_t I = g / a.fx;
      const int64_t cell_r0 = I * a.fx, cell_r1 = lmin((I + 1) * a.fx, a.nx);
      const int64_t r1 = lmin(cell_r1, rb);
      const bool rows_whole = g == cell_r0 && r1 == cell_r1;
      ColAcc acc;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc.s[e] = 0.0;
        acc.mn[e] = __builtin_inff();
        acc.mx[e] = -__builtin_inff();
      }
      acc.nan = 0u;
      const float* p = a.origin + (g - a.ox) * a.pitch + c0;
      const bool vec = a.vector_rows != 0;
      int64_t r = g;
      for (; r + 4 <= r1; r += 4) {
        const float4 v0 = load_cols(p, emask, vec);
        const float4 v1 = load_cols(p + a.pitch, emask, vec);
        const float4 v2 = load_cols(p + 2 * a.pitch, emask, vec);
        const float4 v3 = load_cols(p + 3 * a.pitch, emask, vec);
        acc_row(acc, v0, emask);
        acc_row(acc, v1, emask);
        acc_row(acc, v2, emask);
        acc_row(acc, v3, emask);
        p += 4 * a.pitch;
      }
      for (; r < r1; ++r) {
        const float4 v0 = load_cols(p, emask, vec);
        acc_row(acc, v0, emask);
        p += a.pitch;
      }
      g = r1;

      if constexpr (MODE == 0) {
        __shared__ double lsum[4][kCoarseStripCols];
        __shared__ int lmn[4][kCoarseStripCols], lmx[4][kCoarseStripCols];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool n = (acc.nan >> e) & 1u;
          lsum[wv][4 * lane + e] = acc.s[e];
          lmn[wv][4 * lane + e] = n ? kKeyNan : coarse_key(-acc.mn[e]);
          lmx[wv][4 * lane + e] = n ? kKeyNan : coarse_key(acc.mx[e]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int mis = int(c0 - 4 * lane - (ja * a.fy - a.oy));  // -(strip's misalignment)
        for (int t = lane; t < a.cells_per_strip; t += 64) {
          const int64_t J = ja + t;
          const int pos = t * int(a.fy) - mis;
          double s = 0.0;
          int kn = kKeyLowest, kx = kKeyLowest;
          bool any = false;
          for (int k = 0; k < int(a.fy); ++k) {
            const int64_t gc = J * a.fy + k;
            if (gc >= glo && gc < ghi) {
              any = true;
              s += lsum[wv][pos + k];
              kn = max(kn, lmn[wv][pos + k]);
              kx = max(kx, lmx[wv][pos + k]);
            }
          }
          if (any) emit(a, I, J, rows_whole, s, kn, kx);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      } else {
        double hs = 0.0, ts = 0.0;
        float hmn = __builtin_inff(), hmx = -__builtin_inff(), tmn = hmn, tmx = hmx;
        bool hn = false, tn = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool n = (acc.nan >> e) & 1u;
          if (e < eb) {
            hs += acc.s[e];
            hmn = fminf(hmn, acc.mn[e]);
            hmx = fmaxf(hmx, acc.mx[e]);
            hn |= n;
          } else {
            ts += acc.s[e];
            tmn = fminf(tmn, acc.mn[e]);
            tmx = fmaxf(tmx, acc.mx[e]);
            tn |= n;
          }
        }
        int hkn = hn ? kKeyNan : coarse_key(-hmn), hkx = hn ? kKeyNan : coarse_key(hmx);
        const int tkn = tn ? kKeyNan : coarse_key(-tmn), tkx = tn ? kKeyNan : coarse_key(tmx);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const int d = 1 << k;
          const double os = __shfl_down(hs, d);
          const int on = __shfl_down(hkn, d), ox_ = __shfl_down(hkx, d);
          if ((same >> k) & 1u) {
            hs += os;
            hkn = max(hkn, on);
            hkx = max(hkx, ox_);
          }
        }
        const double ps = __shfl_up(ts, 1);
        const int pn = __shfl_up(tkn, 1), px = __shfl_up(tkx, 1);
        if (prev_tail) {
          hs += ps;
          hkn = max(hkn, pn);
          hkx = max(hkx, px);
        }
        if (head && any_head) emit(a, I, jc, rows_whole, hs, hkn, hkx);
        // A tail that no later lane continues (the strip ends inside a cell).
        if (lane == 63 && any_tail) emit(a, I, jc + 1, rows_whole, ts, tkn, tkx);
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

int grid_1d(int64_t n) { return int(std::clamp<int64_t>(ceil_div(n, 256), 1, 4096)); }

void check_planes(const CoarsePlanes& p, int64_t cells) {
  HEAT_CHECK(p.sum && p.nmin_key && p.max_key && cells >= 0, "coarse planes");
}

}  // namespace

void coarse_set_max_waves(int waves) { g_max_waves.store(std::max(waves, 0)); }

void coarse_reset(const CoarsePlanes& p, int64_t cells, hipStream_t st) {
  check_planes(p, cells);
  if (cells == 0) return;
  hipLaunchKernelGGL(coarse_reset_kernel, dim3(grid_1d(cells)), dim3(256), 0, st, p, cells);
  HIP_CHECK(hipGetLastError());
}

void coarse_encode(const CoarsePlanes& p, int64_t cells, hipStream_t st) {
  check_planes(p, cells);
  if (cells == 0) return;
  hipLaunchKernelGGL(coarse_encode_kernel, dim3(grid_1d(cells)), dim3(256), 0, st, p, cells);
  HIP_CHECK(hipGetLastError());
}

void coarse_decode(const CoarsePlanes& p, int64_t cells, bool negated_min, hipStream_t st) {
  check_planes(p, cells);
  if (cells == 0) return;
  hipLaunchKernelGGL(coarse_decode_kernel, dim3(grid_1d(cells)), dim3(256), 0, st, p, cells,
                     int(negated_min));
  HIP_CHECK(hipGetLastError());
}

CoarsePlan coarse_plan(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                       int64_t oy, int64_t fx, int64_t fy) {
  CoarsePlan pl;
  HEAT_CHECK(lx >= 1 && ly >= 1 && ox >= 0 && oy >= 0 && fx >= 1 && fy >= 1,
             "coarse plan of a %lldx%lld block at (%lld, %lld), factors %lldx%lld", (long long)lx,
             (long long)ly, (long long)ox, (long long)oy, (long long)fx, (long long)fy);
  const uintptr_t addr = reinterpret_cast<uintptr_t>(origin);
  HEAT_CHECK(addr % 4 == 0, "field not 4-byte aligned");
  pl.vector_rows = pitch % 4 == 0;
  const int align = pl.vector_rows ? int((addr >> 2) & 3) : 0;
  const int64_t j0 = oy / fy, ncols = (oy + ly - 1) / fy - j0 + 1;
  const int64_t i0 = ox / fx, nrows = (ox + lx - 1) / fx - i0 + 1;
  // Strips of whole coarse columns: lane 0 starts on the 16-byte boundary at
  // or below the first cell, up to 3 columns early (the same for every strip
  // if fy is a multiple of 4).
  const int mis = !pl.vector_rows ? 0 : fy % 4 == 0 ? int((j0 * fy - oy + align) & 3) : 3;
  const int64_t cps = (kCoarseStripCols - mis) / fy;
  pl.owned = cps >= 1;
  if (pl.owned) {
    pl.cells_per_strip = int(std::min(cps, ncols));
    pl.strips = ceil_div(ncols, pl.cells_per_strip);
  } else {
    pl.strips = ceil_div(ly + align, kCoarseStripCols);
  }
  int cap = g_max_waves.load();
  if (cap <= 0) cap = device_cus() * kCoarseWavesPerCu;
  // Chunks: the longest that still give every wave of the launch a unit.
  for (int R = kCoarseMaxChunkRows;; R /= 2) {
    pl.chunk_rows = R;
    if (fx <= R) {
      pl.rows_per_chunk_cells = int(std::min<int64_t>(R / fx, nrows));
      pl.chunk_rows = int(pl.rows_per_chunk_cells * fx);
      pl.chunks = ceil_div(nrows, pl.rows_per_chunk_cells);
      pl.pieces = 1;
    } else {
      pl.rows_per_chunk_cells = 0;
      pl.chunks = ceil_div(lx, R);
      pl.pieces = int(std::min<int64_t>(ceil_div(fx, R), pl.chunks));
    }
    pl.units = pl.strips * pl.chunks;
    if (pl.units >= cap || R <= kCoarseMinChunkRows) break;
  }
  pl.waves = int(std::min<int64_t>(pl.units, cap));
  return pl;
}

void coarse_block(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                  int64_t oy, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
                  const CoarsePlanes& planes, hipStream_t st) {
  if (lx <= 0 || ly <= 0) return;
  HEAT_CHECK(fx >= 1 && fy >= 1 && ox >= 0 && oy >= 0 && ox + lx <= nx && oy + ly <= ny &&
                 pitch >= ly,
             "coarse of a %lldx%lld block at (%lld, %lld) of a %lldx%lld plate, factors %lldx%lld",
             (long long)lx, (long long)ly, (long long)ox, (long long)oy, (long long)nx,
             (long long)ny, (long long)fx, (long long)fy);
  check_planes(planes, 0);
  const int64_t cc = ceil_div(ny, fy);
  // A factor beyond the plate is the plate: one coarse row / column either way.
  fx = std::min(fx, nx);
  fy = std::min(fy, ny);
  const CoarsePlan pl = coarse_plan(origin, pitch, lx, ly, ox, oy, fx, fy);
  CoarseArgs a{};
  a.origin = origin;
  a.pitch = pitch;
  a.lx = lx;
  a.ly = ly;
  a.ox = ox;
  a.oy = oy;
  a.nx = nx;
  a.ny = ny;
  a.fx = fx;
  a.fy = fy;
  a.cc = cc;
  a.planes = planes;
  a.strips = pl.strips;
  a.units = pl.units;
  a.j0 = oy / fy;
  a.i0 = ox / fx;
  a.align = pl.vector_rows ? int((reinterpret_cast<uintptr_t>(origin) >> 2) & 3) : 0;
  a.owned = int(pl.owned);
  a.cells_per_strip = pl.cells_per_strip;
  a.chunk_rows = pl.chunk_rows;
  a.cells_per_chunk = pl.rows_per_chunk_cells;
  a.vector_rows = int(pl.vector_rows);
  const dim3 grid(unsigned(ceil_div(pl.waves, 4)));
  if (fy < 4) {
    HEAT_CHECK(pl.owned, "coarse plan");
    hipLaunchKernelGGL(coarse_kernel<0>, grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(coarse_kernel<1>, grid, dim3(256), 0, st, a);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace heat::gpu
