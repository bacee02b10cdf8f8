// gfx950 (CDNA4) stencil kernels: device init, naive oracle step, the
// register-streaming temporally blocked step (the hot kernel), residual and
// halo pack/unpack.
//
// Design notes (MI355X-first):
//  * Layout is row-major with y contiguous, so a wave64 covers 64 consecutive
//    float4 = 256 columns of one row: every global access is a fully
//    coalesced 1 KiB dwordx4 wave-instruction (the reference maps threadIdx.x
//    to the strided x index, cuda/cuda_heat.cu:46-59, and is uncoalesced).
//  * The hot kernel (tb_kernel) streams a wave down a 256-column strip and
//    keeps K time levels of a 3-row sliding window in VGPRs.  Each input row
//    is loaded from HBM once and leaves after K fused updates, so HBM traffic
//    per cell-update is 8/K bytes instead of 8.  East/west neighbours cross
//    lanes with DPP wave_shr:1 / wave_shl:1 (fused into v_add_f32_dpp): no
//    LDS, no barriers, waves are fully independent.  Strips overlap by
//    2*round_up(K,4) columns and row chunks by 2K rows (redundant halo
//    compute, the trapezoid of classic temporal blocking).
//  * All variants evaluate the identical FMA expression (heat::stencil), so
//    results are bitwise equal across kernels, depths and decompositions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "heat/common.hpp"
#include "heat/init_fn.hpp"
#include "heat/kernels.hpp"
#include "tb_common.hpp"
#include "tb_exp.hpp"
#include "tb_tile.hpp"

namespace heat::gpu {
namespace {

using tbdetail::in_interior;
using tbdetail::TbArgs;
using tbdetail::TbBox;
using tbdetail::wave_max_atomic;

// --------------------------------------------------------------------------
// init
// --------------------------------------------------------------------------
__global__ void init_kernel(float* base, int64_t pitch, int64_t rows, int64_t hx, int64_t hy,
                            int64_t gx0, int64_t gy0, int64_t nx, int64_t ny, int mode,
                            uint64_t seed) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= pitch) return;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const int64_t gx = gx0 + r - hx, gy = gy0 + c - hy;
    base[r * pitch + c] = init_value(mode, gx, gy, nx, ny, seed);
  }
}

// --------------------------------------------------------------------------
// naive: one cell per thread (independent oracle for the TB kernel)
// --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void naive_kernel(const float* __restrict__ src,
                                                    float* __restrict__ dst, StencilGeom g,
                                                    Box box, unsigned* resid) {
  const int64_t c = box.c0 + int64_t(blockIdx.x) * 64 + threadIdx.x;
  const int64_t r = box.r0 + int64_t(blockIdx.y) * 4 + threadIdx.y;
  if (tbdetail::gated(g.gate)) return;
  unsigned m = 0;
  if (r < box.r1 && c < box.c1) {
    const int64_t i = r * g.pitch + c;
    const float v = src[i];
    float out = v;
    if (in_interior(g.gx0 + r, g.nx) && in_interior(g.gy0 + c, g.ny))
      out = g.numerics == 1
                ? stencil_mpi(v, src[i - g.pitch], src[i + g.pitch], src[i - 1], src[i + 1], g.cx, g.cy)
                : stencil(v, src[i - g.pitch], src[i + g.pitch], src[i - 1], src[i + 1], g.cx, g.cy);
    dst[i] = out;
    m = __float_as_uint(fabsf(out - v));
  }
  if (resid) wave_max_atomic(m, resid);
}

// --------------------------------------------------------------------------
// pack / unpack / residual
// --------------------------------------------------------------------------
__global__ void pack_kernel(const float* __restrict__ origin, int64_t pitch, Box box,
                            float* __restrict__ buf) {
  const int64_t cols = box.c1 - box.c0, n = (box.r1 - box.r0) * cols;
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n;
       k += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = k / cols, c = k % cols;
    buf[k] = origin[(box.r0 + r) * pitch + box.c0 + c];
  }
}

struct BoxCopies {
  BoxCopy c[kMaxBoxCopies];
};

// blockIdx.y selects the box; rows are grid-strided over blockIdx.x, columns
// over the threads (row segments are contiguous in both the field and the
// buffer).
__global__ __launch_bounds__(128) void box_copy_kernel(float* __restrict__ origin, int64_t pitch,
                                                       BoxCopies a, int to_buf) {
  const BoxCopy& c = a.c[blockIdx.y];
  const int64_t rows = c.box.r1 - c.box.r0, cols = c.box.c1 - c.box.c0;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    float* f = origin + (c.box.r0 + r) * pitch + c.box.c0;
    float* b = c.buf + r * cols;
    for (int64_t j = threadIdx.x; j < cols; j += blockDim.x) {
      if (to_buf) b[j] = f[j];
      else f[j] = b[j];
    }
  }
}

__global__ void unpack_kernel(const float* __restrict__ buf, float* __restrict__ origin,
                              int64_t pitch, Box box) {
  const int64_t cols = box.c1 - box.c0, n = (box.r1 - box.r0) * cols;
  for (int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; k < n;
       k += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = k / cols, c = k % cols;
    origin[(box.r0 + r) * pitch + box.c0 + c] = buf[k];
  }
}

__global__ __launch_bounds__(256) void residual_kernel(const float* __restrict__ a,
                                                       const float* __restrict__ b,
                                                       int64_t pitch, Box box, unsigned* resid) {
  const int64_t c = box.c0 + int64_t(blockIdx.x) * 64 + threadIdx.x;
  unsigned m = 0;
  if (c < box.c1)
    for (int64_t r = box.r0 + blockIdx.y * 4 + threadIdx.y; r < box.r1; r += gridDim.y * 4)
      m = max(m, __float_as_uint(fabsf(a[r * pitch + c] - b[r * pitch + c])));
  wave_max_atomic(m, resid);
}

__global__ void judge_kernel(unsigned* resids, int n, int slots, int stride, DeviceGate* gate,
                             double eps, int mpi_compat) {
  // One wave: lane s reads (and zeroes) slot s of every check -- all loads
  // issued before the first use --, the max over the slots is a wave
  // reduction, lane 0 judges.  Checks in order: the first converging one
  // closes the gate.
  constexpr int kMax = 32;  // kTbResidentMaxChecks; longer lists loop
  const int lane = threadIdx.x;
  for (int i0 = 0; i0 < n; i0 += kMax) {
    const int m = min(n - i0, kMax);
    unsigned v[kMax];
#pragma unroll
    for (int j = 0; j < kMax; ++j) v[j] = (j < m && lane < slots) ? resids[lane * stride + i0 + j] : 0u;
#pragma unroll
    for (int j = 0; j < kMax; ++j)
      if (j < m && lane < slots) resids[lane * stride + i0 + j] = 0u;
    // The gate in registers for the whole list (a read-modify-write of the
    // gate in memory per check serialised ~0.4 us per check: 10 us for the
    // 27 checks of a resident span).
    DeviceGate gl{};
    if (lane == 0) gl = *gate;
    for (int j = 0; j < m; ++j) {
      unsigned bits = v[j];  // non-negative floats order like their bits
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) bits = max(bits, unsigned(__shfl_xor(int(bits), off)));
      if (lane == 0 && gl.stop == 0u) {
        float r;
        __builtin_memcpy(&r, &bits, 4);
        const unsigned ordinal = gl.checks;
        gl.checks = ordinal + 1u;
        gl.last_bits = bits;
        unsigned why = 0u;
        if ((bits & 0x7F800000u) == 0x7F800000u) why = 2u;  // inf or NaN
        else if (mpi_compat ? double(r) <= eps : r < float(eps)) why = 1u;
        if (why) {
          gl.reason = why;
          gl.stop_check = ordinal;
          gl.stop = 1u;
        }
      }
    }
    if (lane == 0) *gate = gl;
  }
}

__device__ __forceinline__ int float_key(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : (i ^ 0x7FFFFFFF);
}

__global__ __launch_bounds__(256) void checksum_kernel(const float* __restrict__ origin,
                                                       int64_t pitch, int64_t lx, int64_t ly,
                                                       int64_t ox, int64_t oy, int64_t ny,
                                                       DeviceChecksum* out) {
  // Grid-stride over the block; every term is order-independent (wrapping
  // u64 sums, min/max), except the fp64 sum's last bits.  One set of
  // atomics per workgroup: a per-wave atomic on five hot addresses from
  // ~10^5 waves serialised at the memory side (30 ms for 8192^2).
  unsigned long long h = 0, cnt = 0;
  double sum = 0.0;
  int mn = 0x7FFFFFFF, mx = int(0x80000000);
  for (int64_t r = blockIdx.y; r < lx; r += gridDim.y) {
    const float* row = origin + r * pitch;
    const uint64_t gbase = uint64_t(ox + r) * uint64_t(ny) + uint64_t(oy);
    for (int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; c < ly;
         c += int64_t(gridDim.x) * blockDim.x) {
      const float v = row[c];
      const uint32_t bits = __float_as_uint(v);
      h += mix64((gbase + uint64_t(c)) * 0x100000001B3ull ^ bits);
      sum += double(v);
      const int k = float_key(v);
      mn = min(mn, k);
      mx = max(mx, k);
      ++cnt;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    h += __shfl_xor(h, off);
    cnt += __shfl_xor(cnt, off);
    sum += __shfl_xor(sum, off);
    mn = min(mn, __shfl_xor(mn, off));
    mx = max(mx, __shfl_xor(mx, off));
  }
  __shared__ unsigned long long sh_h[4], sh_c[4];
  __shared__ double sh_s[4];
  __shared__ int sh_mn[4], sh_mx[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh_h[w] = h;
    sh_c[w] = cnt;
    sh_s[w] = sum;
    sh_mn[w] = mn;
    sh_mx[w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < int(blockDim.x >> 6); ++i) {
      h += sh_h[i];
      cnt += sh_c[i];
      sum += sh_s[i];
      mn = min(mn, sh_mn[i]);
      mx = max(mx, sh_mx[i]);
    }
    if (cnt) {
      atomicAdd(&out->hash, h);
      atomicAdd(&out->count, cnt);
      atomicAdd(&out->sum, sum);
      atomicMin(&out->min_key, mn);
      atomicMax(&out->max_key, mx);
    }
  }
}

int grid_1d(int64_t n) { return int(std::min<int64_t>(ceil_div(n, 256), 256 * 16)); }

}  // namespace

namespace {
TbTuning tuning_from_env() {
  TbTuning t;
  auto geti = [](const char* n, int def) {
    const char* e = std::getenv(n);
    return e && *e ? std::atoi(e) : def;
  };
  t.variant = geti("HEAT_TB_VARIANT", -1);
  t.rounds = std::max(0, geti("HEAT_TB_ROUNDS", 0));
  t.min_len = std::max(0, geti("HEAT_TB_MINLEN", 0));
  t.waves = std::max(0, geti("HEAT_TB_WAVES", 0));
  t.tile_rows = std::max(0, geti("HEAT_TB_TILE_ROWS", 0));
  t.tile_waves = std::max(0, geti("HEAT_TB_TILE_WAVES", 0));
  t.tile_xl = geti("HEAT_TB_TILE_XL", -1);
  t.res_diag = geti("HEAT_TB_RES_DIAG", 0) & 31;
  t.nt = geti("HEAT_TB_NT", -1);
  t.tile_max_srps = std::max(0, geti("HEAT_TB_TILE_MAX", 64));
  if (const char* e = std::getenv("HEAT_TB_EDGE_FRAC"); e && *e) t.edge_frac = std::atof(e);
  if (const char* e = std::getenv("HEAT_TB_AGE_WEIGHTS"); e && *e) {
    for (const char* q = e; *q;) {
      char* end = nullptr;
      const double v = std::strtod(q, &end);
      if (end == q) break;
      t.age_weights.push_back(v);
      q = *end == ',' ? end + 1 : end;
    }
  } else if (const char* r = std::getenv("HEAT_TB_AGE_RATIO"); r && *r) {
    t.age_weights = {std::atof(r), 1.0};
  }
  return t;
}
std::mutex g_tuning_mu;
TbTuning& tuning_ref() {
  static TbTuning t = tuning_from_env();
  return t;
}
}  // namespace

TbTuning tb_tuning() {
  std::lock_guard<std::mutex> lk(g_tuning_mu);
  return tuning_ref();
}

void tb_set_tuning(const TbTuning& t) {
  std::lock_guard<std::mutex> lk(g_tuning_mu);
  tuning_ref() = t;
}

int tb_default_rounds() { return tb_tuning().rounds; }

bool tb_trace_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("HEAT_TB_TRACE");
    return e && *e && *e != '0';
  }();
  return on;
}
void tb_trace_once(const char* line) {
  static std::mutex mu;
  static std::vector<std::string> seen;
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& s : seen)
    if (s == line) return;
  seen.emplace_back(line);
  std::fputs(line, stderr);
}

int tb_device_memo(TbMemo which, int a, int b, int c, int (*compute)(int, int, int)) {
  static std::map<std::tuple<int, int, int, int, int>, int> cache;
  static std::mutex mu;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const auto key = std::make_tuple(int(which), dev, a, b, c);
  {
    std::lock_guard<std::mutex> lk(mu);
    if (auto it = cache.find(key); it != cache.end()) return it->second;
  }
  const int v = compute(a, b, c);  // unlocked: it may ask the memo itself
  std::lock_guard<std::mutex> lk(mu);
  return cache.emplace(key, v).first->second;
}

int tb_simd_count() {
  return tb_device_memo(TbMemo::kSimds, 0, 0, 0, [](int, int, int) {
    int dev = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return std::max(1, cus) * 4;
  });
}

int tb_resident_waves(int depth, int variant) {
  // Cached per (device, depth, variant): CUs x resident blocks per CU x 4 waves.
  return tb_device_memo(TbMemo::kStreamWaves, depth, variant, 0, [](int depth, int variant, int) {
    const int cus = tb_simd_count() / 4;
    const int lag = tb_variant_lag(variant);
    if (tb_variant_split(variant)) {
      // Work units are two-wave pipelines, two per block.
      const int occ = (variant & tbv::kShiftMixed)
                          ? tb_exp("the mixed-shift split build (kShiftMixed)").tbxm_occupancy_split(depth)
                          : tbx::occupancy_split(depth);
      return std::max(1, cus * std::max(1, occ) * 2);
    }
    const int per_cu = (variant & tbv::kFloat2)  ? tb_exp("the float2-lane build (kFloat2)").tbn_occupancy(depth, lag)
                       : (variant & tbv::kScalar) ? tbs::occupancy(depth, lag)
                                                  : tb_exp("the packed build (no kScalar)").tbp_occupancy(depth, lag);
    return std::max(1, cus * std::max(1, per_cu) * 4);
  });
}

int tb_default_variant(int depth) { return tb_default_variant(depth, tb_tuning()); }

int tb_auto_variant(int depth, int64_t strip_rows_per_simd) {
  return tb_auto_variant(depth, strip_rows_per_simd, tb_tuning());
}

void init_field(float* origin, const Layout& L, int64_t gx0, int64_t gy0, int64_t nx, int64_t ny,
                int mode, uint64_t seed, hipStream_t st) {
  float* base = origin - L.origin();
  dim3 grid(unsigned(ceil_div(L.pitch, 256)), unsigned(std::min<int64_t>(L.rows, 1024)));
  hipLaunchKernelGGL(init_kernel, grid, dim3(256), 0, st, base, L.pitch, L.rows, int64_t(L.hx),
                     int64_t(L.hy), gx0, gy0, nx, ny, mode, seed);
  HIP_CHECK(hipGetLastError());
}

void naive_step(const float* src, float* dst, const StencilGeom& g, const Box& box,
                unsigned* resid, hipStream_t st) {
  if (box.empty()) return;
  dim3 grid(unsigned(ceil_div(box.cols(), 64)), unsigned(ceil_div(box.rows(), 4)));
  hipLaunchKernelGGL(naive_kernel, grid, dim3(64, 4), 0, st, src, dst, g, box, resid);
  HIP_CHECK(hipGetLastError());
}

namespace {
// Stamp buffers per device: with one host thread per GPU (`heat --gpus N`)
// each rank's launches stamp into its own device's buffer only.
struct Stamps {
  unsigned long long* buf = nullptr;
  int64_t waves = 0;
};
std::mutex g_stamps_mu;
std::map<int, Stamps> g_stamps;

Stamps stamps_of_current_device() {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_stamps_mu);
  auto it = g_stamps.find(dev);
  return it == g_stamps.end() ? Stamps{} : it->second;
}
}  // namespace

void tb_set_stamps(unsigned long long* buf, int64_t waves) {
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_stamps_mu);
  if (buf) g_stamps[dev] = Stamps{buf, waves};
  else g_stamps.erase(dev);
}

bool tb_mid_residual(int depth) {
  // Depth 12 under the automatic variant choice is always the level-split
  // pipelines (tb_split_rl*.hip) or the workgroup tiles (tb_tile.hip), which
  // take a residual at any inner step; forced variants keep the last step.
  return depth == kTbDeepDepth && tb_tuning().variant < 0;
}

namespace {
std::mutex g_exp_mu;
const TbExpKernels* g_exp = nullptr;
}  // namespace

bool tb_exp_loaded() {
  std::lock_guard<std::mutex> lk(g_exp_mu);
  return g_exp != nullptr;
}

const TbExpKernels& tb_exp(const char* what) {
  std::lock_guard<std::mutex> lk(g_exp_mu);
  HEAT_CHECK(g_exp != nullptr,
             "%s is an experiment kernel build: `make exp`, then load "
             "parallel_heat_amd/_lib/libheat_exp.so (HEAT_EXP=1)", what);
  return *g_exp;
}

// HEAT_TB_SPLIT_PK=1: the streaming level-split launches take the packed-f32
// build (round-6 A/B, an experiment build).
bool split_pk_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("HEAT_TB_SPLIT_PK");
    return e && *e && *e != '0';
  }();
  return on;
}

void tb_step(const float* src, float* dst, const StencilGeom& g, const Box* boxes, int nbox,
             int depth, unsigned* resid, hipStream_t st, int waves_target, int variant,
             int res_level, TbChain* chain) {
  if (chain) chain->chained = false;
  HEAT_CHECK(nbox >= 0 && nbox <= 5, "nbox=%d", nbox);  // API limit (5 boxes)
  HEAT_CHECK(res_level >= 0 && res_level <= depth, "residual level %d of a depth-%d pass",
             res_level, depth);
  if (res_level == depth || resid == nullptr) res_level = 0;  // 0: the last step
  const TbTuning tune = tb_tuning();
  const bool forced = variant >= 0 || tune.variant >= 0;
  const int simds = tb_simd_count();
  // The tile kernel takes any even depth up to 16 (Solver picks 10 for
  // checks every 10k steps on tile-sized blocks); the streaming kernels the
  // built ones.  A tile variant at an odd depth comes back as a streaming one.
  variant = tb_choose_variant(variant, depth, boxes, nbox, simds, tune);
  HEAT_CHECK(tb_depth_supported(depth) || ((variant & tbv::kTile) && depth <= 16),
             "unsupported TB depth %d (variant %d)", depth, variant);
  if (variant & tbv::kTile) {
    tbw::step(src, dst, g, boxes, nbox, depth, resid, res_level, st, variant, tune);
    return;
  }
  // Inner-level residuals: the level-split build at depth 12 (and the tiles).
  const bool split = tb_variant_split(variant);
  HEAT_CHECK(res_level == 0 || (split && depth == kTbDeepDepth),
             "a residual at step %d of a depth-%d pass needs the depth-12 level-split or tile "
             "kernel (variant %d%s)", res_level, depth, variant, forced ? ", forced" : "");
  const int lag = tb_variant_lag(variant);
  const int resident = waves_target <= 0 ? tb_resident_waves(depth, variant) : 0;
  const TbPlan plan = tb_plan_launch(variant, depth, boxes, nbox, g.gx0, g.nx, g.pitch, waves_target,
                                     resident, simds, tune);
  if (plan.nbox == 0) return;
  TbArgs args{};
  args.src = src;
  args.dst = dst;
  args.resid = resid;
  args.res_level = res_level > 0 ? res_level : depth;
  args.g = g;
  args.nbox = plan.nbox;
  args.total_waves = plan.total_waves;
  args.flags = plan.flags;
  args.age_groups = plan.age_groups;
  std::copy(std::begin(plan.age_cum), std::end(plan.age_cum), args.age_cum);
  args.lin_total = plan.lin_total;
  args.lin_slack = plan.lin_slack;
  std::copy(std::begin(plan.box), std::end(plan.box), args.box);
  if (tb_trace_enabled()) {
    // HEAT_TB_TRACE=1: each distinct plan once on stderr (planner checks).
    char line[320];
    tb_plan_trace_line(line, depth, plan);
    tb_trace_once(line);
  }
  if (const Stamps sb = stamps_of_current_device(); sb.buf) {
    const int64_t need = int64_t(plan.units) * (split ? 2 : 1);
    HEAT_CHECK(need <= sb.waves, "stamp buffer holds %lld waves, launch has %lld",
               (long long)sb.waves, (long long)need);
    args.stamps = sb.buf;
  }
  if (chain && chain->passes > 1) {
    // Chained passes: the streaming build's classic one-box plan of one
    // dispatch round (every unit resident: the units poll each other).
    // args.total_waves counts the units of one age group (launch_chain).
    const int G = (args.flags & tbdetail::kTbAgePairs) ? args.age_groups : 1;
    int blocks = (args.total_waves + 1) / 2;
    if (G > 1) blocks = (blocks + 7) / 8 * 8 * G;
    static const int occ = tb_exp("the chained build (HEAT_TB_CHAIN=1)").tbc_occupancy_chain(kTbDeepDepth);
    int dev = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const bool fits = split && !(variant & tbv::kShiftMixed) && (args.flags & tbdetail::kTbStreamRows) &&
                      !(args.flags & tbdetail::kTbLinear) && !(args.flags & tbdetail::kTbAltDirection) &&
                      plan.nbox == 1 && resid == nullptr && depth == kTbDeepDepth && args.stamps == nullptr &&
                      int64_t(args.total_waves) * G <= chain->max_units && blocks <= cus * occ;
    if (tb_trace_enabled()) {
      char line[320];
      std::snprintf(line, sizeof line,
                    "[heat chain] passes %d split %d mixed %d stream %d linear %d alt %d boxes %d resid %d "
                    "depth %d units %d x %d max %d blocks %d cus %d occ %d -> %d\n",
                    chain->passes, int(split), int((variant & tbv::kShiftMixed) != 0),
                    int((args.flags & tbdetail::kTbStreamRows) != 0),
                    int((args.flags & tbdetail::kTbLinear) != 0),
                    int((args.flags & tbdetail::kTbAltDirection) != 0), plan.nbox, int(resid != nullptr), depth,
                    args.total_waves, G, chain->max_units, blocks, cus, occ, int(fits));
      tb_trace_once(line);
    }
    if (fits) {
      chain->chained = tb_exp("the chained build (HEAT_TB_CHAIN=1)")
                           .tbc_launch_chain(args, depth, chain->passes, chain->flags, chain->done,
                                             chain->err, st);
      HIP_CHECK(hipGetLastError());
      return;
    }
  }
  bool ok;
  if (split) {
    if (variant & tbv::kShiftMixed)
      ok = tb_exp("the mixed-shift split build (kShiftMixed)").tbxm_launch_split(args, depth, st);
    else if (!(args.flags & tbdetail::kTbStreamRows))
      ok = tbx::launch_split(args, depth, st);
    else if (split_pk_enabled())
      ok = tb_exp("the packed split build (HEAT_TB_SPLIT_PK=1)").tbxnp_launch_split(args, depth, st);
    else
      ok = tbxn::launch_split(args, depth, st);
  } else if (variant & tbv::kFloat2) {
    ok = tb_exp("the float2-lane build (kFloat2)").tbn_launch(args, depth, lag, st);
  } else if (variant & tbv::kScalar) {
    ok = tbs::launch(args, depth, lag, st);
  } else {
    ok = tb_exp("the packed build (no kScalar)").tbp_launch(args, depth, lag, st);
  }
  HEAT_CHECK(ok, "TB depth %d is not instantiated for variant %d (depth %d: scalar ring-3+ramp only)",
             depth, variant, kTbDeepDepth);
  HIP_CHECK(hipGetLastError());
}

void pack_box(const float* origin, int64_t pitch, const Box& box, float* buf, hipStream_t st) {
  if (box.empty()) return;
  hipLaunchKernelGGL(pack_kernel, dim3(grid_1d(box.rows() * box.cols())), dim3(256), 0, st,
                     origin, pitch, box, buf);
  HIP_CHECK(hipGetLastError());
}

void copy_boxes(float* origin, int64_t pitch, const BoxCopy* copies, int n, bool to_buf,
                hipStream_t st) {
  HEAT_CHECK(n >= 0 && n <= kMaxBoxCopies, "copy_boxes: %d boxes", n);
  BoxCopies a{};
  int m = 0;
  int64_t rows = 0;
  for (int i = 0; i < n; ++i) {
    if (copies[i].box.empty()) continue;
    a.c[m++] = copies[i];
    rows = std::max(rows, copies[i].box.rows());
  }
  if (m == 0) return;
  dim3 grid(unsigned(std::min<int64_t>(rows, 2048)), unsigned(m));
  hipLaunchKernelGGL(box_copy_kernel, grid, dim3(128), 0, st, origin, pitch, a, int(to_buf));
  HIP_CHECK(hipGetLastError());
}

void unpack_box(const float* buf, float* origin, int64_t pitch, const Box& box, hipStream_t st) {
  if (box.empty()) return;
  hipLaunchKernelGGL(unpack_kernel, dim3(grid_1d(box.rows() * box.cols())), dim3(256), 0, st,
                     buf, origin, pitch, box);
  HIP_CHECK(hipGetLastError());
}

float checksum_key_to_float(int key) {
  const int i = key >= 0 ? key : (key ^ 0x7FFFFFFF);
  float f;
  std::memcpy(&f, &i, 4);
  return f;
}

void checksum_block(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                    int64_t oy, int64_t ny, DeviceChecksum* out, hipStream_t st) {
  if (lx <= 0 || ly <= 0) return;
  // ~8 workgroups per CU in total, grid-stride inside.
  const int64_t gx = std::min<int64_t>(ceil_div(ly, 256), 16);
  dim3 grid(unsigned(gx), unsigned(std::min<int64_t>(lx, std::max<int64_t>(1, 2048 / gx))));
  hipLaunchKernelGGL(checksum_kernel, grid, dim3(256), 0, st, origin, pitch, lx, ly, ox, oy, ny,
                     out);
  HIP_CHECK(hipGetLastError());
}

void judge_check(unsigned* resid, DeviceGate* gate, double eps, bool mpi_compat, hipStream_t st,
                 int n, int slots, int stride) {
  HEAT_CHECK(n >= 1 && slots >= 1 && slots <= 64 && (slots == 1 || stride >= n),
             "judge of %d checks x %d slots", n, slots);
  hipLaunchKernelGGL(judge_kernel, dim3(1), dim3(64), 0, st, resid, n, slots, stride, gate, eps,
                     int(mpi_compat));
  HIP_CHECK(hipGetLastError());
}

void residual_box(const float* a, const float* b, int64_t pitch, const Box& box, unsigned* resid,
                  hipStream_t st) {
  if (box.empty()) return;
  dim3 grid(unsigned(ceil_div(box.cols(), 64)),
            unsigned(std::min<int64_t>(ceil_div(box.rows(), 4), 1024)));
  hipLaunchKernelGGL(residual_kernel, grid, dim3(64, 4), 0, st, a, b, pitch, box, resid);
  HIP_CHECK(hipGetLastError());
}

}  // namespace heat::gpu

extern "C" void heat_register_exp_kernels(const heat::gpu::TbExpKernels* k) {
  std::lock_guard<std::mutex> lk(heat::gpu::g_exp_mu);
  heat::gpu::g_exp = k;
}
