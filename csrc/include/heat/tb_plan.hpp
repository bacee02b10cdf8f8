// Launch planning of the temporally blocked kernels (host side, no GPU code):
// the variant flags and tuning knobs, the plan of a streaming launch
// (tb_step), and the shape search of the workgroup tiles (tb_tile.hip,
// tb_resident.hip, resident_shape_static).  Everything here is integer
// arithmetic on boxes: device facts (SIMDs, CUs, resident waves, occupancies)
// come in as arguments, so the self-test runs the planners without a GPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "heat/common.hpp"
#include "heat/topology.hpp"

namespace heat::gpu {

// Variant flags of the temporally blocked kernel (tb_step's `variant`; the
// same names in parallel_heat_amd.ops.TbVariant).  Bits 0-1 choose the
// register pipeline, the rest the build and the launch layout.
namespace tbv {
enum : int {
  kRing3 = 0,           // 3-row rings, skew 1 (LAG 1)
  kRing4 = 1,           // 4-row rings, skew 2 (LAG 2)
  kRing2 = 2,           // 2-row rings + copy (LAG 0)
  kRamp = 3,            // 3-row rings + compile-time ramp skip (LAG 3)
  kPipeMask = 3,
  kScalar = 4,          // scalar row update build (tbs; depth 12 lives here)
  kPrefetch6 = 8,       // with kRamp: 6-row prefetch (retired, LAG 4)
  kXcdGroups = 16,      // contiguous wave ranges per XCD
  kAltDirection = 32,   // odd chunks stream bottom-up
  kFloat2 = 64,         // float2 lanes, 128-column strips (tbn)
  kForceAgePairs = 256, // age groups even at equal weights (tests)
  kDiagNoStore = 1024,  // diagnostics: no output stores (wrong results)
  kSplit = 2048,        // two-wave level-split pipelines (tbx; depths 8, 12)
  kDiagCachedRows = 4096,  // diagnostics: cache-resident input rows (wrong results)
  kNoAgePairs = 16384,  // never age-group (A/B of the weights)
  kLinear = 32768,      // force the balanced linear plan (equal strip-rows per unit)
  kNoLinear = 65536,    // never switch to it (by default it replaces a classic
                        // plan that fills < 90 % of the launch's units)
  kTile = 131072,       // workgroup tiles: 8 waves x R rows of a strip in VGPRs,
                        // neighbour rows through LDS each step (tbw, tb_tile.hip)
  kTileDpp = 262144,    // with kTile: DPP lane shifts instead of ds_bpermute
  kShiftMixed = 524288, // with kSplit: west shift DPP, east ds_bpermute (tbxm, tb_split_mixed.hip)
  // Defaults: depth <= 8 and small launches at 12; large launches at 12.
  kDefault = kRamp | kScalar | kXcdGroups,  // 23
  kDefaultDeep = kDefault | kSplit,         // 2071
};
}  // namespace tbv

// Depths the temporally blocked kernel is instantiated for.
constexpr int kTbMaxDepth = 8;    // 1..8: every build
// Rows of the older : younger wave of a chunk pair at two waves per SIMD
// (kTbAgePairs; HEAT_TB_AGE_RATIO sets it, <= 1 = off).  Off by default: it
// evens the two waves' finish times (busy fraction 0.77 -> 0.81) but not the
// launch span, which the SIMD's combined issue rate sets
// (profiles/tb_wave_timeline_r1.md).
constexpr double kTbAgeRatio = 1.0;
// Level-split pipelines at two per SIMD: the first-dispatched half of the
// grid takes 1.7x the rows of the second half in each pair of adjacent
// chunks: +4-7 % at 2048..8192-row blocks (profiles/tb_split_age_pairs_r2.md).
constexpr double kTbSplitAgeWeights[2] = {1.7, 1.0};
// Linear plans of split pipelines at four blocks per CU: one share per
// dispatch round (oldest first).
constexpr double kTbLinearAgeWeights[4] = {2.0, 1.95, 1.15, 1.0};
constexpr int kTbDeepDepth = 12;  // + 12: scalar ring-3+ramp build (variant bits 4|3)
bool tb_depth_supported(int k);
// Output columns per 256-column strip at depth k.
// Output columns per TB strip (64 lanes x lane_cols, minus the overlap) and
// the lane width of a variant (4: float4 lanes; variant bit 64: float2).
int tb_strip_width(int k, int lane_cols = 4);
int tb_lane_cols(int variant);
int tb_variant_lag(int variant);
// The variant's build has the kTbDeepDepth instantiation (scalar ring-3+ramp).
bool tb_variant_deep(int variant);
// Bit 2048: each (strip, chunk) runs on a two-wave level-split pipeline
// (depths 8 and 12; scalar ring-3+ramp variants only).
bool tb_variant_split(int variant);
// Launch-planner knobs of the TB kernel.  Defaults are the tuned values;
// each HEAT_TB_* environment variable overrides its field when the process
// first plans a launch (diagnostics and A/B sweeps), and tb_set_tuning()
// replaces the whole set at run time (tests, tools).
struct TbTuning {
  int variant = -1;        // HEAT_TB_VARIANT: force a variant (-1: per launch)
  int rounds = 0;          // HEAT_TB_ROUNDS: whole resident rounds per launch (0: from the work)
  int min_len = 0;         // HEAT_TB_MINLEN: minimum chunk rows (0: max(depth, 8))
  int waves = 0;           // HEAT_TB_WAVES: waves per launch of the solver (0: planner)
  double edge_frac = 1.0;  // HEAT_TB_EDGE_FRAC: top/bottom edge chunk length factor
  // HEAT_TB_AGE_WEIGHTS "w0,w1,.." (or HEAT_TB_AGE_RATIO r = {r, 1}): row
  // shares of the age groups; empty = the built-in weights.
  std::vector<double> age_weights;
  int tile_rows = 0;       // HEAT_TB_TILE_ROWS: rows per wave of kTile launches (0: planner)
  int tile_waves = 0;      // HEAT_TB_TILE_WAVES: waves per kTile workgroup, 8 or 16 (0: planner)
  int tile_xl = -1;        // HEAT_TB_TILE_XL: kTile lane shifts, 0 DPP, 1 ds_bpermute,
                           // 2 mixed (-1: mixed unless the variant has kTileDpp)
  int tile_max_srps = 64;  // HEAT_TB_TILE_MAX: workgroup tiles below this many strip-rows
                           // per SIMD (the automatic variant and Solver::tile_sized)
  int nt = -1;             // HEAT_TB_NT: level-split rows non-temporal (1) or plain (0);
                           // -1: non-temporal when a pass sweeps > kTbStreamBytes
  int res_diag = 0;        // HEAT_TB_RES_DIAG: resident-tile timing diagnostics (bits 0-2
                           // give WRONG results): bit 0 no neighbour wait, 1 no ghost reload,
                           // 2 no publish; bit 3 every tile on the masked (edge) path
};
// Waves per SIMD the planner uses for a launch with this much work per SIMD
// (strip-rows / SIMDs), at most max_per_simd.
int tb_auto_waves_per_simd(int depth, int64_t strip_rows_per_simd, int max_per_simd);

namespace tbdetail {

struct TbBox {
  int64_t r0, r1, c0, c1;
  int nstrips, nchunks, chunk_len, wave_begin;
  int64_t lin0;  // linear plans: strip-rows of the boxes before this one
};

constexpr int kMaxBoxes = 16;
// Box B in strips of W output columns.
inline void set_strips(TbBox& t, const Box& B, int W) {
  t.r0 = B.r0, t.r1 = B.r1, t.c0 = B.c0, t.c1 = B.c1;
  t.nstrips = int(ceil_div(B.cols(), W));
}

// Launch-time layout options (variant bits 16 and 32, see tb_step):
//   kTbXcdGroups     remap blocks so each XCD (blocks b, b+8, ... under the
//                    observed round-robin placement) gets a contiguous range
//                    of waves: vertically adjacent chunks share one L2.
//   kTbAltDirection  odd chunks stream bottom-up, so the 2K halo rows two
//                    adjacent chunks both read are read at about the same
//                    time (both at the start or both at the end).
constexpr int kTbXcdGroups = 1;
constexpr int kTbAltDirection = 2;
//   kTbAgePairs      age groups: the G blocks a CU holds (dispatch rounds:
//                    grid part a = round a) split each group of G adjacent
//                    chunks unevenly, older (earlier-dispatched) blocks taking
//                    more rows: the SIMD's issue arbitration favours older
//                    waves, so with equal chunks the youngest set the launch
//                    tail (tools/wave_timeline.py by_age_rank,
//                    profiles/tb_split_age_pairs_r2.md).
constexpr int kTbAgePairs = 4;
//   kTbDiagNoStore   diagnostics: skip the output stores (wrong results; a
//                    timing probe of the store traffic; variant bit 1024).
constexpr int kTbDiagNoStore = 8;
//   kTbDiagCachedRows diagnostics: every input row load reads one of the
//                    chunk's first 4 rows (cache-resident; wrong results, a
//                    probe of load latency; variant bit 4096).
constexpr int kTbDiagCachedRows = 16;
//   kTbLinear        balanced plan: unit u takes strip-rows [u, u+1) * total /
//                    units of the box sequence (variant bit 32768), so every
//                    SIMD gets the same work whatever the shape; a unit may
//                    run several segments (strip / box / Dirichlet-mode ends).
constexpr int kTbLinear = 32;
//   kTbStreamRows    level-split launches take the streaming build
//                    (tb_split_nt.hip: non-temporal row loads and stores)
//                    when one pass sweeps more than the MALL holds
//                    (kTbStreamBytes, HEAT_TB_NT overrides).
constexpr int kTbStreamRows = 64;

}  // namespace tbdetail

// Field bytes one pass must sweep before the level-split launches stream
// their rows (kTbStreamRows): 3/4 of the 256 MB MALL (4096 x 8192 = 134 MB
// measured faster plain, 8192^2 = 268 MB non-temporal).
constexpr int64_t kTbStreamBytes = int64_t(192) << 20;

// --------------------------------------------------------------------------
// The streaming launch (tb_step)
// --------------------------------------------------------------------------

// The variant choices of kernels.hpp with the tuning as an argument.
int tb_default_variant(int depth, const TbTuning& tune);
int tb_auto_variant(int depth, int64_t strip_rows_per_simd, const TbTuning& tune);
// The variant of a tb_step launch over `boxes` asked with `requested` (-1:
// the automatic choice from the work per SIMD; an even depth the streaming
// builds lack stays on the tiles).  A kTile variant at an odd depth comes
// back as the default single-wave streaming build with the other bits kept,
// so a returned variant has kTile at even depths only.
int tb_choose_variant(int requested, int depth, const Box* boxes, int nbox, int simds,
                      const TbTuning& tune);

// What tb_step copies into the kernel arguments (tbdetail::TbArgs), and what
// its trace line prints.  nbox == 0: nothing to launch.
struct TbPlan {
  tbdetail::TbBox box[tbdetail::kMaxBoxes] = {};
  int nbox = 0;
  int total_waves = 0;  // units of one age group (TbArgs::total_waves)
  int flags = 0;        // tbdetail::kTb*
  int age_groups = 0;
  int age_cum[5] = {0, 0, 0, 0, 0};
  int64_t lin_total = 0, lin_slack = 0;
  // The trace line (and the stamp buffer's size check).
  int variant = 0;       // as given
  int waves_target = 0;  // resolved: > 0
  int bpc = 0;           // blocks per CU (0: waves_target or rounds given)
  int units = 0;         // waves or pipelines of the launch, all age groups
  int64_t total_strip_rows = 0;
};
// The plan of a streaming launch of the resolved (non-tile) `variant`:
// gx0, nx, pitch: the StencilGeom fields; waves_target as tb_step's;
// resident_waves: tb_resident_waves(depth, variant), read only when
// waves_target <= 0.
TbPlan tb_plan_launch(int variant, int depth, const Box* boxes, int nbox, int64_t gx0, int64_t nx,
                      int64_t pitch, int waves_target, int resident_waves, int simds,
                      const TbTuning& tune);
// The plan's HEAT_TB_TRACE line.
void tb_plan_trace_line(char (&line)[320], int depth, const TbPlan& p);

// --------------------------------------------------------------------------
// Workgroup tiles (tb_tile.hip, tb_resident.hip)
// --------------------------------------------------------------------------
namespace tbw {

// Issue estimate of one step of a tile launch (shape planning): the row
// updates of the busiest SIMD -- dispatch spreads workgroups over the CUs,
// `occ` at most per CU -- times the cycles per row-update op at that SIMD's
// wave count (2.7 with >= 4 waves, 3.1 with fewer: tools/probes/valu_rate.hip
// and the tile sweeps).  A CU with two tiles where others have one sets the
// pace of the launch (of the whole resident grid, through the neighbour
// waits): 468 tiles of 13 x 8 rows ran 10 % slower than 252 of 12 x 16 on a
// 1024 x 8192 block (profiles/r4_resident.md).
inline double tile_step_estimate(int64_t units, int cus, int occ, int rows, int waves) {
  const int64_t cap = int64_t(cus) * occ;
  const int64_t full = (units - 1) / cap;              // full dispatch rounds
  const int64_t last = units - full * cap;             // tiles of the last round
  const int64_t busiest = (last + cus - 1) / cus;      // tiles on its busiest CU
  auto cost = [&](int64_t tiles) {
    const double wps = double(tiles * waves) / 4.0;    // waves per SIMD
    return wps * rows * (wps >= 4.0 ? 2.7 : 3.1);
  };
  return double(full) * cost(occ) + cost(busiest);
}

// A tile is one 256-column strip by `waves` waves x `rows` rows.
struct TileShape {
  int rows, waves;
};
// The instantiated shapes: of the per-pass tiles, and of the resident tiles
// with the co-resident workgroups per CU the occupancy API reports for them
// on gfx950 (resident_shape_static; also RES_SHAPES of parallel/model.py).
constexpr TileShape kTileShapes[] = {{12, 8}, {13, 8}, {14, 8}, {16, 8}, {20, 8},
                                     {24, 8}, {28, 8}, {32, 8}, {12, 16}, {20, 16}};
constexpr TileShape kResidentShapes[] = {{12, 8}, {13, 8}, {14, 8}, {16, 8},
                                         {20, 8}, {24, 8}, {12, 16}, {20, 16}};
constexpr int kResidentOccGfx950[] = {2, 2, 2, 2, 1, 1, 1, 1};
static_assert(sizeof kResidentShapes / sizeof *kResidentShapes ==
              sizeof kResidentOccGfx950 / sizeof *kResidentOccGfx950);

// Useful rows of a tile: its rows less the K-deep ghost ring above and below.
inline int64_t tile_useful_rows(int rows, int waves, int depth) {
  return int64_t(waves) * rows - 2 * int64_t(depth);
}

struct TilePlan {
  int rows = 0, waves = 0;  // rows == 0: no shape fits
  int64_t units = 0;
  double est = 0.0;
};
// The shape search: among the shapes that pass the tuning's filters
// (tile_rows / tile_waves > 0: that value only), whose useful rows are at
// least max(depth, 4) and whose build exists (occ(i) > 0: resident
// workgroups per CU of shapes[i], asked only for shapes that got this far),
// the first with the lowest tile_step_estimate.  one_round: only shapes whose
// tiles are all co-resident.
template <class Occ, int N>
TilePlan tile_shape_search(const Box* boxes, int nbox, int depth, int cus, const TileShape (&shapes)[N],
                           Occ&& occ, int tile_rows, int tile_waves, bool one_round) {
  const int W = tb_strip_width(depth, 4);
  TilePlan best;
  for (int i = 0; i < N; ++i) {
    const TileShape& sh = shapes[i];
    if (tile_rows > 0 && sh.rows != tile_rows) continue;
    if (tile_waves > 0 && sh.waves != tile_waves) continue;
    const int64_t hmax = tile_useful_rows(sh.rows, sh.waves, depth);
    if (hmax < std::max(depth, 4)) continue;
    int64_t units = 0;
    for (int b = 0; b < nbox; ++b)
      if (!boxes[b].empty()) units += ceil_div(boxes[b].cols(), W) * ceil_div(boxes[b].rows(), hmax);
    const int o = occ(i);
    if (o <= 0 || (one_round && units > int64_t(cus) * o)) continue;
    const double est = tile_step_estimate(units, cus, o, sh.rows, sh.waves);
    if (best.rows == 0 || est < best.est) best = TilePlan{sh.rows, sh.waves, units, est};
  }
  return best;
}

// Every tile of a strip but the last is at least K rows deep (resident
// tiles: a ghost ring comes from the direct neighbours only).
inline bool tiles_at_least_depth(int64_t box_rows, const TilePlan& pl, int depth) {
  const int64_t hmax = tile_useful_rows(pl.rows, pl.waves, depth);
  return ceil_div(box_rows, ceil_div(box_rows, hmax)) >= depth;
}

// The resident plan of a box: the one-round search over kResidentShapes
// (rows == 0: none, or the box or depth is not one the resident tiles take).
template <class Occ>
TilePlan resident_tile_plan(const Box& box, int depth, int cus, Occ&& occ, int tile_rows = 0,
                            int tile_waves = 0) {
  if (box.empty() || depth < 4 || depth % 2 != 0 || box.c0 % 4 != 0) return {};
  return tile_shape_search(&box, 1, depth, cus, kResidentShapes, occ, tile_rows, tile_waves, true);
}

// Box B as tiles of the shape: strips, tiles per strip (nchunks), useful rows
// per tile (chunk_len) and the box's first unit.  Returns its units.
inline int64_t tile_fill_box(tbdetail::TbBox& t, const Box& B, int depth, const TilePlan& pl,
                             int64_t first_unit) {
  tbdetail::set_strips(t, B, tb_strip_width(depth, 4));
  t.nchunks = int(ceil_div(B.rows(), tile_useful_rows(pl.rows, pl.waves, depth)));
  t.chunk_len = int(ceil_div(B.rows(), int64_t(t.nchunks)));
  t.wave_begin = int(first_unit);
  return int64_t(t.nstrips) * t.nchunks;
}


// The HEAT_TB_TRACE lines of a tile launch (xl: its lane shifts; box0: the
// first filled box) and of a resident launch.
void tile_trace_line(char (&line)[200], int depth, const TilePlan& pl, int xl, int nbox,
                     int64_t units, const tbdetail::TbBox& box0);
void resident_trace_line(char (&line)[200], int depth, int passes, const TilePlan& pl, int xl);

}  // namespace tbw
}  // namespace heat::gpu
