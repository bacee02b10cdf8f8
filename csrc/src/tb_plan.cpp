// Launch planning of the temporally blocked kernels (see tb_plan.hpp).
#include "heat/tb_plan.hpp"

#include <cmath>
#include <cstdio>
#include <iterator>

namespace heat::gpu {

bool tb_depth_supported(int k) {
  // 1..8 in every build; 12 in the scalar ring-3+ramp build only
  // (tb_scalar.hip, HEAT_TB_DEEP).
  return (k >= 1 && k <= kTbMaxDepth) || k == kTbDeepDepth;
}

int tb_strip_width(int k, int lane_cols) {
  return 64 * lane_cols - 2 * int(round_up(k, lane_cols));
}
int tb_lane_cols(int variant) { return (variant & tbv::kFloat2) ? 2 : 4; }

int tb_variant_lag(int variant) {
  const int pipe = variant & tbv::kPipeMask;
  if (pipe == tbv::kRamp && (variant & tbv::kPrefetch6)) return 4;  // retired
  switch (pipe) {
    case tbv::kRing4: return 2;
    case tbv::kRing2: return 0;
    case tbv::kRamp: return 3;
    default: return 1;
  }
}

bool tb_variant_split(int variant) {
  // Level-split two-wave pipelines (tb_split.hip; scalar ring-3+ramp).
  return (variant & tbv::kSplit) && tb_variant_deep(variant);
}

bool tb_variant_deep(int variant) {
  return (variant & tbv::kScalar) && !(variant & tbv::kFloat2) && tb_variant_lag(variant) == 3;
}

int tb_auto_waves_per_simd(int depth, int64_t strip_rows_per_simd, int max_per_simd) {
  // Fewer, longer chunks for small problems: each chunk pays a ~2K-row
  // pipeline ramp, and more waves per SIMD only buy latency hiding.  The
  // thresholds come from the waves sweep over slab heights 512..8192
  // (tools/sweep_waves.sh, profiles/tb_waves_per_simd_r1.md): at K=8 one
  // wave per SIMD wins below ~48 strip-rows per SIMD, two below ~100.
  int w = max_per_simd;
  if (strip_rows_per_simd < 6 * int64_t(depth)) w = 1;
  else if (strip_rows_per_simd * 2 < 25 * int64_t(depth)) w = 2;
  return std::max(1, std::min(w, max_per_simd));
}

int tb_default_variant(int depth, const TbTuning& tune) {
  if (const int v = tune.variant; v >= 0) return v;
  // Ring-3 + ramp skip, scalar build, XCD-grouped blocks (23); at depth 12
  // on large launches as two-wave level-split pipelines with ds_bpermute
  // lane shifts (2071): +5 % in bench.py, +9-10 % in the interleaved kernel
  // A/B (profiles/tb_wave_timeline_r1.md).  tb_step picks per launch from
  // the work size (tb_auto_variant).
  return depth == kTbDeepDepth ? tbv::kDefaultDeep : tbv::kDefault;
}

int tb_auto_variant(int depth, int64_t strip_rows_per_simd, const TbTuning& tune) {
  if (const int v = tune.variant; v >= 0) return v;
  // The split pipelines need about 64 strip-rows per SIMD to pay for their
  // second wave: below that (the per-rank blocks of 4-8 GPU runs: 1024 x
  // 8192, 2048 x 4096, 1536 x 8192, ...) one wave per (strip, chunk) at
  // depth 12 is 8-12 % faster, above it the split is 2-4 % faster
  // (profiles/tb_block_shapes_r2.md).
  // Below 64 (the 8-GPU blocks 1024 x 8192 and 2048 x 4096 and their
  // deep-halo passes, 1536-row blocks) the workgroup tiles win: +6-10 % over
  // one wave per chunk inside the plate at 36, and +36-38 % on blocks with a
  // plate edge (the first and last rank, whose time the max over ranks
  // reports) at 36 and 54, where one wave per chunk loses 8 % inside the
  // plate (profiles/r3_tile.md).  Even depths only (the tile runs steps in
  // pairs).  From 64 the split pipelines keep the edge ranks within 2 %.
  if (depth >= 4 && depth % 2 == 0 && strip_rows_per_simd < tune.tile_max_srps)
    return tbv::kTile | tbv::kXcdGroups;
  if (depth == kTbDeepDepth && strip_rows_per_simd < 64) return tbv::kDefault;
  // Depth 8 on whole-GPU plates (the remainder passes of 1000 = 82 x 12 +
  // 8 + 8 at 8192^2: 288 strip-rows per SIMD) as split pipelines too:
  // bench 5.21-5.22 vs 5.19-5.21 interleaved (profiles/r5_stores.md).
  if (depth == 8 && strip_rows_per_simd >= 256) return tbv::kDefaultDeep;
  return tb_default_variant(depth, tune);
}

namespace {
// Strip-rows of the boxes in strips of W output columns.
int64_t strip_rows(const Box* boxes, int nbox, int W) {
  int64_t rows = 0;
  for (int b = 0; b < nbox; ++b)
    if (!boxes[b].empty()) rows += ceil_div(boxes[b].cols(), W) * boxes[b].rows();
  return rows;
}
// Age groups (kTbAgePairs) for launches of whole resident rounds: blocks
// dispatched earlier issue faster (the SIMD's arbitration favours older
// waves), so the grid is split into G parts (part a = the a-th share of
// the dispatch rounds) and older parts get more rows.  Default: two parts
// at kTbSplitAgeWeights for the level-split pipelines; none (kTbAgeRatio
// = 1) for single-wave pipelines.  HEAT_TB_AGE_WEIGHTS="w0,w1,..." (2-4
// parts) or HEAT_TB_AGE_RATIO=r (two parts r : 1) override; "1" = off.
// Four parts (one per round at 4 blocks per CU) measured slower than two
// whatever the weights (profiles/tb_split_age_pairs_r2.md).
// Returns G (0: none) and the row shares.
int age_groups_of(bool split_v, int max_groups, const TbTuning& tune, std::vector<double>& weights) {
  if (!tune.age_weights.empty())
    weights = tune.age_weights;
  else if (split_v)
    weights.assign(std::begin(kTbSplitAgeWeights), std::end(kTbSplitAgeWeights));
  else
    weights = {kTbAgeRatio, 1.0};
  bool uneven = false;
  for (double w : weights) uneven = uneven || w != weights[0] || w <= 0.0;
  const int n = int(weights.size());
  return uneven && n >= 2 && n <= max_groups ? n : 0;
}

// A classic plan with chunks of L rows (groups of G chunks with age groups):
// fills p.box / p.nbox and returns the waves.  Rows whose chunk window
// reaches the global top/bottom row run the generic (masked) path:
// HEAT_TB_EDGE_FRAC < 1 gives them shorter chunks, as separate sub-boxes.
// Default 1 (no edge sub-boxes) since the round-2 main loop: the edge chunks
// at 0.75 finished ~30 us before the rest of an 8192^2 launch; bench.py 1.0
// vs 0.95 / 0.9 / 0.75: +0.4 / +1.2 / +1.2 % (profiles/tb_edge_frac_r2.md).
int classic_plan(TbPlan& p, int64_t L, int64_t min_len, double edge_frac, int G, int W, int depth,
                 const Box* boxes, int nbox, int64_t gx0, int64_t nx) {
  const int64_t edge_len = std::max<int64_t>(std::min<int64_t>(min_len, L),
                                             int64_t(double(L) * edge_frac));
  int n = 0, waves = 0;
  auto add = [&](const Box& B, int64_t clen) {
    if (B.empty()) return;
    HEAT_CHECK(n < tbdetail::kMaxBoxes, "too many TB sub-boxes");
    tbdetail::TbBox& t = p.box[n++];
    tbdetail::set_strips(t, B, W);
    t.chunk_len = int(std::min<int64_t>(clen, B.rows()));
    t.nchunks = int(ceil_div(B.rows(), t.chunk_len));
    if (G > 0) {
      // Units are groups of G chunks (G * chunk_len rows), one wave (or
      // pipeline) of each age.
      t.chunk_len = int(std::max<int64_t>(1, ceil_div(std::min<int64_t>(G * clen, B.rows()), G)));
      t.nchunks = int(ceil_div(B.rows(), G * int64_t(t.chunk_len)));
    }
    t.wave_begin = waves;
    waves += t.nstrips * t.nchunks * std::max(G, 1);
  };
  for (int b = 0; b < nbox; ++b) {
    const Box& B = boxes[b];
    if (B.empty()) continue;
    Box mid = B, top{}, bot{};
    if (edge_len < L && B.rows() > 2 * L) {
      // Local rows whose window [r - depth, r + depth] touches global row 0 / nx-1.
      const int64_t top_end = 1 - gx0 + depth;         // first row clear of the top
      const int64_t bot_begin = nx - 2 - gx0 - depth;  // last row clear of the bottom
      if (B.r0 < top_end) {
        const int64_t e = std::min(B.r1, std::max(top_end, B.r0 + edge_len));
        top = Box{B.r0, e, B.c0, B.c1};
        mid.r0 = e;
      }
      if (B.r1 - 1 > bot_begin && mid.r1 > mid.r0) {
        const int64_t s0 = std::max(mid.r0, std::min(bot_begin + 1, B.r1 - edge_len));
        bot = Box{s0, B.r1, B.c0, B.c1};
        mid.r1 = s0;
      }
    }
    // Units in plate order (top edge, middle, bottom edge): XCD groups
    // take contiguous unit ranges, so the short edge units land on the
    // first and the last XCD instead of all on the first (which then
    // idled for the last ~15 % of the launch, tools/wave_timeline.py
    // xcd_last_end_us).
    add(top, edge_len);
    add(mid, L);
    add(bot, edge_len);
  }
  p.nbox = n;
  return waves;
}

}  // namespace

int tb_choose_variant(int requested, int depth, const Box* boxes, int nbox, int simds,
                      const TbTuning& tune) {
  int variant = requested;
  if (variant < 0) {
    // Both defaults use float4 lanes (same strip width).
    variant = tb_auto_variant(depth, strip_rows(boxes, nbox, tb_strip_width(depth, 4)) / simds, tune);
    // Even depths only the tile kernel builds (10, 14, 16: checks every 10k
    // steps on tile-sized blocks) stay on it whatever the launch size: a
    // deep-halo box grown past the tile threshold (Solver::tile_sized_at
    // judges the owned block) is still a valid tile launch, only slower.
    if (!tb_depth_supported(depth) && depth % 2 == 0 && depth <= 16)
      variant = tbv::kTile | tbv::kXcdGroups;
  }
  // The tile kernel runs steps in (down, up) pairs: even depths only; an
  // odd pass (a remainder or a check-cut pass) streams, with the default
  // single-wave build (scalar update + ramp; dropping only the tile bits
  // left the packed build, an experiment kernel since round 6).
  if ((variant & tbv::kTile) && depth % 2 != 0)
    variant = (variant & ~(tbv::kTile | tbv::kTileDpp | 3)) | tbv::kDefault;
  return variant;
}

TbPlan tb_plan_launch(int variant, int depth, const Box* boxes, int nbox, int64_t gx0, int64_t nx,
                      int64_t pitch, int waves_target, int resident_waves, int simds,
                      const TbTuning& tune) {
  TbPlan p;
  p.variant = variant;
  for (int b = 0; b < nbox; ++b)
    HEAT_CHECK(boxes[b].empty() || boxes[b].c0 % 4 == 0, "TB box column start %lld not a multiple of 4",
               (long long)boxes[b].c0);
  const int W = tb_strip_width(depth, tb_lane_cols(variant));
  const int64_t total_strip_rows = strip_rows(boxes, nbox, W);
  p.total_strip_rows = total_strip_rows;
  const bool split_v = tb_variant_split(variant);
  int G = 0;  // age groups of this launch (0: none)
  std::vector<double> weights;
  if ((variant & tbv::kForceAgePairs) && (G = age_groups_of(split_v, 4, tune, weights)) == 0) {
    G = 2;  // tests: even weights still group
    weights.assign(2, 1.0);
  }
  if (waves_target <= 0) {
    // Whole rounds of the resident wave capacity (a partial last round leaves
    // SIMDs idle for the tail of the launch); by default with the number of
    // waves per SIMD chosen from the work per SIMD.
    const int rounds = waves_target < 0 ? -waves_target : tune.rounds;
    if (rounds > 0) {
      waves_target = rounds * resident_waves;
    } else {
      const int per_simd = tb_auto_waves_per_simd(depth, total_strip_rows / simds,
                                                  std::max(1, resident_waves / simds));
      waves_target = simds * per_simd;
      // Blocks per CU = dispatch rounds: single-wave pipelines put one wave
      // per SIMD in a block, level-split blocks hold two pipelines (4 waves).
      p.bpc = split_v ? 2 * per_simd : per_simd;
      if (G == 0 && p.bpc >= 2 && !(variant & tbv::kFloat2) && !(variant & tbv::kNoAgePairs))
        G = age_groups_of(split_v, p.bpc, tune, weights);
    }
  }
  p.waves_target = waves_target;
  const bool pairs = G > 0;
  p.flags = ((variant & tbv::kXcdGroups) ? tbdetail::kTbXcdGroups : 0) |
            ((variant & tbv::kAltDirection) ? tbdetail::kTbAltDirection : 0) |
            ((variant & tbv::kDiagNoStore) ? tbdetail::kTbDiagNoStore : 0) |
            ((variant & tbv::kDiagCachedRows) ? tbdetail::kTbDiagCachedRows : 0);
  // Split rows into chunks so the whole launch has about waves_target waves,
  // but never shorter than 4*depth rows (keeps the redundant 2*depth-row
  // halo reads below ~50 %).
  // Minimum chunk length in rows (multiples of depth; HEAT_TB_MINLEN overrides).
  const int64_t min_len = tune.min_len > 0 ? tune.min_len : std::max<int64_t>(depth, 8);
  int64_t len = std::max<int64_t>(min_len, ceil_div(total_strip_rows, waves_target));
  int waves = 0;
  bool linear = variant & tbv::kLinear;
  if (!linear) {
    // Keep the total within waves_target (whole resident rounds): a few extra
    // waves would form a nearly empty extra round.
    waves = classic_plan(p, len, min_len, tune.edge_frac, G, W, depth, boxes, nbox, gx0, nx);
    // No chunk is longer than the tallest box, so a length past it plans the
    // same: capped there, len * waves cannot overflow on a target far below
    // the strips.
    int64_t max_rows = 1;
    for (int b = 0; b < nbox; ++b) max_rows = std::max(max_rows, boxes[b].rows());
    for (int it = 0; it < 8 && waves > waves_target; ++it) {
      len = std::min(max_rows, std::max(len + 1, ceil_div(len * int64_t(waves), int64_t(waves_target))));
      waves = classic_plan(p, len, min_len, tune.edge_frac, G, W, depth, boxes, nbox, gx0, nx);
    }
    // Few long chunks per strip quantise badly: 565 strips x 131072 rows
    // (131072^2 on one GPU, or a 16384-row slab of it) became 1130 two-wave
    // pipelines for 2048 slots, 2.25 blocks per CU, every chunk touching the
    // plate's top or bottom row (masked path).  Balanced linear plans ran
    // those at 5.16 / 4.65 Tcells/s instead of 3.50 / 4.33; at 8192^2 (the
    // classic plan fills 98 %) they lose 24 %: units that cross a strip end
    // or split off the masked edge rows pay a second pipeline ramp, and in a
    // one-round launch the slowest unit sets the time
    // (profiles/r3_linear_plans.md).
    linear = !(variant & tbv::kNoLinear) && waves < (9 * int64_t(waves_target)) / 10 &&
             total_strip_rows >= 32 * int64_t(depth) * waves_target;
  }
  if (linear) {
    // Balanced plan: the boxes as one strip-row sequence cut into equal
    // ranges, one per unit (per group of G units with age pairs), so every
    // unit -- and every SIMD -- gets the same rows whatever the shape.
    int n = 0;
    int64_t total = 0;
    for (int b = 0; b < nbox; ++b) {
      const Box& B = boxes[b];
      if (B.empty()) continue;
      tbdetail::TbBox& t = p.box[n++];
      tbdetail::set_strips(t, B, W);
      t.nchunks = 1;
      t.chunk_len = int(std::min<int64_t>(B.rows(), INT32_MAX));
      t.wave_begin = 0;
      t.lin0 = total;
      total += int64_t(t.nstrips) * B.rows();
    }
    p.nbox = n;
    if (n == 0) return p;
    // Long linear units accumulate the SIMD's age bias: with four blocks
    // per CU every dispatch round gets its own row share
    // (kTbLinearAgeWeights; 16384 x 131072 slab 4.70 -> 5.15 Tcells/s,
    // profiles/r3_raw/r3age_a16384.log).
    if (pairs && tune.age_weights.empty() && split_v && p.bpc >= 4) {
      weights.assign(std::begin(kTbLinearAgeWeights), std::end(kTbLinearAgeWeights));
      G = int(weights.size());
    }
    const int Gl = pairs ? G : 1;
    const int64_t units = std::max<int64_t>(
        Gl, std::min<int64_t>(waves_target, total / std::max<int64_t>(1, min_len)));
    waves = int(units / Gl * Gl);
    p.lin_total = total;
    p.lin_slack = 2 * int64_t(depth);
    p.flags |= tbdetail::kTbLinear;
  }
  if (p.nbox == 0) return p;
  p.units = p.total_waves = waves;
  if (pairs) {
    // wave_begin / total_waves count groups (units of one age).
    for (int b = 0; b < p.nbox; ++b) p.box[b].wave_begin /= G;
    p.total_waves = waves / G;
    p.flags |= tbdetail::kTbAgePairs;
    p.age_groups = G;
    double tot = 0.0;
    for (double w : weights) tot += w;
    double acc = 0.0;
    p.age_cum[0] = 0;
    for (int a = 0; a < G; ++a) {
      acc += weights[size_t(a)];
      p.age_cum[a + 1] = a + 1 == G ? 1024 : int(std::lround(1024.0 * acc / tot));
    }
  }
  if (split_v && !(variant & tbv::kShiftMixed)) {
    // Streaming rows when one pass sweeps more field than the MALL (256 MB)
    // holds: its rows come back one sweep later, never from L2 or the MALL.
    int64_t bytes = 0;
    for (int b = 0; b < nbox; ++b)
      if (!boxes[b].empty()) bytes += boxes[b].rows() * pitch * int64_t(sizeof(float));
    const bool nt = tune.nt >= 0 ? tune.nt != 0 : bytes > kTbStreamBytes;
    if (nt) p.flags |= tbdetail::kTbStreamRows;
  }
  return p;
}

void tb_plan_trace_line(char (&line)[320], int depth, const TbPlan& p) {
  std::snprintf(line, sizeof line,
                "[heat tb] depth %d variant %d boxes %d strip_rows %lld waves_target %d bpc %d "
                "linear %d units %d age_groups %d cum %d,%d,%d,%d chunk0 %d nchunks0 %d nt %d\n",
                depth, p.variant, p.nbox, (long long)p.total_strip_rows, p.waves_target, p.bpc,
                int((p.flags & tbdetail::kTbLinear) != 0), p.units, p.age_groups, p.age_cum[1],
                p.age_cum[2], p.age_cum[3], p.age_cum[4], p.box[0].chunk_len, p.box[0].nchunks,
                int((p.flags & tbdetail::kTbStreamRows) != 0));
}

namespace tbw {

void tile_trace_line(char (&line)[200], int depth, const TilePlan& pl, int xl, int nbox,
                     int64_t units, const tbdetail::TbBox& box0) {
  std::snprintf(line, sizeof line,
                "[heat tb] tile depth %d rows %d waves %d bpermute %d boxes %d units %lld tiles0 %d "
                "len0 %d\n",
                depth, pl.rows, pl.waves, xl, nbox, (long long)units, box0.nchunks, box0.chunk_len);
}

void resident_trace_line(char (&line)[200], int depth, int passes, const TilePlan& pl, int xl) {
  std::snprintf(line, sizeof line, "[heat tb] resident depth %d passes %d rows %d waves %d xl %d tiles %d\n",
                depth, passes, pl.rows, pl.waves, xl, int(pl.units));
}

}  // namespace tbw
}  // namespace heat::gpu
