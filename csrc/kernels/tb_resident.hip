// Resident workgroup tiles: the tile kernel (tb_tile.hip) with each tile kept
// in VGPRs across the P passes of one launch.
//
// A tile pass of the 8-GPU per-rank blocks costs ~11 us fixed plus ~1.7 us
// per step (profiles/r3_tile.md): every pass relaunches, and every tile
// reloads its whole 8R-row footprint at once (48 MB per pass at 1024 x 8192)
// before any step can start.  Here the grid is one dispatch round (every
// tile co-resident, checked on the host) and stays for P passes:
//
//   pass 0      load the tile from src, as tb_tile.hip does;
//   pass p      K steps in registers; the last step publishes the tile's
//               useful EDGE BANDS (K rows at the top and bottom, KK columns
//               at the left and right of its useful region) into exchange
//               field xb[p & 1] with write-through (sc1) stores, then every
//               wave drains (vmcnt 0), the workgroup barrier, and one lane
//               stores flag[tile] = p + 1 (agent-scope, sc1);
//   pass p + 1  wave 0 polls the flags of the <= 8 neighbour tiles (relaxed
//               sc1 loads, bounded spin) until they reach p + 1, the barrier
//               releases the other waves, and each wave reloads only its
//               GHOST cells -- the K-deep ring around the useful region,
//               which is exactly the neighbours' edge bands -- from
//               xb[p & 1] with sc1 loads (MI355X_MICROARCH.md "Valid forms",
//               first row: sc1 payload both sides, no acquire fence);
//   last pass   stores the useful region to dst, like tb_tile.hip.
//
// Ghost cells outside the launch's box are not reloaded (their registers are
// don't-care, as clamped rows are in tb_tile.hip): on deep-halo blocks the
// invalid region grows from the box edge by K per pass exactly as the
// shrinking boxes of separate passes do (Solver::enqueue_resident).
// Double-buffered exchange fields make the protocol race-free: a tile
// rewrites xb[p & 1] at the end of pass p + 2 only after it has seen every
// neighbour's flag p + 2, i.e. after every neighbour finished the pass p + 1
// that read it.  Flags and the completion counter are zero at every launch:
// zeroed once when the buffers are allocated, then re-zeroed by the tile that
// finishes last (the completion counter tells it; every other tile is past
// its last poll by then), in place of a memset node per launch
// (cdna_hip_programming.md Guideline 16, "Re-initialise every call"); every
// spin is bounded and reports through *err instead of hanging the device.
//
// Results are bitwise those of separate passes (heat::stencil, the same
// Tile code).  Reference: the per-rank compute of
// mpi/mpi_heat_improved_persistent_stat.c:162-234, which this replaces.
#include <cstdlib>

#include "heat/common.hpp"
#include "heat/plan.hpp"
#include "tb_resident_kern.hpp"

namespace heat::gpu::tbw {

// The lane-shift builds (tb_resident_xl<XL>.hip, compiled in parallel).
bool res_launch_x0(const ResArgs& ra, int rows, int waves, int blocks, hipStream_t st);
bool res_launch_x1(const ResArgs& ra, int rows, int waves, int blocks, hipStream_t st);
bool res_launch_x2(const ResArgs& ra, int rows, int waves, int blocks, hipStream_t st);
int res_occupancy_x0(int rows, int waves);
int res_occupancy_x1(int rows, int waves);
int res_occupancy_x2(int rows, int waves);

namespace {
int occupancy_res(int rows, int waves, int xl) {
  return xl == 1 ? res_occupancy_x1(rows, waves)
         : xl == 2 ? res_occupancy_x2(rows, waves)
                   : res_occupancy_x0(rows, waves);
}

bool launch_res(const ResArgs& ra, int rows, int waves, int xl, int blocks, hipStream_t st) {
  return xl == 1 ? res_launch_x1(ra, rows, waves, blocks, st)
         : xl == 2 ? res_launch_x2(ra, rows, waves, blocks, st)
                   : res_launch_x0(ra, rows, waves, blocks, st);
}

int cached_occupancy_res(int rows, int waves, int xl) {
  return tb_device_memo(TbMemo::kResidentOccupancy, rows, waves, xl, occupancy_res);
}

int res_xl(int variant, const TbTuning& tune) {
  // Mixed lane shifts unless a forced variant asks for DPP (variant -1 is the
  // automatic choice, not "every flag": it ran the all-DPP build, 11 % slower
  // than ds_bpermute shifts on 1024 x 8192, profiles/r4_resident.md).
  if (tune.tile_xl >= 0 && tune.tile_xl <= 2) return tune.tile_xl;
  return variant >= 0 && (variant & tbv::kTileDpp) ? 0 : 2;
}

// The shape with the lowest step estimate among those whose tiles are all
// co-resident (one dispatch round; the occupancy of the resident
// instantiation itself, bounded by its VGPR granule).
TilePlan plan_res(const Box& box, int depth, int xl, const TbTuning& tune) {
  return resident_tile_plan(
      box, depth, tb_simd_count() / 4,
      [&](int i) { return cached_occupancy_res(kResidentShapes[i].rows, kResidentShapes[i].waves, xl); },
      tune.tile_rows, tune.tile_waves);
}
}  // namespace

}  // namespace heat::gpu::tbw

namespace heat::gpu {

bool tb_resident_fits(const Box& box, int depth, int variant) {
  return tb_resident_shape(box, depth, variant) != 0;
}

int tb_resident_shape(const Box& box, int depth, int variant) {
  using namespace tbw;
  const TbTuning tune = tb_tuning();
  const TilePlan pl = plan_res(box, depth, res_xl(variant, tune), tune);
  // Every tile but the last of a strip (and every strip but the last) must
  // be at least K rows (KK columns) deep: a ghost ring comes from the
  // direct neighbours only.
  if (pl.rows == 0 || !tiles_at_least_depth(box.rows(), pl, depth)) return 0;
  return res_shape(pl.rows, pl.waves);
}

void tb_resident_step(const float* src, float* dst, const StencilGeom& g, const Box& box,
                      int depth, int passes, const TbResidentBuffers& xb, hipStream_t st,
                      int variant, const TbResidentCheck* checks, int nchecks, unsigned* resids,
                      int64_t own_rows, int64_t own_cols) {
  using namespace tbw;
  HEAT_CHECK(passes >= 2, "a resident launch spans >= 2 passes (%d)", passes);
  const TbTuning tune = tb_tuning();
  int xl = res_xl(variant, tune);
  const TilePlan pl = plan_res(box, depth, xl, tune);
  HEAT_CHECK(pl.rows > 0, "resident tiles do not fit box %lldx%lld at depth %d",
             (long long)box.rows(), (long long)box.cols(), depth);
  const int units = int(pl.units);  // one dispatch round
  HEAT_CHECK(units <= xb.max_tiles, "%d resident tiles, flag buffer holds %d", units, xb.max_tiles);
  HEAT_CHECK(xb.bytes < (int64_t(1) << 31), "exchange field of %lld bytes (32-bit offsets)",
             (long long)xb.bytes);
  ResArgs ra{};
  TbArgs& a = ra.a;
  a.src = src;
  a.dst = dst;
  HEAT_CHECK(nchecks >= 0 && nchecks <= kResMaxChecks && (nchecks == 0 || resids != nullptr),
             "%d checks in a resident launch (at most %d)", nchecks, kResMaxChecks);
  for (int c = 0; c < nchecks; ++c) {
    HEAT_CHECK(checks[c].pass >= 0 && checks[c].pass < passes && checks[c].step >= 2 &&
                   checks[c].step <= depth && checks[c].step % 2 == 0 &&
                   (c == 0 || checks[c].pass > checks[c - 1].pass),
               "resident check %d at pass %d step %d (passes %d, depth %d)", c, checks[c].pass,
               checks[c].step, passes, depth);
    ra.chk_pass[c] = checks[c].pass;
    ra.chk_step[c] = checks[c].step;
  }
  ra.nchk = nchecks;
  ra.resids = resids;
  a.resid = nchecks > 0 ? resids : nullptr;  // selects the RES 1 instantiation
  // Timing diagnostic: the RES 1 build without checks (what the residual
  // instantiation costs by itself, profiles/r5_resident_checks.md).
  static const bool diag_res1 = [] {
    const char* e = std::getenv("HEAT_TB_RES_DIAG_RES1");
    return e && *e && *e != '0';
  }();
  if (diag_res1 && resids) a.resid = resids;
  // Lane shifts: the shape is planned with the mixed shifts (XL 2); a
  // packed-update launch (rows <= kTilePkRows, checked or not) then runs with
  // DPP shifts for both neighbours (XL 0), the packed update's best partner
  // (tools/probes/stencil_chain.hip: packed + DPP 65 vs 73 cycles per row
  // update; 1168 x 8192 plate 4.90 vs 4.62 Tcells/s, 2192 x 4168 4.54 vs
  // 4.43, profiles/r6_raw/r6h/; checks every 20 steps on 1024 x 8192 4.01
  // vs 3.80, r6l; unchecked launches have the left / element-3 right edge
  // modes, tile_dispatch).  The round-4 all-DPP build was 11 % slower with
  // the scalar update, which the taller tiles keep.
  if (variant < 0 && tune.tile_xl < 0 && pl.rows <= kTilePkRows &&
      cached_occupancy_res(pl.rows, pl.waves, 0) >= cached_occupancy_res(pl.rows, pl.waves, xl))
    xl = 0;
  a.res_level = depth;
  a.g = g;
  a.flags = (variant < 0 || (variant & tbv::kXcdGroups)) ? tbdetail::kTbXcdGroups : 0;
  TbBox& t = a.box[0];
  a.total_waves = int(tile_fill_box(t, box, depth, pl, 0));
  HEAT_CHECK(t.chunk_len >= depth, "resident tiles of %d rows at depth %d", t.chunk_len, depth);
  a.nbox = 1;
  HEAT_CHECK(a.total_waves == units, "resident plan %d != %d tiles", units, a.total_waves);
  ra.passes = passes;
  ra.depth = depth;
  ra.xbase[0] = xb.base[0];
  ra.xbase[1] = xb.base[1];
  ra.xorigin = xb.origin;
  ra.xbytes = int(xb.bytes);
  HEAT_CHECK(xb.done != nullptr, "resident launch without a completion counter");
  ra.flags = xb.flags;
  ra.done = xb.done;
  ra.err = xb.err;
  ra.own_r1 = nchecks > 0 ? own_rows : box.r1;
  ra.own_c1 = nchecks > 0 ? own_cols : box.c1;
  ra.diag = tune.res_diag;
  // The flags and the completion counter are zero: zeroed once when the
  // buffers are allocated, then by the last tile of every launch.
  if (tb_trace_enabled()) {
    char line[200];
    resident_trace_line(line, depth, passes, pl, xl);
    tb_trace_once(line);
  }
  HEAT_CHECK(launch_res(ra, pl.rows, pl.waves, xl, units, st), "resident %dx%d not built",
             pl.rows, pl.waves);
  HIP_CHECK(hipGetLastError());
}

}  // namespace heat::gpu
