// Workgroup-tile temporally blocked Jacobi kernel (variant bit kTile).
//
// The register-streaming kernel (tb_stream.inl) gives every wave its own
// (strip, chunk) and pays the trapezoid of classic temporal blocking: each
// chunk recomputes K - l rows beyond both of its ends at level l.  On the
// per-rank blocks of 4-8 GPU runs (1024 x 8192, 2048 x 4096: 36 strip-rows per
// SIMD) that is 1.30x the useful row updates, and there is only room for one
// wave per SIMD, which issues a VALU op every ~4-6 cycles instead of ~2-3
// (profiles/r3_small_blocks.md).
//
// Here a workgroup of NW = 8 (or 16) waves owns one tile: a 256-column strip
// (64 lanes x float4) by NW * R rows, every wave R consecutive rows held in
// VGPRs for the whole launch.  A time step updates all rows in place; the
// only data a wave needs from outside its registers are the last row of the
// wave above and the first row of the wave below, exchanged through LDS (one
// barrier per step, halfway through it, see tile_run).  The tile pays its
// own K-deep ghost ring (2K of NW * R rows, round_up(K, 4) columns per side)
// instead of a trapezoid per wave -- about the same VALU work -- but runs
// 2-4 waves per SIMD (two workgroups per CU up to R = 16) where the
// streaming kernel has room for one (profiles/r3_tile.md).  East/west
// neighbours cross lanes with DPP wave shifts and / or ds_bpermute (XL).
//
// Input rows [r0 - K, r1 + K) and columns [c0 - round_up(K, 4), ...) of each
// box are read (the same footprint as tb_stream.inl); rows of the tile past
// that range load a clamped (valid, don't-care) row: their values only reach
// rows outside the useful range within K steps.  The update is heat::stencil,
// so results are bitwise identical to every other kernel.
//
// Reference kernel this replaces: cuda/cuda_heat.cu:140-163 (one step per
// launch, global memory) and :42-138 (the fused residual).
#include "tb_tile.hpp"

#include "heat/common.hpp"

namespace heat::gpu::tbw {

using tbdetail::TbArgs;
using tbdetail::TbBox;

namespace {
bool launch_xl(const TbArgs& args, int depth, int rows, int waves, int xl, hipStream_t st) {
  if (depth < 2 || depth % 2 != 0 || waves * rows <= 2 * depth) return false;
  return xl == 1 ? tile_launch_x1(args, depth, rows, waves, st)
         : xl == 2 ? tile_launch_x2(args, depth, rows, waves, st)
                   : tile_launch_x0(args, depth, rows, waves, st);
}

int occupancy_xl(int rows, int waves, int xl) {
  return xl == 1 ? tile_occupancy_x1(rows, waves)
         : xl == 2 ? tile_occupancy_x2(rows, waves)
                   : tile_occupancy_x0(rows, waves);
}
}  // namespace

bool launch(const TbArgs& args, int depth, int rows, int waves, bool bpermute, hipStream_t st) {
  return launch_xl(args, depth, rows, waves, bpermute ? 1 : 0, st);
}

int occupancy(int rows, int waves, bool bpermute) { return occupancy_xl(rows, waves, bpermute ? 1 : 0); }

// The launch planner.  A tile is one 256-column strip by NW waves x R rows;
// its useful rows are NW * R - 2 * depth.  The shape comes from the
// instantiated set by the estimated time of the launch (tile_shape_search):
// dispatch rounds x (rows each SIMD updates per round) x (relative cycles per
// VALU op: 2.7 with two or more independent workgroups per CU, 3.1 with one,
// whose waves stall together at its barriers; calibrated on the 8-GPU blocks,
// profiles/r3_tile.md).
void step(const float* src, float* dst, const StencilGeom& g, const Box* boxes, int nbox, int depth,
          unsigned* resid, int res_level, hipStream_t st, int variant, const TbTuning& tune) {
  // Lane shifts: mixed (2: the left shift a DPP wave shift folded into the
  // add, the right one ds_bpermute issued ahead; +3-6 % over ds_bpermute for
  // both, which waited on LDS issue 13 % of the time, profiles/r3_tile.md)
  // unless the variant asks for DPP (0); TbTuning::tile_xl (HEAT_TB_TILE_XL)
  // 0/1/2 overrides.
  const int bp = tune.tile_xl >= 0 && tune.tile_xl <= 2 ? tune.tile_xl : (variant & tbv::kTileDpp) ? 0 : 2;
  // Resident blocks per CU, cached per (device, rows, waves, shifts).
  auto occ = [&](int i) {
    return tb_device_memo(TbMemo::kTileOccupancy, kTileShapes[i].rows, kTileShapes[i].waves, bp, occupancy_xl);
  };
  const TilePlan best = tile_shape_search(boxes, nbox, depth, tb_simd_count() / 4, kTileShapes, occ,
                                          tune.tile_rows, tune.tile_waves, false);
  HEAT_CHECK(best.rows > 0, "no tile shape fits depth %d (HEAT_TB_TILE_ROWS=%d, HEAT_TB_TILE_WAVES=%d)",
             depth, tune.tile_rows, tune.tile_waves);
  TbArgs args{};
  args.src = src;
  args.dst = dst;
  args.resid = resid;
  args.res_level = res_level > 0 && res_level < depth ? res_level : depth;
  args.g = g;
  args.flags = (variant & tbv::kXcdGroups) ? tbdetail::kTbXcdGroups : 0;
  int n = 0;
  int64_t units = 0;
  for (int b = 0; b < nbox; ++b) {
    const Box& B = boxes[b];
    if (B.empty()) continue;
    HEAT_CHECK(B.c0 % 4 == 0, "TB box column start %lld not a multiple of 4", (long long)B.c0);
    HEAT_CHECK(n < tbdetail::kMaxBoxes, "too many TB boxes");
    units += tile_fill_box(args.box[n++], B, depth, best, units);
  }
  if (n == 0) return;
  HEAT_CHECK(units < (int64_t(1) << 31), "tile launch too large");
  args.nbox = n;
  args.total_waves = int(units);
  if (tb_trace_enabled()) {
    char line[200];
    tile_trace_line(line, depth, best, bp, n, units, args.box[0]);
    tb_trace_once(line);
  }
  HEAT_CHECK(launch_xl(args, depth, best.rows, best.waves, bp, st), "tile %dx%d not instantiated",
             best.rows, best.waves);
  HIP_CHECK(hipGetLastError());
}

}  // namespace heat::gpu::tbw
