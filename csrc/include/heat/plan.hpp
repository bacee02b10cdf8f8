// Resident-aware planning of the deep-halo depth (host side, no GPU code):
// which passes-per-exchange m keeps every rank's resident span box inside a
// one-dispatch-round resident tile plan of the same shape as its owned
// block's.  Separate from topology.hpp so the kernel units, which include
// that header, do not depend on it (tb_resident.hip alone includes this one,
// for the resident shapes below).
//
// Also the geometry of a pass, shared by the solver, the planner and `heat
// --plan`: which cells a pass of depth k computes and which ghosts stay valid.
#pragma once

#include <functional>
#include <utility>

#include "heat/topology.hpp"

namespace heat {

// The sides and axes of one rank.  open[d]: side d has ghosts to keep: a
// neighbour rank, or the rank's own insulated or periodic plate edge (a rank
// without a neighbour on a side is at the plate edge there).  ns, ew: the axis
// is decomposed, has an insulated side or is periodic; from global quantities
// only, so every rank agrees.  An open side lies on an active axis.
struct Sides {
  bool open[4] = {false, false, false, false};
  bool ns = false, ew = false;
};
Sides make_sides(const Cart& cart, const Block& b, unsigned insulated, unsigned periodic);

// The lx x ly owned block grown by er rows and ec columns into the ghost ring
// on every open side: the box of a deep-halo pass.
inline Box grown_box(int64_t lx, int64_t ly, const Sides& s, int64_t er, int64_t ec) {
  return Box{s.open[North] ? -er : 0, lx + (s.open[South] ? er : 0), s.open[West] ? -ec : 0,
             ly + (s.open[East] ? ec : 0)};
}

// gr, gc: how many ghost rows/columns of the current field hold the current
// time level.  A k-step pass needs k; an exchange refills H.  Invariant: they
// never exceed the depth of the last exchange of this buffer -- N/S row
// messages carry the sender's own (stale) ghost columns into our corners, and
// only the corner unpack of THAT exchange overwrites them up to its depth (the
// overlap schedule exchanges k < H and then claims 0;
// tests/test_gpu_loopback.py::test_loopback_deep_halo_chunked mixes depths and
// short tail segments on 2 x 2 ranks).  The pass then also updates the
// (valid - k) ghost rows/columns next to the block, which become the valid
// ghosts of the next level.  Only active axes count, so every rank makes the
// same decision.
struct GhostState {
  int64_t gr = 0, gc = 0;
  bool needs_exchange(const Sides& s, int k) const { return (s.ns && gr < k) || (s.ew && gc < k); }
  void refill(int64_t H) { gr = gc = H; }
  // A k-step pass: returns the growth (er, ec) of its box and leaves the
  // validity after it.  `tb`: TB boxes start on a float4 column, so the column
  // extension is rounded down to a multiple of 4.
  std::pair<int64_t, int64_t> advance(const Sides& s, int k, bool tb) {
    gr = s.ns ? gr - k : 0;
    gc = s.ew ? (tb ? (gc - k) / 4 * 4 : gc - k) : 0;
    return {gr, gc};
  }
};

// The first box of a resident span after an exchange of H = m * depth deep
// halos: rank b's owned block after refill(H) and advance(depth) of the TB
// kernels.
Box span_box(const Cart& cart, const Block& b, int depth, int m, unsigned insulated = 0,
             unsigned periodic = 0);

// One launch of a k-step pass run by kernels that take fewer than k steps: n
// steps over the pass's box grown by `grow`, the steps still to come behind
// it; takes_resid: it ends at the pass's check level.
struct SubPass {
  int n = 0, grow = 0;
  bool takes_resid = false;
};
// The launch that starts at step j of the pass (j = 0, then j += n up to k):
// at most group_max steps, and none past step rl when rl > j.
inline SubPass sub_pass(int k, int rl, int group_max, int j) {
  const int left = (j < rl ? rl : k) - j, n = left < group_max ? left : group_max;
  return {n, k - j - n, j + n == rl};
}
// The first steps of a pass again, `left` of them still to run: the depth of
// the next launch.  All at once if the kernel takes that depth (`supported`),
// else left mod 8 first, then 8s.
inline int replay_depth(int left, bool supported) {
  return supported ? left : (left % 8 != 0 ? left % 8 : 8);
}

// The overlap schedules' split of the owned block: an interior that needs no
// ghosts, `band` away from every side with a neighbour rank (column cuts on
// float4 columns; empty: no split), and the boundary bands around it: top,
// bottom, left, right.
struct InteriorSplit {
  Box interior, bands[4];
};
InteriorSplit interior_split(int64_t lx, int64_t ly, const std::array<int, 4>& nbr, int64_t band);

// A resident tile plan's shape as one int: rows per wave << 8 | waves per
// workgroup (0: the box has no one-round resident plan).
constexpr int res_shape(int rows, int waves) { return rows << 8 | waves; }

// The fewest passes per exchange worth a resident span: a span pays one
// whole-tile load and store, shorter spans lose to m = 8 streaming passes
// (4 x 1 slabs of 8192^2 fit only at m = 2: 4.18 Tcells/s on the 2072-row
// box against the split pipelines' 4.08 on 2216 rows, even once the 4x
// exchanges are paid; profiles/r6_resident_protocol.md).
constexpr int kResMinPasses = 4;

// Resident-aware halo depth (passes per exchange): the largest m in
// [2, mmax] whose H = m * depth fits every rank's extent along the
// decomposed axes and for which every rank's first span box has a one-round
// resident plan of the SAME shape as its owned block's (`shape`); 0 when the
// owned blocks have none or no m >= 2 keeps it.  Large m trades redundant
// ghost compute for fewer exchanges, but a box past its block's plan falls
// to another shape or to the per-pass kernels (round-6 sweeps, one MI355X,
// rank boxes at m-pass spans, per owned cell):
//   8192^2 on 8 x 1: m = 7 (1168 rows, 12 x 16 tiles) 3.72 Tcells/s, m = 8
//     (1192 rows, 14 x 8 two per CU) 3.40;  4 x 2: m = 7 3.88, m = 8 3.36;
//   8192^2 on 2 x 2: m = 5 (4144^2, 20 x 16) 4.73, m = 8 (4180^2, split
//     pipelines) 3.79.
int resident_halo_passes(const Cart& cart, int64_t nx, int64_t ny, int depth, int mmax,
                         const std::function<int(const Box&)>& shape, unsigned insulated = 0,
                         unsigned periodic = 0);

// Rows (columns) a rank can lend to an H-deep halo along each axis: the
// smallest block extent of any rank along a decomposed axis, one less along
// an axis with an insulated side (its ghosts mirror rows 1..H); the smallest
// block extent itself along a periodic axis (wrap sources are the last or
// first H rows of a block); INT64_MAX along an axis with none of these.  The
// ghost depth is at most the smaller one.
int64_t halo_extent_limit(const Cart& cart, int64_t nx, int64_t ny, unsigned insulated,
                          unsigned periodic = 0);

// Host-side resident plan of a box at `depth` on an MI355X (`cus` CUs): the
// tile planner's shapes and choice (tb_plan.hpp resident_tile_plan: the lowest
// tile_step_estimate among the shapes whose tiles are all co-resident) with
// the co-resident workgroups per CU the occupancy API reports for gfx950
// (kResidentOccGfx950; also RES_SHAPES of parallel/model.py).  `heat --plan` uses it without a
// GPU; the solver asks the device (gpu::tb_resident_shape).
int resident_shape_static(const Box& box, int depth, int cus = 256);

namespace gpu {
// The device planner's shape for a resident launch over `box` (0: none);
// tb_resident.hip.
int tb_resident_shape(const Box& box, int depth, int variant = -1);
}  // namespace gpu

}  // namespace heat
