// Device kernel launchers (gfx950).  Implementations: csrc/kernels/*.hip.
//
// Reference kernels these replace:
//   heat(old,new)              cuda/cuda_heat.cu:140-163  -> naive_step / tb_step
//   heat<threads>(old,new,f)   cuda/cuda_heat.cu:42-138   -> the same kernels with the
//                                                           fused max|delta| residual
//   semi_reduce(f)             cuda/cuda_heat.cu:32-40    -> removed: the residual is a
//                                                           single device word (atomic max)
//   MPI col_type datatype      mpi/...c:82-84             -> pack_box / unpack_box
//   host inidat + H2D copies   cuda/cuda_heat.cu:194-198  -> init_field (device side)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "heat/io.hpp"
#include "heat/tb_plan.hpp"
#include "heat/topology.hpp"

namespace heat::gpu {

// Geometry shared by all stencil kernels.  `src`/`dst` point at local owned
// cell (0,0) of a field allocated with some Layout; (gx0, gy0) are the
// global coordinates of that cell.  Only cells with 1 <= gx <= nx-2 and
// 1 <= gy <= ny-2 are updated (fixed Dirichlet ring); every other
// cell keeps its value.  Insulated plate edges (Params::insulated) reach the
// kernels only through this geometry: the solver hands them a plate extended
// by its ghost depth beyond every insulated side (Solver::geom), whose ghost
// cells fill_insulated_ghosts keeps equal to the plate's mirror image; a
// periodic axis (Params::periodic) likewise, its ghost cells holding the
// opposite edge of the plate (a neighbour rank's halo, or fill_edge_ghosts).
struct StencilGeom {
  int64_t pitch = 0;
  int64_t gx0 = 0, gy0 = 0;
  int64_t nx = 0, ny = 0;
  float cx = 0.1f, cy = 0.1f;
  int numerics = 0;  // heat::Numerics (naive kernel only; TB is always Fp32)
  // Convergence gate (device word, null = none): a launch whose gate reads
  // non-zero writes nothing (see judge_check).
  const unsigned* gate = nullptr;
};

// Fill every allocated cell (owned, ghost ring and padding) of a field with
// the initial condition at its global coordinates (0 outside the plate).
void init_field(float* origin, const Layout& L, int64_t gx0, int64_t gy0, int64_t nx,
                int64_t ny, int mode, uint64_t seed, hipStream_t st);

// One Jacobi step over `box` (local coordinates), one cell per thread.
// If resid != nullptr, atomically max-reduces |new - old| (as float bits)
// over the box into *resid.
void naive_step(const float* src, float* dst, const StencilGeom& g, const Box& box,
                unsigned* resid, hipStream_t st);

// `depth` fused Jacobi steps over up to 5 output boxes in one launch using
// the register-streaming temporally blocked kernel.  Reads rows
// [r0-depth, r1+depth) and columns [c0-round_up(depth,4), ...) of src, so the
// ghost ring must be at least that deep and valid (halo exchanged).
// Box column starts must be multiples of 4.  Writes: the boxes, and, since a
// wave stores whole float4 lanes, possibly box rows x [c1, round_up(c1, 4))
// with unspecified values (padding, or ghost columns the next exchange
// refills); no other cell of dst (tests/test_gpu_edge_modes.py checks it on a
// sentinel-filled field).  naive_step and lds_step write their box alone.
// `waves_target` steers the row
// chunking (parallelism vs. redundant halo work): > 0 absolute wave count,
// 0 default rounds, < 0 that many whole rounds of resident waves.
// `variant`: bits 0-1 pipeline (0: 3-row rings, skew 1; 1: 4-row rings,
// skew 2; 2: 2-row rings + copy; 3: 3-row rings + ramp skip), bit 2
// scalar-update build; -1 = default
// (HEAT_TB_VARIANT or the tuned choice).
// One Jacobi step over `box` from an LDS-staged 32x256 halo tile per
// workgroup (float4 lanes, DPP east/west); honours g.numerics.
void lds_step(const float* src, float* dst, const StencilGeom& g, const Box& box,
              unsigned* resid, hipStream_t st);

// One Jacobi step over `box` as banded matrix products on the fp32 MFMA
// units (v_mfma_f32_16x16x4_f32); rounding differs from heat::stencil.
void mfma_step(const float* src, float* dst, const StencilGeom& g, const Box& box,
               unsigned* resid, hipStream_t st);

// res_level (with resid): the step 1..depth whose max |new - old| is taken;
// 0 = depth (the pass's last step).  Inner levels need tb_mid_residual(depth).
// chain (optional): run chain->passes passes of `depth` steps in ONE launch
// of the chained level-split kernel (tb_chain.hip) when this launch's plan
// qualifies (the streaming split build, one box, no residual, a classic
// plan of one dispatch round, at most chain->max_units units); the passes
// ping-pong between src and dst (an odd count ends in dst).  chain->chained
// reports whether it ran; if not, nothing was launched.
struct TbChain {
  int passes = 1;
  unsigned* flags = nullptr;  // >= max_units words, zero (the launch re-zeroes them)
  unsigned* done = nullptr;   // zero (re-zeroed by the launch)
  unsigned* err = nullptr;    // set non-zero if a unit's poll gave up
  int max_units = 0;
  bool chained = false;
};
void tb_step(const float* src, float* dst, const StencilGeom& g, const Box* boxes, int nbox,
             int depth, unsigned* resid, hipStream_t st, int waves_target = 0, int variant = -1,
             int res_level = 0, TbChain* chain = nullptr);
// Resident workgroup tiles (tb_resident.hip): `passes` passes of `depth`
// steps over ONE box in a single launch whose tiles stay in VGPRs, trading
// only their K-deep ghost rings between passes through two exchange fields
// (same layout as the field) and per-tile flags.  The tiles of the box must
// all be co-resident (tb_resident_fits).  src is read by the first pass only;
// dst receives the last pass's box.  checks: convergence checks inside the
// launch (increasing passes, at most one per pass, each at an even level
// 2 <= checks[c].step <= depth): check c writes the max |delta| of that
// step over the owned block [0, own_rows) x [0, own_cols) into
// resids[slot * kTbResidentMaxChecks + c] (atomic max per wave, 64 slots;
// words zeroed by the caller, kTbResidentSlots * kTbResidentMaxChecks of
// them: judge_check(resids, ..., n, kTbResidentSlots, kTbResidentMaxChecks)).
struct TbResidentBuffers {
  float* base[2] = {nullptr, nullptr};  // exchange field allocations
  int64_t origin = 0;                   // owned cell (0, 0) in floats from base
  int64_t bytes = 0;                    // allocation size
  unsigned* flags = nullptr;            // >= max_tiles words, 16-byte aligned, zeroed once
  int max_tiles = 0;
  unsigned* done = nullptr;             // completion counter, zeroed once
  unsigned* err = nullptr;              // set non-zero if a neighbour wait gave up
};
struct TbResidentCheck {
  int pass = 0, step = 0;
};
constexpr int kTbResidentMaxChecks = 64;  // a 1024-step gated segment checking every 20 steps: 51
bool tb_resident_fits(const Box& box, int depth, int variant = -1);
void tb_resident_step(const float* src, float* dst, const StencilGeom& g, const Box& box,
                      int depth, int passes, const TbResidentBuffers& xb, hipStream_t st,
                      int variant = -1, const TbResidentCheck* checks = nullptr,
                      int nchecks = 0, unsigned* resids = nullptr, int64_t own_rows = 0,
                      int64_t own_cols = 0);

// The automatic variant choice at this depth takes a residual at any inner
// level (depth 12: level-split pipelines or workgroup tiles), so a
// convergence check can ride inside a full-depth pass instead of cutting it.
bool tb_mid_residual(int depth);
// Variant a launch of `depth` uses by default (HEAT_TB_VARIANT overrides).
int tb_default_variant(int depth);
// Variant tb_step picks for a launch of `depth` with this much work
// (strip-rows of 232/256-column float4 strips per SIMD).
int tb_auto_variant(int depth, int64_t strip_rows_per_simd);
// Diagnostics: while set, every tb_step launch writes 4 u64 per wave into buf
// ({start, end} s_memrealtime ticks (100 MHz), block, strip<<32 | chunk);
// waves = buffer capacity in waves.  nullptr switches it off.
void tb_set_stamps(unsigned long long* buf, int64_t waves);
// The variant flags, TbTuning and the launch planners: heat/tb_plan.hpp.
TbTuning tb_tuning();  // a copy of the current set
void tb_set_tuning(const TbTuning& t);
// Whole rounds of resident waves per launch (TbTuning::rounds; 0 = unset: the
// planner picks waves per SIMD from the work, tb_auto_waves_per_simd).
int tb_default_rounds();
// Resident waves of the TB kernel instantiation on the current device.
int tb_resident_waves(int depth, int variant);
// SIMDs of the current device (CUs x 4).
int tb_simd_count();

// Copy a box of a strided field to/from a contiguous buffer (E/W halos).
void pack_box(const float* origin, int64_t pitch, const Box& box, float* buf, hipStream_t st);
// Up to kMaxBoxCopies boxes <-> their contiguous buffers (row-major
// rows x cols) in ONE launch: the packing / unpacking of a whole halo
// exchange (E/W columns and ghost corners).
constexpr int kMaxBoxCopies = 8;
struct BoxCopy {
  Box box;
  float* buf = nullptr;
};
void copy_boxes(float* origin, int64_t pitch, const BoxCopy* copies, int n, bool to_buf,
                hipStream_t st);
void unpack_box(const float* buf, float* origin, int64_t pitch, const Box& box, hipStream_t st);

// Insulated (zero-flux) plate edges (ghost_fill.hip): in ONE launch, fill the
// ghost frame [-depth, lx+depth) x [-depth, ly+depth) of a field beyond every
// side in `sides` (bit 1 << heat::Dir: this rank's insulated plate edges)
// with the mirror image of the field across that edge row / column, the edge
// cell itself not repeated: (r < 0, c) := (-r, c), (r >= lx, c) :=
// (2(lx-1) - r, c), likewise for columns, both reflections for a cell beyond
// two insulated sides.  Only cells beyond at least one side of `sides` are
// written; a source is never a target, but it may be a ghost cell that a real
// neighbour's halo filled, so this runs after the exchange's unpack on the
// same stream.  Needs lx > depth (ly > depth) along an axis with a side in
// `sides` and a ghost ring at least `depth` deep.  Graph-capturable.
void fill_insulated_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int sides,
                           int depth, hipStream_t st);
// The general fill, a mode per side: mirror beyond the sides in
// `insulated_sides` as above, wrap beyond both sides of every axis in
// `periodic_axes` (Params::periodic bits: an axis this rank spans alone),
// (r < 0, c) := (r + lx, c), (r >= lx, c) := (r - lx, c), likewise for
// columns; a frame cell's source is the per-axis composition of the maps, so a
// corner between a wrapped axis and a mirrored or neighbour-filled side comes
// out right in the same launch.  An axis cannot be wrapped and have a mirrored
// side; a wrapped axis needs an extent >= depth.  fill_insulated_ghosts is
// this with no periodic axis.
void fill_edge_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int insulated_sides,
                      int periodic_axes, int depth, hipStream_t st);

// Order-independent checksum of the owned block, accumulated on the device
// into out (zeroed by the caller): hash (u64, wrapping sum of
// mix64(global index, bits)), sum (f64), min/max (order-preserving int keys).
struct DeviceChecksum {
  unsigned long long hash;
  double sum;
  int min_key, max_key;
  unsigned long long count;
};
void checksum_block(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                    int64_t oy, int64_t ny, DeviceChecksum* out, hipStream_t st);
float checksum_key_to_float(int key);

// Coarse view of a field (coarse.hip): factors fx (rows) and fy (columns)
// give the CR x CC grid of heat::coarse_dims; coarse cell (I, J) covers plate
// rows [I*fx, min((I+1)*fx, nx)) and columns [J*fy, min((J+1)*fy, ny)).  Per
// cell the planes hold the fp64 sum of its values (no fixed order) and its
// min / max as order-preserving int keys, NaN on top, the min as the key of
// the negated value so that both merge by an integer max (the residual
// word's trick): a cell that holds a NaN reads NaN in all three.
struct CoarsePlanes {
  double* sum = nullptr;
  int* nmin_key = nullptr;  // key(-min)
  int* max_key = nullptr;
};
// Planes of `cells` cells to the identity (sum 0, min +inf, max -inf).
void coarse_reset(const CoarsePlanes& p, int64_t cells, hipStream_t st);
// In place, float planes (min, max) <-> keys.  Decoding with negated_min
// leaves -min in the min plane (what an all-reduce by max wants).
void coarse_encode(const CoarsePlanes& p, int64_t cells, hipStream_t st);
void coarse_decode(const CoarsePlanes& p, int64_t cells, bool negated_min, hipStream_t st);
// MERGE the lx x ly block whose cell (0, 0) is plate cell (ox, oy) at
// `origin` into the planes of the nx x ny plate.  Blocks merged into one set
// of planes must be disjoint: a coarse cell that lies whole inside one wave's
// share of the block is written with plain stores, only cells cut by a
// strip, a row chunk or the block's edge go through atomics (one per wave
// and cell).  Reads owned cells only, never a ghost or padding cell.
// Graph-capturable, no host synchronisation.
void coarse_block(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                  int64_t oy, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
                  const CoarsePlanes& planes, hipStream_t st);
// The launch plan of coarse_block.  A unit is one wave's share: a strip of at
// most kCoarseStripCols columns (whole coarse columns where fy allows:
// `owned`) times a chunk of at most chunk_rows rows (whole coarse rows where
// fx <= chunk_rows); the launch's waves grid-stride over the units.
constexpr int kCoarseStripCols = 256;    // 64 lanes x float4
constexpr int kCoarseMaxChunkRows = 64;  // halved down to kCoarseMinChunkRows
constexpr int kCoarseMinChunkRows = 8;   // while the units do not fill the device
constexpr int kCoarseWavesPerCu = 32;    // launch size: waves per CU
struct CoarsePlan {
  bool owned = false;        // strips hold whole coarse columns
  int cells_per_strip = 0;   // owned: coarse columns per strip
  int64_t strips = 0, chunks = 0, units = 0;
  int chunk_rows = 0;        // rows per chunk (fx > chunk_rows: pieces of a coarse row)
  int rows_per_chunk_cells = 0;  // fx <= chunk_rows: coarse rows per chunk, else 0
  int pieces = 1;            // fx > chunk_rows: chunks per coarse row
  int waves = 0;             // waves launched
  bool vector_rows = false;  // rows read as aligned float4 (else scalar loads)
};
CoarsePlan coarse_plan(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                       int64_t oy, int64_t fx, int64_t fy);
// Tests: cap the waves of a launch (0: kCoarseWavesPerCu per CU).
void coarse_set_max_waves(int waves);

// Refinement (refine.hip; definition in io.hpp): fill the lx x ly block at
// `origin` from the source grid S (CC columns) and the tables of the block's
// rows and columns (lx and ly entries), all device memory:
//   u(r, c) = lerp(lerp(S[i0,j0], S[i0,j1], wy), lerp(S[i1,j0], S[i1,j1], wy), wx)
// bit for bit what heat::refine_block gives.  Writes the block's cells only,
// never a ghost or padding cell.  No LDS, atomics or scratch; graph-capturable,
// no host synchronisation.
void refine_block(float* origin, int64_t pitch, int64_t lx, int64_t ly, const float* S,
                  int64_t cc, const RefineTable& rows, const RefineTable& cols, hipStream_t st);
// The launch plan of refine_block.  A unit is one wave's share: a strip of
// kRefineStripCols columns (a lane owns 4 adjacent ones; lane 0 of strip 0
// starts on the 16-byte boundary at or below the origin, `align` columns
// early) times a chunk of chunk_rows rows; the launch's waves grid-stride
// over the units.
constexpr int kRefineStripCols = 256;    // 64 lanes x float4
constexpr int kRefineMaxChunkRows = 64;  // halved down to kRefineMinChunkRows
constexpr int kRefineMinChunkRows = 8;   // while the units do not fill the device
constexpr int kRefineWavesPerCu = 32;    // launch size: waves per CU
struct RefinePlan {
  int64_t strips = 0, chunks = 0, units = 0;
  int chunk_rows = 0;
  int waves = 0;             // waves launched
  int align = 0;             // columns lane 0 of strip 0 starts before the origin
  bool vector_rows = false;  // whole lanes store an aligned float4 (else dwords)
};
RefinePlan refine_plan(const float* origin, int64_t pitch, int64_t lx, int64_t ly);
// Tests: cap the waves of a launch (0: kRefineWavesPerCu per CU).
void refine_set_max_waves(int waves);

// One Jacobi step with a static per-cell heat source over `box` (source.hip):
//   u' = heat::stencil(c, n, s, w, e, cx, cy) + q
// one rounded fp32 add after the unchanged FMA expression; q has the layout of
// src and dst (the same pitch, cell (0, 0) at the pointer).  lds_step's
// contract: only cells with 1 <= gx <= nx-2 and 1 <= gy <= ny-2 are updated
// (a fixed cell keeps its value and ignores q), the box alone is written, a
// closed g.gate writes nothing, and with resid the max |new - old| over the
// box's updated cells is max-reduced as float bits (a NaN on top) with one
// atomic per workgroup.  Reads u in rows [r0-1, r1] x columns [c0-1, c1] and q
// in the box, nothing else.  fp32 numerics only.  Two LDS words (the
// residual), no scratch; graph-capturable, no host synchronisation.
void source_step(const float* src, float* dst, const float* q, const StencilGeom& g,
                 const Box& box, unsigned* resid, hipStream_t st);
// The launch plan of source_step.  A unit is one wave's share: a strip of
// kSourceStripCols columns (a lane owns 4 adjacent ones; lane 0 of strip 0
// starts on the 16-byte boundary at or below the box's first column, `align`
// columns early) times a chunk of chunk_rows rows, streamed with a 3-row
// window in registers; the launch's waves grid-stride over the units.
constexpr int kSourceStripCols = 256;    // 64 lanes x float4
constexpr int kSourceMaxChunkRows = 64;  // shortened, down to kSourceMinChunkRows,
constexpr int kSourceMinChunkRows = 8;   // while the units do not fill one round of the launch
constexpr int kSourceWavesPerCu = 16;    // launch size: waves per CU (half the occupancy: at
                                         // 8192^2 4096 waves ran 1.2x faster than 7104,
                                         // profiles/source.md)
struct SourcePlan {
  int64_t strips = 0, chunks = 0, units = 0;
  int chunk_rows = 0;
  int waves = 0;             // waves launched
  int align = 0;             // columns lane 0 of strip 0 starts before the box
  bool vector_rows = false;  // whole lanes move aligned float4s (else dwords): the pitch is
                             // a multiple of 4 and the three arrays share their 16-byte phase
};
SourcePlan source_plan(const float* src, const float* dst, const float* q, int64_t pitch,
                       const Box& box);
// Tests: cap the waves of a launch (0: kSourceWavesPerCu per CU, at most the
// kernel's resident waves).
void source_set_max_waves(int waves);
// Tests and tools/source_bench.py only (process-global: it changes every
// launch of every solver in the process): q loads and dst stores non-temporal
// (1) or plain (0); -1, the default: by the bytes a step sweeps, non-temporal
// above the Infinity Cache's 256 MiB (profiles/source.md).
void source_set_nontemporal(int mode);

// k fused source steps in one launch (source_tb.hip), 2 <= k <=
// kSourceTbMaxDepth: dst on `box` is bit for bit what k calls of source_step
// give, call j = 0 .. k-1 over `box` grown by k-1-j on every side and clipped
// to the plate rectangle of g; src and dst must not alias and src is left
// untouched.  Cells of a fixed edge and cells off the plate keep their centre
// value at every level.  Reads src only in `box` grown by k and q only in
// `box` grown by k-1, both clipped to the plate; writes dst on `box` alone.
// With resid: max |u_k - u_{k-1}| over the updated cells of `box` (the last
// level only), as float bits with a NaN on top, one atomic per workgroup.  A
// closed g.gate writes nothing.  Any 4-byte-aligned pointers and any pitch >=
// the box's width (dword accesses unless the pitch is a multiple of 4 and the
// arrays share their 16-byte phase).  Two LDS words, no scratch;
// graph-capturable, no host synchronisation.
constexpr int kSourceTbMaxDepth = 8;
void source_tb_step(const float* src, float* dst, const float* q, const StencilGeom& g,
                    const Box& box, int k, unsigned* resid, hipStream_t st);
// The launch plan of source_tb_step.  A unit is one wave's share: a strip of
// kSourceTbStripCols columns, of which it stores the middle strip_stride =
// kSourceTbStripCols - 2 overlap (overlap = round_up(k, 4): neighbouring
// strips share that many columns per side, lane 0 of strip 0 starts `align` +
// overlap columns left of the box), times a chunk of chunk_rows rows, streamed
// with the k levels' row windows and a ring of k rows of q in registers (k
// more rows of src above and below the chunk).
constexpr int kSourceTbStripCols = 256;     // 64 lanes x float4
constexpr int kSourceTbMaxChunkRows = 256;  // 2k of chunk_rows + 2k streamed rows are redundant;
constexpr int kSourceTbMinChunkRows = 32;   // shortened while the units do not fill a round
constexpr int kSourceTbWavesPerCu = 8;      // launch size: two waves per SIMD
struct SourceTbPlan {
  int64_t strips = 0, chunks = 0, units = 0;
  int chunk_rows = 0;
  int waves = 0;         // waves launched
  int align = 0;         // columns between the 16-byte boundary and box.c0
  int overlap = 0;       // round_up(k, 4)
  int strip_stride = 0;  // columns a strip stores
  bool vector_rows = false;
};
SourceTbPlan source_tb_plan(const float* src, const float* dst, const float* q, int64_t pitch,
                            const Box& box, int k);
// Tests: cap the waves of a launch (0: kSourceTbWavesPerCu per CU, at most the
// kernel's resident waves).  With a cap the plan needs no device.
void source_tb_set_max_waves(int waves);
// Fused launches enqueued by this process so far (tests: which kernel ran).
long long source_tb_launches();

// Device-side convergence decision (one per check, stream-ordered after the
// residual of the check's pass and its all-reduce): the host never waits on a
// check.  Unless the gate is already closed, judge_check compares the
// residual with eps (compat mpi: double(r) <= eps, mpi/...c:245; otherwise
// r < float(eps), cuda/cuda_heat.cu:67), closes the gate on convergence or on
// a non-finite residual, and zeroes the residual word for the next check.
// Every stencil launch given the gate (StencilGeom::gate = &stop) returns at
// once after that, so passes queued behind the converging check write
// nothing.  The host reads the record after the run.
struct DeviceGate {
  unsigned stop;        // gate word: non-zero once closed
  unsigned reason;      // 1 converged, 2 non-finite residual
  unsigned stop_check;  // ordinal (0-based, since the last reset) of the closing check
  unsigned checks;      // checks judged while open
  unsigned last_bits;   // residual (float bits) of the last judged check
  unsigned pad[3];
};
// n > 1: n consecutive checks judged in order in one launch (the checks of a
// resident span); check i's residual is the max of resid[s * stride + i]
// over s < slots (the span's tiles spread their atomics over `slots` cache
// lines: 500 workgroups on one word serialised ~3.5 us per check).
void judge_check(unsigned* resid, DeviceGate* gate, double eps, bool mpi_compat, hipStream_t st,
                 int n = 1, int slots = 1, int stride = 0);
// The resident span's residual block: kTbResidentSlots lines of
// kTbResidentMaxChecks words (TbResidentBuffers / tb_resident_step resids);
// wave w of tile t adds to slot (t * waves + w) % kTbResidentSlots.
constexpr int kTbResidentSlots = 64;

// Max |a-b| over a box (standalone residual), atomically into *resid.
void residual_box(const float* a, const float* b, int64_t pitch, const Box& box, unsigned* resid,
                  hipStream_t st);

}  // namespace heat::gpu
