// Grid I/O.
//
// * Text ".dat" output byte-compatible with the reference's prtdat
//   (cuda/cuda_heat.cu:285-300, mpi/mpi_heat_improved_persistent_stat.c:326-341):
//   "%6.1f" values, one line per iy from ny-1 down to 0 (transposed and
//   y-flipped), ix left to right, single spaces, '\n' at line end.
// * A reader for that format (tests, round trips).
// * A raw binary format with a small header, used for output of grids too
//   large for text and for checkpoint/resume (the reference has neither).
// * An order-independent checksum so huge runs can be compared across
//   decompositions without moving the grid to one host.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace heat {

// Append the "%6.1f" rendering of v to out (bit-exact with glibc printf).
void format_6_1f(float v, std::string& out);

// Write a full nx x ny row-major grid in prtdat format.
void write_dat(const std::string& path, int64_t nx, int64_t ny, const float* grid);
// Read a prtdat file back into an nx x ny row-major grid (values are the
// printed, i.e. rounded, numbers).
std::vector<float> read_dat(const std::string& path, int64_t* nx, int64_t* ny);

struct BinHeader {
  char magic[8];       // "HEATF32\0"
  uint32_t version;    // 1
  uint32_t parity;     // reserved (buffer parity at checkpoint time)
  int64_t nx, ny;
  int64_t step;        // completed steps
  float cx, cy;
  uint64_t reserved[3];  // [0]: bin_config_tag of the writer (0 = unknown)
};
static_assert(sizeof(BinHeader) == 72, "BinHeader layout");

// Create/truncate a binary grid file and write its header (rank 0).
void bin_create(const std::string& path, const BinHeader& h);
// Write a block of rows [ox, ox+lx) x cols [oy, oy+ly) taken from a strided
// source into an existing binary grid file (every rank writes its own block).
void bin_write_block(const std::string& path, int64_t nx, int64_t ny, int64_t ox, int64_t oy,
                     int64_t lx, int64_t ly, const float* src, int64_t src_pitch);
BinHeader bin_read_header(const std::string& path);
// fsync `tmp` and rename it over `path` (atomic replacement of a checkpoint).
void bin_commit(const std::string& tmp, const std::string& path);
// Header tag of the modes that change the continuation of a run.
inline uint64_t bin_config_tag(int compat, int numerics) {
  return (uint64_t(1) << 63) | (uint64_t(numerics & 0xff) << 8) | uint64_t(compat & 0xff);
}
void bin_read_block(const std::string& path, int64_t ox, int64_t oy, int64_t lx, int64_t ly,
                    float* dst, int64_t dst_pitch);

// Order-independent checksum of a block of cells with their global indices.
struct Checksum {
  uint64_t hash = 0;   // sum mod 2^64 of mix(bits, global index): order independent
  double sum = 0.0;    // plain fp64 sum (order dependent in the last bits)
  double min = 0.0, max = 0.0;
  int64_t count = 0;
  void merge(const Checksum& o);
};
Checksum checksum_block(const float* src, int64_t src_pitch, int64_t ox, int64_t oy, int64_t lx,
                        int64_t ly, int64_t ny);

// Coarse view of a field: integer factors fx (rows) and fy (columns) give the
// CR x CC grid, CR = ceil(nx / fx), CC = ceil(ny / fy); coarse cell (I, J)
// covers plate rows [I*fx, min((I+1)*fx, nx)) and columns
// [J*fy, min((J+1)*fy, ny)).  The planes are all-reduced whole, so a view has
// at most kCoarseMaxCells cells.
constexpr int64_t kCoarseMaxCells = int64_t(1) << 22;
// Throws (naming the limit and the factors) on a factor < 1 or a grid above
// the limit.
void coarse_dims(int64_t nx, int64_t ny, int64_t fx, int64_t fy, int64_t* cr, int64_t* cc);
// MERGE the lx x ly block of host memory whose cell (0, 0) is plate cell
// (ox, oy) into the CR x CC planes of the nx x ny plate: sum += the fp64 sum
// of the cell's values, min / max the smaller / larger, a NaN in the cell
// making all three NaN.  The caller initialises the planes (0, +inf, -inf);
// several disjoint blocks may be merged into one set (host twin of
// gpu::coarse_block).
void coarse_block(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                  int64_t oy, int64_t nx, int64_t ny, int64_t fx, int64_t fy, double* sum,
                  float* mn, float* mx);

// Refinement, the inverse of the coarse view's geometry: a CR x CC source grid
// S (CR = ceil(nx / fx), CC = ceil(ny / fy), at most kCoarseMaxCells cells)
// fills the nx x ny plate, piecewise constant (order 0) or cell-centred
// bilinear (order 1).  Source row I covers plate rows [lo, hi) =
// [I*fx, min((I+1)*fx, nx)); twice its centre is the integer c2_I = lo + hi - 1.
// Columns likewise.
//
// Per axis a table gives every plate index i two source indices and a weight:
//   order 0: i0 = i1 = i / f, w = 0.
//   order 1: t = 2i, k = the largest I with c2_I <= t (-1 if none).
//     0 <= k < C-1:  (k, k+1, float(double(t - c2_k) / double(c2_{k+1} - c2_k)))
//     else, no wrap or C == 1:  i0 = i1 = (k < 0 ? 0 : C-1), w = 0   (clamp)
//     else, wrap:  (C-1, 0, float(double(t - c2_{C-1} + (k < 0 ? 2n : 0)) /
//                                 double(c2_0 + 2n - c2_{C-1})))
// Always 0 <= w < 1, and i0 == i1 implies w == 0.  Integers and one fp64
// quotient rounded once to fp32: the same on every host.
//
// Cell (i, j), all in fp32, columns first:
//   lerp(a, b, w) = (w == 0) ? a : fmaf(w, b - a, a)
//   top = lerp(S[i0,j0], S[i0,j1], wy);  bot = lerp(S[i1,j0], S[i1,j1], wy)
//   u = lerp(top, bot, wx)
// The select makes order 0 a bit-exact copy (NaN payloads, infinities); other
// non-finite or overflowing values follow the expression.
struct RefineTable {
  const int32_t* i0 = nullptr;
  const int32_t* i1 = nullptr;
  const float* w = nullptr;
};
// The table entries of plate indices [begin, begin + count) of an axis of n
// cells refined by f.
void refine_axis(int64_t n, int64_t f, int order, bool wrap, int64_t begin, int64_t count,
                 int32_t* i0, int32_t* i1, float* w);
// The plate index whose value a cell at index i of an axis of n cells holds,
// i possibly beyond the plate (a ghost cell): i itself inside the plate,
// i mod n on a wrapped (periodic) axis, the mirror image -i or 2(n-1) - i
// beyond a mirrored (insulated) end, else the nearest plate index (beyond a
// fixed end, which no update reaches).
int64_t ghost_axis_index(int64_t i, int64_t n, bool wrap, bool mirror_lo, bool mirror_hi);
// refine_axis for indices [begin, begin + count) that may lie beyond the plate:
// entry q is the plate's table entry at ghost_axis_index(begin + q).  A field
// that is a function of the plate index alone (the heat source) gets its ghost
// cells this way, without communication.
void refine_axis_ext(int64_t n, int64_t f, int order, bool wrap, bool mirror_lo, bool mirror_hi,
                     int64_t begin, int64_t count, int32_t* i0, int32_t* i1, float* w);
// Throws unless fx, fy, order are valid and a CR x CC source is what
// coarse_dims gives for the plate (the message names all four numbers).
void refine_check(int64_t nx, int64_t ny, int64_t cr, int64_t cc, int64_t fx, int64_t fy,
                  int order);
// Fill the lx x ly block of host memory at `origin` from S (CC columns) and
// the tables of the block's rows and columns (lx and ly entries): host twin of
// gpu::refine_block.  Writes the block's cells only.
void refine_block(float* origin, int64_t pitch, int64_t lx, int64_t ly, const float* S,
                  int64_t cc, const RefineTable& rows, const RefineTable& cols);

}  // namespace heat
