// Process topology / decomposition (see topology.hpp for the reference map).
#include "heat/plan.hpp"
#include "heat/tb_plan.hpp"
#include "heat/topology.hpp"

#include <algorithm>
#include <cmath>

#include "heat/common.hpp"

namespace heat {

std::vector<int> dims_create(int nnodes, int ndims) {
  HEAT_CHECK(nnodes >= 1 && ndims >= 1, "nnodes=%d ndims=%d", nnodes, ndims);
  std::vector<int> dims(ndims, 1);
  if (ndims == 1) {
    dims[0] = nnodes;
    return dims;
  }
  if (ndims == 2) {
    // Most balanced split: the largest divisor d <= sqrt(n) gives [n/d, d].
    int d = int(std::sqrt(double(nnodes)));
    while (d > 1 && nnodes % d != 0) --d;
    dims[0] = nnodes / d;
    dims[1] = d;
    return dims;
  }
  // General case: largest prime factors first, each to the smallest dim.
  std::vector<int> primes;
  int n = nnodes;
  for (int p = 2; int64_t(p) * p <= n; ++p)
    while (n % p == 0) { primes.push_back(p); n /= p; }
  if (n > 1) primes.push_back(n);
  std::sort(primes.rbegin(), primes.rend());
  for (int p : primes) *std::min_element(dims.begin(), dims.end()) *= p;
  std::sort(dims.rbegin(), dims.rend());
  return dims;
}

Cart::Cart(int world_size, DecompKind kind, int px_req, int py_req, int64_t nx, int64_t ny)
    : world(world_size) {
  HEAT_CHECK(world_size >= 1, "world size %d", world_size);
  if (px_req > 0 || py_req > 0) {
    if (px_req <= 0) px_req = world_size / py_req;
    if (py_req <= 0) py_req = world_size / px_req;
    HEAT_CHECK(int64_t(px_req) * py_req == world_size,
               "process grid %dx%d does not match world size %d", px_req, py_req, world_size);
    px = px_req;
    py = py_req;
  } else if (kind == DecompKind::Rows) {
    px = world_size;
    py = 1;
  } else {
    auto d = dims_create(world_size, 2);
    px = d[0];
    py = d[1];
  }
  HEAT_CHECK(px <= nx && py <= ny, "process grid %dx%d larger than grid %lldx%lld", px, py,
             (long long)nx, (long long)ny);
}

int Cart::rank_of(int cx, int cy) const {
  if (cx < 0 || cx >= px || cy < 0 || cy >= py) return kNoNeighbor;
  return cx * py + cy;
}

int Cart::rank_of(int cx, int cy, unsigned periodic) const {
  if ((periodic & kPeriodicX) && px > 1) cx = (cx + px) % px;
  if ((periodic & kPeriodicY) && py > 1) cy = (cy + py) % py;
  return rank_of(cx, cy);
}

std::array<int, 4> Cart::neighbors(int rank, unsigned periodic) const {
  auto c = coords(rank);
  std::array<int, 4> n{};
  n[North] = rank_of(c[0] - 1, c[1], periodic);
  n[South] = rank_of(c[0] + 1, c[1], periodic);
  n[West] = rank_of(c[0], c[1] - 1, periodic);
  n[East] = rank_of(c[0], c[1] + 1, periodic);
  return n;
}

std::array<int, 4> Cart::diagonal_neighbors(int rank, unsigned periodic) const {
  auto c = coords(rank);
  std::array<int, 4> n{};
  n[NorthWest] = rank_of(c[0] - 1, c[1] - 1, periodic);
  n[NorthEast] = rank_of(c[0] - 1, c[1] + 1, periodic);
  n[SouthWest] = rank_of(c[0] + 1, c[1] - 1, periodic);
  n[SouthEast] = rank_of(c[0] + 1, c[1] + 1, periodic);
  return n;
}

Span block_span(int64_t n, int parts, int index) {
  HEAT_CHECK(parts >= 1 && index >= 0 && index < parts, "parts=%d index=%d", parts, index);
  const int64_t base = n / parts, rem = n % parts;
  Span s;
  s.size = base + (index < rem ? 1 : 0);
  s.offset = index * base + std::min<int64_t>(index, rem);
  return s;
}

Block make_block(const Cart& cart, int rank, int64_t nx, int64_t ny, unsigned periodic) {
  HEAT_CHECK(rank >= 0 && rank < cart.world, "rank %d of %d", rank, cart.world);
  Block b;
  b.rank = rank;
  auto c = cart.coords(rank);
  b.cx = c[0];
  b.cy = c[1];
  auto sx = block_span(nx, cart.px, b.cx);
  auto sy = block_span(ny, cart.py, b.cy);
  b.ox = sx.offset;
  b.lx = sx.size;
  b.oy = sy.offset;
  b.ly = sy.size;
  b.nbr = cart.neighbors(rank, periodic);
  b.diag = cart.diagonal_neighbors(rank, periodic);
  return b;
}

Layout Layout::make(int64_t lx, int64_t ly, int halo) {
  HEAT_CHECK(lx >= 1 && ly >= 1 && halo >= 1, "lx=%lld ly=%lld halo=%d", (long long)lx,
             (long long)ly, halo);
  Layout L;
  L.lx = lx;
  L.ly = ly;
  L.hx = halo;
  L.hy = int(round_up(halo, 4));  // keeps owned column 0 16-B aligned
  // Left ghost + owned + right ghost, plus one full 256-column strip of slack
  // for the TB kernel's last strip, rounded to 256 B.
  L.pitch = round_up(L.hy + ly + L.hy + 256, 64);
  L.rows = lx + 2 * int64_t(halo);
  return L;
}

Box span_box(const Cart& cart, const Block& b, int depth, int m, unsigned insulated,
             unsigned periodic) {
  const Sides s = make_sides(cart, b, insulated, periodic);
  GhostState g;
  g.refill(int64_t(m) * depth);
  const auto e = g.advance(s, depth, true);
  return grown_box(b.lx, b.ly, s, e.first, e.second);
}

Sides make_sides(const Cart& cart, const Block& b, unsigned insulated, unsigned periodic) {
  // A periodic axis is decomposed and both its sides are open, as if insulated.
  insulated |= periodic_sides(periodic);
  auto open = [&](int d) { return b.nbr[size_t(d)] >= 0 || ((insulated >> d) & 1) != 0; };
  return {{open(North), open(South), open(West), open(East)},
          cart.px > 1 || (insulated & 3) != 0, cart.py > 1 || (insulated & 12) != 0};
}

InteriorSplit interior_split(int64_t lx, int64_t ly, const std::array<int, 4>& nbr, int64_t band) {
  const int64_t r0 = nbr[North] >= 0 ? band : 0, r1 = nbr[South] >= 0 ? lx - band : lx;
  const int64_t c0 = nbr[West] >= 0 ? round_up(band, 4) : 0;
  const int64_t c1 = nbr[East] >= 0 ? round_down(ly - band, 4) : ly;
  return {{r0, r1, c0, c1}, {{0, r0, 0, ly}, {r1, lx, 0, ly}, {r0, r1, 0, c0}, {r0, r1, c1, ly}}};
}

int64_t halo_extent_limit(const Cart& cart, int64_t nx, int64_t ny, unsigned insulated,
                          unsigned periodic) {
  const bool ins_x = (insulated & 3) != 0, ins_y = (insulated & 12) != 0;
  const bool per_x = (periodic & kPeriodicX) != 0, per_y = (periodic & kPeriodicY) != 0;
  int64_t ext = INT64_MAX;
  for (int r = 0; r < cart.world; ++r) {
    const Block b = make_block(cart, r, nx, ny);
    if (cart.px > 1 || ins_x || per_x) ext = std::min(ext, b.lx - (ins_x ? 1 : 0));
    if (cart.py > 1 || ins_y || per_y) ext = std::min(ext, b.ly - (ins_y ? 1 : 0));
  }
  return ext;
}

int resident_halo_passes(const Cart& cart, int64_t nx, int64_t ny, int depth, int mmax,
                         const std::function<int(const Box&)>& shape, unsigned insulated,
                         unsigned periodic) {
  if ((cart.world < 2 && insulated == 0 && periodic == 0) || depth < 1) return 0;
  std::vector<Block> blocks;
  std::vector<int> own;
  for (int r = 0; r < cart.world; ++r) {
    blocks.push_back(make_block(cart, r, nx, ny, periodic));
    const Block& b = blocks.back();
    own.push_back(shape(Box{0, b.lx, 0, b.ly}));
    if (own.back() == 0) return 0;
  }
  const int64_t min_ext = halo_extent_limit(cart, nx, ny, insulated, periodic);
  for (int m = int(std::min<int64_t>(mmax, min_ext / depth)); m >= 2; --m) {
    bool ok = true;
    for (size_t i = 0; i < blocks.size() && ok; ++i)
      ok = shape(span_box(cart, blocks[i], depth, m, insulated, periodic)) == own[i];
    if (ok) return m;
  }
  return 0;
}

int resident_shape_static(const Box& box, int depth, int cus) {
  using namespace gpu::tbw;
  const TilePlan pl =
      resident_tile_plan(box, depth, cus, [](int i) { return kResidentOccGfx950[i]; });
  if (pl.rows == 0 || !tiles_at_least_depth(box.rows(), pl, depth)) return 0;
  return res_shape(pl.rows, pl.waves);
}

}  // namespace heat
