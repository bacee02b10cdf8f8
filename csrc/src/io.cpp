// Grid I/O: prtdat-compatible text, binary blocks, checksums.
#include "heat/io.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>

#include "heat/common.hpp"
#include "heat/init_fn.hpp"

namespace heat {

void format_6_1f(float v, std::string& out) {
  // v*10 is exact in double for every finite float (24 + 4 mantissa bits), so
  // rounding it with the current (nearest-even) mode reproduces printf's
  // correctly rounded "%.1f" exactly, ties included.
  if (!std::isfinite(v) || std::fabs(v) >= 1e15f) {
    char buf[64];
    int n = std::snprintf(buf, sizeof buf, "%6.1f", double(v));
    out.append(buf, size_t(n));
    return;
  }
  double q = std::nearbyint(double(v) * 10.0);
  bool neg = std::signbit(v);
  uint64_t m = uint64_t(std::fabs(q));
  char digits[24];
  int nd = 0;
  uint64_t ip = m / 10;
  digits[nd++] = char('0' + m % 10);
  digits[nd++] = '.';
  do {
    digits[nd++] = char('0' + ip % 10);
    ip /= 10;
  } while (ip);
  if (neg) digits[nd++] = '-';
  for (int pad = nd; pad < 6; ++pad) out.push_back(' ');
  for (int i = nd - 1; i >= 0; --i) out.push_back(digits[i]);
}

void write_dat(const std::string& path, int64_t nx, int64_t ny, const float* grid) {
  FILE* fp = std::fopen(path.c_str(), "w");
  HEAT_CHECK(fp != nullptr, "cannot open %s for writing", path.c_str());
  std::string line;
  line.reserve(size_t(nx) * 8 + 8);
  for (int64_t iy = ny - 1; iy >= 0; --iy) {
    line.clear();
    for (int64_t ix = 0; ix < nx; ++ix) {
      format_6_1f(grid[ix * ny + iy], line);
      line.push_back(ix != nx - 1 ? ' ' : '\n');
    }
    HEAT_CHECK(std::fwrite(line.data(), 1, line.size(), fp) == line.size(), "short write to %s",
               path.c_str());
  }
  HEAT_CHECK(std::fclose(fp) == 0, "close %s", path.c_str());
}

std::vector<float> read_dat(const std::string& path, int64_t* nx_out, int64_t* ny_out) {
  std::ifstream in(path);
  HEAT_CHECK(in.good(), "cannot open %s", path.c_str());
  std::vector<std::vector<float>> lines;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::vector<float> vals;
    const char* p = line.c_str();
    char* end = nullptr;
    while (true) {
      float v = std::strtof(p, &end);
      if (end == p) break;
      vals.push_back(v);
      p = end;
    }
    lines.push_back(std::move(vals));
  }
  const int64_t ny = int64_t(lines.size());
  HEAT_CHECK(ny > 0, "empty dat file %s", path.c_str());
  const int64_t nx = int64_t(lines[0].size());
  std::vector<float> g(size_t(nx * ny));
  for (int64_t l = 0; l < ny; ++l) {
    HEAT_CHECK(int64_t(lines[l].size()) == nx, "ragged dat file %s", path.c_str());
    const int64_t iy = ny - 1 - l;
    for (int64_t ix = 0; ix < nx; ++ix) g[ix * ny + iy] = lines[l][ix];
  }
  *nx_out = nx;
  *ny_out = ny;
  return g;
}

void bin_create(const std::string& path, const BinHeader& h) {
  int fd = ::open(path.c_str(), O_CREAT | O_TRUNC | O_WRONLY, 0644);
  HEAT_CHECK(fd >= 0, "cannot create %s", path.c_str());
  HEAT_CHECK(::pwrite(fd, &h, sizeof h, 0) == ssize_t(sizeof h), "header write %s", path.c_str());
  // Size the file so every rank can pwrite its own block.
  const off_t total = off_t(sizeof h) + off_t(h.nx) * off_t(h.ny) * 4;
  HEAT_CHECK(::ftruncate(fd, total) == 0, "ftruncate %s", path.c_str());
  ::close(fd);
}

void bin_write_block(const std::string& path, int64_t nx, int64_t ny, int64_t ox, int64_t oy,
                     int64_t lx, int64_t ly, const float* src, int64_t src_pitch) {
  HEAT_CHECK(ox >= 0 && oy >= 0 && ox + lx <= nx && oy + ly <= ny, "block out of range");
  int fd = ::open(path.c_str(), O_WRONLY);
  HEAT_CHECK(fd >= 0, "cannot open %s", path.c_str());
  for (int64_t r = 0; r < lx; ++r) {
    const off_t off = off_t(sizeof(BinHeader)) + (off_t(ox + r) * ny + oy) * 4;
    const ssize_t n = ssize_t(ly * 4);
    HEAT_CHECK(::pwrite(fd, src + r * src_pitch, size_t(n), off) == n, "row write %s",
               path.c_str());
  }
  // Each rank makes its own rows durable before the commit barrier: ranks of
  // a TCP run may sit on different hosts, where rank 0's fsync does not
  // reach their page caches.
  const int rc = ::fsync(fd);
  ::close(fd);
  HEAT_CHECK(rc == 0, "fsync %s", path.c_str());
}

void bin_commit(const std::string& tmp, const std::string& path) {
  // Every rank has fsynced its rows (bin_write_block) and passed the caller's
  // barrier: fsync the header, rename, then fsync the directory so the swap
  // itself survives a crash (the previous checkpoint stays valid until then).
  int fd = ::open(tmp.c_str(), O_RDONLY);
  HEAT_CHECK(fd >= 0, "cannot open %s", tmp.c_str());
  const int rc = ::fsync(fd);
  ::close(fd);
  HEAT_CHECK(rc == 0, "fsync %s", tmp.c_str());
  HEAT_CHECK(::rename(tmp.c_str(), path.c_str()) == 0, "rename %s -> %s", tmp.c_str(),
             path.c_str());
  const size_t slash = path.find_last_of('/');
  const std::string dir = slash == std::string::npos ? "." : (slash == 0 ? "/" : path.substr(0, slash));
  const int dfd = ::open(dir.c_str(), O_RDONLY | O_DIRECTORY);
  HEAT_CHECK(dfd >= 0, "cannot open directory %s", dir.c_str());
  const int drc = ::fsync(dfd);
  ::close(dfd);
  HEAT_CHECK(drc == 0, "fsync directory %s", dir.c_str());
}

BinHeader bin_read_header(const std::string& path) {
  BinHeader h{};
  int fd = ::open(path.c_str(), O_RDONLY);
  HEAT_CHECK(fd >= 0, "cannot open %s", path.c_str());
  HEAT_CHECK(::pread(fd, &h, sizeof h, 0) == ssize_t(sizeof h), "header read %s", path.c_str());
  ::close(fd);
  HEAT_CHECK(std::memcmp(h.magic, "HEATF32", 8) == 0 && h.version == 1,
             "%s is not a heat binary grid", path.c_str());
  return h;
}

void bin_read_block(const std::string& path, int64_t ox, int64_t oy, int64_t lx, int64_t ly,
                    float* dst, int64_t dst_pitch) {
  BinHeader h = bin_read_header(path);
  HEAT_CHECK(ox >= 0 && oy >= 0 && ox + lx <= h.nx && oy + ly <= h.ny, "block out of range");
  int fd = ::open(path.c_str(), O_RDONLY);
  HEAT_CHECK(fd >= 0, "cannot open %s", path.c_str());
  for (int64_t r = 0; r < lx; ++r) {
    const off_t off = off_t(sizeof(BinHeader)) + (off_t(ox + r) * h.ny + oy) * 4;
    const ssize_t n = ssize_t(ly * 4);
    HEAT_CHECK(::pread(fd, dst + r * dst_pitch, size_t(n), off) == n, "row read %s",
               path.c_str());
  }
  ::close(fd);
}

void Checksum::merge(const Checksum& o) {
  if (o.count == 0) return;
  if (count == 0) {
    min = o.min;
    max = o.max;
  } else {
    min = std::min(min, o.min);
    max = std::max(max, o.max);
  }
  hash += o.hash;
  sum += o.sum;
  count += o.count;
}

Checksum checksum_block(const float* src, int64_t src_pitch, int64_t ox, int64_t oy, int64_t lx,
                        int64_t ly, int64_t ny) {
  Checksum c;
  c.min = std::numeric_limits<double>::infinity();
  c.max = -std::numeric_limits<double>::infinity();
  for (int64_t r = 0; r < lx; ++r) {
    const float* row = src + r * src_pitch;
    double rs = 0.0;
    for (int64_t j = 0; j < ly; ++j) {
      uint32_t bits;
      std::memcpy(&bits, &row[j], 4);
      const uint64_t gidx = uint64_t(ox + r) * uint64_t(ny) + uint64_t(oy + j);
      c.hash += mix64(gidx * 0x100000001B3ull ^ bits);
      const double v = row[j];
      rs += v;
      c.min = std::min(c.min, v);
      c.max = std::max(c.max, v);
    }
    c.sum += rs;
  }
  c.count = lx * ly;
  return c;
}

void coarse_dims(int64_t nx, int64_t ny, int64_t fx, int64_t fy, int64_t* cr, int64_t* cc) {
  HEAT_CHECK(nx >= 1 && ny >= 1, "coarse view of a %lldx%lld plate", (long long)nx, (long long)ny);
  HEAT_CHECK(fx >= 1 && fy >= 1, "coarse factors %lldx%lld: a factor must be >= 1", (long long)fx,
             (long long)fy);
  const int64_t r = ceil_div(nx, fx), c = ceil_div(ny, fy);
  HEAT_CHECK(r <= kCoarseMaxCells && c <= kCoarseMaxCells && r * c <= kCoarseMaxCells,
             "coarse factors %lldx%lld give a %lldx%lld grid of a %lldx%lld plate: above the "
             "limit of %lld coarse cells (2^22)",
             (long long)fx, (long long)fy, (long long)r, (long long)c, (long long)nx, (long long)ny,
             (long long)kCoarseMaxCells);
  if (cr) *cr = r;
  if (cc) *cc = c;
}

void coarse_block(const float* origin, int64_t pitch, int64_t lx, int64_t ly, int64_t ox,
                  int64_t oy, int64_t nx, int64_t ny, int64_t fx, int64_t fy, double* sum,
                  float* mn, float* mx) {
  if (lx <= 0 || ly <= 0) return;
  HEAT_CHECK(fx >= 1 && fy >= 1 && ox >= 0 && oy >= 0 && ox + lx <= nx && oy + ly <= ny,
             "coarse of a %lldx%lld block at (%lld, %lld) of a %lldx%lld plate, factors %lldx%lld",
             (long long)lx, (long long)ly, (long long)ox, (long long)oy, (long long)nx,
             (long long)ny, (long long)fx, (long long)fy);
  const int64_t cc = ceil_div(ny, fy);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // Coarse row by coarse row, each column segment of a cell row by row.
  for (int64_t g = ox; g < ox + lx;) {
    const int64_t I = g / fx, g1 = std::min(ox + lx, fx > nx ? nx : (I + 1) * fx);
    for (int64_t h = oy; h < oy + ly;) {
      const int64_t J = h / fy, h1 = std::min(oy + ly, fy > ny ? ny : (J + 1) * fy);
      double s = 0.0;
      float lo = std::numeric_limits<float>::infinity(), hi = -lo;
      bool has_nan = false;
      for (int64_t r = g; r < g1; ++r) {
        const float* row = origin + (r - ox) * pitch;
        for (int64_t c = h; c < h1; ++c) {
          const float v = row[c - oy];
          s += double(v);
          lo = std::min(lo, v);
          hi = std::max(hi, v);
          has_nan |= v != v;
        }
      }
      const int64_t k = I * cc + J;
      sum[k] += s;
      mn[k] = (has_nan || mn[k] != mn[k]) ? nan : std::min(mn[k], lo);
      mx[k] = (has_nan || mx[k] != mx[k]) ? nan : std::max(mx[k], hi);
      h = h1;
    }
    g = g1;
  }
}

void refine_axis(int64_t n, int64_t f, int order, bool wrap, int64_t begin, int64_t count,
                 int32_t* i0, int32_t* i1, float* w) {
  HEAT_CHECK(n >= 1 && f >= 1 && (order == 0 || order == 1),
             "refine axis: n %lld, factor %lld, order %d", (long long)n, (long long)f, order);
  HEAT_CHECK(begin >= 0 && count >= 0 && begin + count <= n, "refine axis: [%lld, %lld) of %lld",
             (long long)begin, (long long)(begin + count), (long long)n);
  const int64_t C = ceil_div(n, f);
  HEAT_CHECK(C <= kCoarseMaxCells, "refine axis: %lld source cells", (long long)C);
  auto c2 = [&](int64_t I) { return I * f + std::min((I + 1) * f, n) - 1; };
  for (int64_t q = 0; q < count; ++q) {
    const int64_t i = begin + q;
    int64_t a, b;
    float wt = 0.f;
    if (order == 0) {
      a = b = i / f;
    } else {
      // The cell of i is I = i / f; c2 of the next cell is above 2i, c2 of the
      // one before is not: k is I or I - 1.
      const int64_t t = 2 * i, I = i / f, k = c2(I) <= t ? I : I - 1;
      if (k >= 0 && k < C - 1) {
        a = k;
        b = k + 1;
        wt = float(double(t - c2(k)) / double(c2(k + 1) - c2(k)));
      } else if (!wrap || C == 1) {
        a = b = k < 0 ? 0 : C - 1;
      } else {
        a = C - 1;
        b = 0;
        wt = float(double(t - c2(C - 1) + (k < 0 ? 2 * n : 0)) / double(c2(0) + 2 * n - c2(C - 1)));
      }
    }
    i0[q] = int32_t(a);
    i1[q] = int32_t(b);
    w[q] = wt;
  }
}

int64_t ghost_axis_index(int64_t i, int64_t n, bool wrap, bool mirror_lo, bool mirror_hi) {
  if (i >= 0 && i < n) return i;
  if (wrap) return ((i % n) + n) % n;
  const int64_t m = i < 0 ? (mirror_lo ? -i : 0) : (mirror_hi ? 2 * (n - 1) - i : n - 1);
  return std::min(std::max<int64_t>(m, 0), n - 1);  // a mirror deeper than the plate: clamped
}

void refine_axis_ext(int64_t n, int64_t f, int order, bool wrap, bool mirror_lo, bool mirror_hi,
                     int64_t begin, int64_t count, int32_t* i0, int32_t* i1, float* w) {
  HEAT_CHECK(n >= 1 && count >= 0, "refine axis: %lld entries of %lld cells", (long long)count,
             (long long)n);
  for (int64_t q = 0; q < count; ++q)
    refine_axis(n, f, order, wrap, ghost_axis_index(begin + q, n, wrap, mirror_lo, mirror_hi), 1,
                i0 + q, i1 + q, w + q);
}

void refine_check(int64_t nx, int64_t ny, int64_t cr, int64_t cc, int64_t fx, int64_t fy,
                  int order) {
  HEAT_CHECK(order == 0 || order == 1, "refine order %d: expected 0 or 1", order);
  int64_t r = 0, c = 0;
  coarse_dims(nx, ny, fx, fy, &r, &c);
  HEAT_CHECK(r == cr && c == cc,
             "refine: a %lldx%lld source grid does not fit factors %lldx%lld on a %lldx%lld plate, "
             "which need a %lldx%lld grid",
             (long long)cr, (long long)cc, (long long)fx, (long long)fy, (long long)nx,
             (long long)ny, (long long)r, (long long)c);
}

namespace {
inline float refine_lerp(float a, float b, float w) {
  return w == 0.f ? a : std::fmaf(w, b - a, a);
}
}  // namespace

void refine_block(float* origin, int64_t pitch, int64_t lx, int64_t ly, const float* S,
                  int64_t cc, const RefineTable& rows, const RefineTable& cols) {
  if (lx <= 0 || ly <= 0) return;
  HEAT_CHECK(origin && S && pitch >= ly && cc >= 1 && rows.i0 && rows.i1 && rows.w && cols.i0 &&
                 cols.i1 && cols.w,
             "refine of a %lldx%lld block", (long long)lx, (long long)ly);
  // The column pass of a source row pair is reused while the pair stays.
  std::vector<float> top(static_cast<size_t>(ly)), bot(static_cast<size_t>(ly));
  int32_t pa = -1, pb = -1;
  for (int64_t r = 0; r < lx; ++r) {
    const int32_t a = rows.i0[r], b = rows.i1[r];
    if (a != pa || b != pb) {
      const float* sa = S + int64_t(a) * cc;
      const float* sb = S + int64_t(b) * cc;
      for (int64_t c = 0; c < ly; ++c) {
        const int32_t j0 = cols.i0[c], j1 = cols.i1[c];
        top[size_t(c)] = refine_lerp(sa[j0], sa[j1], cols.w[c]);
        bot[size_t(c)] = refine_lerp(sb[j0], sb[j1], cols.w[c]);
      }
      pa = a;
      pb = b;
    }
    float* dst = origin + r * pitch;
    const float wx = rows.w[r];
    for (int64_t c = 0; c < ly; ++c) dst[c] = refine_lerp(top[size_t(c)], bot[size_t(c)], wx);
  }
}

}  // namespace heat
