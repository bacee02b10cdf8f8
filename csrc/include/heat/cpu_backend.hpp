// CPU reference backend (serial / OpenMP).  This is the test oracle and the
// analogue of the reference's MPI/OpenMP loop nests
// (mpi/mpi_heat_improved_persistent_stat.c:162-234, OpenMP pragmas at
// :163-165, :181-183, :210-212).  It evaluates the same FMA expression as the
// GPU kernels (heat::stencil) and is therefore bitwise identical to them.
#pragma once

#include <cstdint>

#include "heat/topology.hpp"

namespace heat::cpu {

struct Geom {
  int64_t pitch = 0;
  int64_t gx0 = 0, gy0 = 0;
  int64_t nx = 0, ny = 0;
  float cx = 0.1f, cy = 0.1f;
  int numerics = 0;  // heat::Numerics
};
// The same geometry from a struct with fields of these names (the solver's
// gpu::StencilGeom, which this header does not see), field by field.
template <class G>
Geom geom_of(const G& s) {
  Geom g;
  g.pitch = s.pitch;
  g.gx0 = s.gx0;
  g.gy0 = s.gy0;
  g.nx = s.nx;
  g.ny = s.ny;
  g.cx = s.cx;
  g.cy = s.cy;
  g.numerics = s.numerics;
  return g;
}

void set_threads(int n);
int get_threads();

// Fill every allocated cell of a host field with the initial condition.
void init_field(float* origin, const Layout& L, int64_t gx0, int64_t gy0, int64_t nx, int64_t ny,
                int mode, uint64_t seed);

// One Jacobi step over box; returns max |new-old| over the box (as float;
// NaN if any cell became NaN) when want_resid, else 0.
float step(const float* src, float* dst, const Geom& g, const Box& box, bool want_resid);

// Host twin of gpu::source_step (kernels.hpp): the same step with a static
// per-cell source q in the layout of src and dst,
//   u' = heat::stencil(c, n, s, w, e, cx, cy) + q
// one rounded fp32 add after the unchanged FMA expression; a cell the step
// does not update ignores q.  fp32 numerics only.
float step_source(const float* src, float* dst, const float* q, const Geom& g, const Box& box,
                  bool want_resid);

// Host twin of gpu::fill_insulated_ghosts (kernels.hpp): mirror the field
// into the `depth`-deep ghost frame beyond the insulated sides in `sides`.
void fill_insulated_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int sides,
                           int depth);
// Host twin of gpu::fill_edge_ghosts: also wrap the field into the frame
// beyond both sides of the axes in `periodic_axes` (1 x, 2 y).
void fill_edge_ghosts(float* origin, int64_t pitch, int64_t lx, int64_t ly, int insulated_sides,
                      int periodic_axes, int depth);

void copy_box(const float* src, int64_t src_pitch, float* dst, int64_t dst_pitch, const Box& box);

}  // namespace heat::cpu
