// The arithmetic of global localisation's seeder (seed/ndt2d_seed.hip): the pick of a free cell from
// the uniforms of particles/ndt2d_philox.h, the cell -> pose arithmetic and the free flag of the table's
// compaction (particles/ndt2d_compact.h) -- the contract of include/ndt2d_hip.h ("Global localisation").
// Plain C++ without HIP types, host and device: every thread of the kernels runs it, and a
// stand-alone host program checks it (tests/cpp/seed_fn_check.cpp).  Every operation is written out
// in the order a restatement has to follow (tests/seed_restatement.py); a sum and a product that
// must round separately are separate statements under a contraction-off pragma, whatever the flags
// of the translation unit.
#ifndef NDT2D_SEED_FN_H_
#define NDT2D_SEED_FN_H_

#include <stdint.h>

#include "../particles/ndt2d_philox.h"   // (relative: a stand-alone check needs this directory alone on its path)

#if defined(__HIPCC__)
#define NDT2D_SEED_HD __host__ __device__
#else
#define NDT2D_SEED_HD
#endif

// (g++ has no such pragma in C++: a GNU build passes -ffp-contract=off, as build.py and the tests do)
#if defined(__clang__)
#define NDT2D_SEED_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NDT2D_SEED_NO_CONTRACT
#endif

namespace ndt2d
{
namespace seed
{

constexpr double kPi = 3.14159265358979323846;       // the double M_PI
constexpr double kTwoPi = 2.0 * kPi;                 // exact: a power of two times M_PI
// The index into free_cells[n_free] (n_free in 1 .. 2^31 - 1): one double multiply, truncation,
// and the clamp that rounding of the product to n_free would need.
NDT2D_SEED_HD inline uint64_t pick(double u, uint64_t n_free)
{
  const double scaled = u * static_cast<double>(n_free);
  const uint64_t k = static_cast<uint32_t>(scaled);   // scaled <= n_free < 2^31: a 32-bit conversion
  return k < n_free - 1 ? k : n_free - 1;
}

// origin + (cell + u) * resolution: one add, one multiply, one add, each rounded on its own.
NDT2D_SEED_HD inline double coordinate(double origin, uint32_t cell, double u, double resolution)
{
  NDT2D_SEED_NO_CONTRACT
  const double in_cells = static_cast<double>(cell) + u;
  const double metres = in_cells * resolution;
  const double out = origin + metres;
  return out;
}

// -pi + (2 pi) u: one multiply, one add.  u = uniform24: the result lies in (-pi, pi).
NDT2D_SEED_HD inline double heading(double u)
{
  NDT2D_SEED_NO_CONTRACT
  const double turn = kTwoPi * u;
  const double out = -kPi + turn;
  return out;
}

struct Geometry
{
  double origin_x, origin_y, resolution;
  uint32_t width;
};

struct Sample
{
  double x, y, theta;
  double inject;   // the inject draw, in [0, 1)
};

// Particle `index` (global: first_index + i) at (seed, step): block A = counter (index, step) gives
// the cell and the offsets in it, block B = counter (index, step + 1) the heading and the inject
// draw.  A function of (seed, step, index, table, geometry) and nothing else.
NDT2D_SEED_HD inline Sample sample(uint64_t seed, uint64_t step, uint64_t index,
                                   const uint32_t * free_cells, uint64_t n_free, const Geometry & g)
{
  uint32_t a[4], b[4];
  particles::philox4x32_10(seed, index, step, a);
  particles::philox4x32_10(seed, index, step + 1, b);
  const uint32_t cell = free_cells[pick(particles::uniform53(a[0], a[1]), n_free)];
  const uint32_t cy = cell / g.width;
  const uint32_t cx = cell - cy * g.width;
  Sample s;
  s.x = coordinate(g.origin_x, cx, particles::uniform24(a[2]), g.resolution);
  s.y = coordinate(g.origin_y, cy, particles::uniform24(a[3]), g.resolution);
  s.theta = heading(particles::uniform24(b[0]));
  s.inject = particles::uniform53(b[1], b[2]);
  return s;
}

// ---- the free table ----

// A cell is free when its byte is exactly 0 (-1 unknown, 100 occupied, anything else: not free).
NDT2D_SEED_HD inline bool is_free(signed char value) { return value == 0; }

// Item i of the region {x0, y0, w, h}, row by row: its row-major index in the map.  Ascending in i.
NDT2D_SEED_HD inline uint32_t region_cell(uint32_t i, uint32_t x0, uint32_t y0, uint32_t w, uint32_t width)
{
  const uint32_t row = i / w;
  const uint32_t col = i - row * w;
  return (y0 + row) * width + (x0 + col);
}

}  // namespace seed
}  // namespace ndt2d

#endif  // NDT2D_SEED_FN_H_
