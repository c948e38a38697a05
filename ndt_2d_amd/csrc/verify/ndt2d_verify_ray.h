// The ray of the match verification (verify/ndt2d_verify_kernel.h): the integer line from the job's
// origin cell to a beam's own cell, and the closest approach of the segment robot -> beam end to a
// cell's Gaussian -- the contract of include/ndt2d_hip.h ("Match verification", "The ray").  Plain
// C++ without HIP types, host and device: every lane of the kernel runs it for its beam, and a
// stand-alone host program checks it (tests/cpp/verify_ray_check.cpp).  Every operation is written
// out in the order a restatement has to follow; the translation units are compiled with
// -ffp-contract=off.
#ifndef NDT2D_VERIFY_RAY_H_
#define NDT2D_VERIFY_RAY_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_VERIFY_HD __host__ __device__
#else
#define NDT2D_VERIFY_HD
#endif

namespace ndt2d
{
namespace verify
{

// A grid side the line's 32-bit error term takes (2 err stays far below 2^31).
constexpr uint32_t kMaxGridSide = 1u << 24;

// The line between two cells, at one of its cells: the all-octant error form of
// src/occupancy_grid.cpp:93-131.
struct Line
{
  int32_t x, y;            // the cell now visited
  int32_t end_x, end_y;
  int32_t dx, dy;          // |end_x - ox|, -|end_y - oy|
  int32_t sx, sy;
  int32_t err;
  uint32_t max_cells;      // dx - dy + 1: no line visits more cells
};

NDT2D_VERIFY_HD inline int32_t magnitude(int32_t v) { return v < 0 ? -v : v; }

// The line at its first cell, the origin (ox, oy).
NDT2D_VERIFY_HD inline Line line_begin(int32_t ox, int32_t oy, int32_t gx, int32_t gy)
{
  Line l;
  l.x = ox;
  l.y = oy;
  l.end_x = gx;
  l.end_y = gy;
  l.dx = magnitude(gx - ox);
  l.dy = -magnitude(gy - oy);
  l.sx = ox < gx ? 1 : -1;
  l.sy = oy < gy ? 1 : -1;
  l.err = l.dx + l.dy;
  l.max_cells = static_cast<uint32_t>(l.dx - l.dy + 1);
  return l;
}

// From the cell now visited to the next one: false when the walk is over.
NDT2D_VERIFY_HD inline bool line_next(Line & l)
{
  if (l.x == l.end_x && l.y == l.end_y) return false;
  if (2 * l.err >= l.dy)
  {
    if (l.x == l.end_x) return false;
    l.err += l.dy;
    l.x += l.sx;
  }
  if (2 * l.err <= l.dx)
  {
    if (l.y == l.end_y) return false;
    l.err += l.dx;
    l.y += l.sy;
  }
  return true;
}

// Chebyshev distance of the cell now visited to the end cell.  It never grows along the line: once
// it is <= 1 no later cell is tested.
NDT2D_VERIFY_HD inline int32_t line_to_end(const Line & l)
{
  const int32_t ax = magnitude(l.end_x - l.x), ay = magnitude(l.end_y - l.y);
  return ax > ay ? ax : ay;
}

// May the cell now visited be tested (if it can score): not the origin cell (ox, oy), and outside
// the end's own 3 x 3.
NDT2D_VERIFY_HD inline bool line_cell_testable(const Line & l, int32_t ox, int32_t oy)
{
  return !(l.x == ox && l.y == oy) && line_to_end(l) > 1;
}

// r^T I r at the closest approach (in the cell's own metric) of the segment o -> q to the mean m:
// u = q - o, w = m - o, I = (i00, i01, i11).
NDT2D_VERIFY_HD inline double approach(double ux, double uy, double wx, double wy, double i00, double i01, double i11)
{
  const double iu0 = i00 * ux + i01 * uy;
  const double iu1 = i01 * ux + i11 * uy;
  const double D = ux * iu0 + uy * iu1;
  const double N = wx * iu0 + wy * iu1;
  double t = N / D;
  if (!(D > 0.0)) t = 0.0;
  if (!(t >= 0.0)) t = 0.0;
  else if (t > 1.0) t = 1.0;
  const double rx = wx - t * ux;
  const double ry = wy - t * uy;
  const double ir0 = i00 * rx + i01 * ry;
  const double ir1 = i01 * rx + i11 * ry;
  return rx * ir0 + ry * ir1;
}

NDT2D_VERIFY_HD inline bool pierces(double rIr, double gate_pierce) { return rIr <= gate_pierce; }

}  // namespace verify
}  // namespace ndt2d

#endif  // NDT2D_VERIFY_RAY_H_
