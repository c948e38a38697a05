// The arithmetic of the wide search's bound image (wide/ndt2d_wide.hip): the exact maximum of a
// cell's exponent over a rectangle, the pixel's value from the cells its box touches, the geometry
// of the image and the look-up of a point in it -- the contract of include/ndt2d_hip.h ("Wide
// search").  Plain C++ without HIP types, host and device: every thread of the image kernel runs it,
// and a stand-alone host program checks it (tests/cpp/wide_fn_check.cpp).  Every operation is
// written out in the order a restatement has to follow (tests/wide_restatement.py); sums and
// products round separately under a contraction-off pragma, whatever the flags of the translation
// unit.
#ifndef NDT2D_WIDE_FN_H_
#define NDT2D_WIDE_FN_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_WIDE_HD __host__ __device__
#else
#define NDT2D_WIDE_HD
#endif

// (g++ has no such pragma in C++: a GNU build passes -ffp-contract=off, as build.py and the tests do)
#if defined(__clang__)
#define NDT2D_WIDE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NDT2D_WIDE_NO_CONTRACT
#endif

namespace ndt2d
{
namespace wide
{

constexpr double kGuard = 1.0e-9;                       // metres round a box and round a cell
constexpr double kInflate = 1.0 + 0x1.0p-40;            // of a pixel's value
constexpr double kFloor = 0x1.0p-1000;                  // added to the value of a pixel whose box meets a scoring cell
constexpr uint32_t kMaxBoxCells = 8;                    // cells a box may touch per axis
constexpr uint64_t kMaxPixels = 1ull << 26;
constexpr uint32_t kMaxTileSteps = 32;
constexpr uint32_t kMaxPixelsPerTile = 8;

// Cell::score's exponent on a packed record (h = -0.5 information), the roundings of
// record_exponent (ndt2d_device_fn.h).
NDT2D_WIDE_HD inline double exponent_at(double mx, double my, double h00, double h01, double h11, double px, double py)
{
  NDT2D_WIDE_NO_CONTRACT
  const double q0 = px - mx;
  const double q1 = py - my;
  const double a0 = q0 * h00;
  const double a1 = q1 * h01;
  const double r0 = a0 + a1;
  const double b0 = q0 * h01;
  const double b1 = q1 * h11;
  const double r1 = b0 + b1;
  const double t0 = r0 * q0;
  const double t1 = r1 * q1;
  return t0 + t1;
}

NDT2D_WIDE_HD inline bool record_finite(double mx, double my, double h00, double h01, double h11)
{
  const double s = ((((mx - mx) + (my - my)) + (h00 - h00)) + (h01 - h01)) + (h11 - h11);   // NaN for any inf / NaN
  return s == 0.0;
}

// v into the running maximum; a NaN value (products of a finite record that overflowed against
// each other) counts as +inf: the bound must not drop it.
NDT2D_WIDE_HD inline double take_max(double best, double v)
{
  if (v != v) return HUGE_VAL;
  return v > best ? v : best;
}

NDT2D_WIDE_HD inline double clamp_to(double v, double lo, double hi)
{
  return v < lo ? lo : (v > hi ? hi : v);
}

// The maximum of the exponent over [x0, x1] x [y0, y1] (x0 <= x1, y0 <= y1, finite record): the
// largest of the four corners, the stationary point of each edge clamped to the edge, and the
// interior stationary point -- the mean, where the exponent is 0 -- when it lies in the rectangle.
// Along an edge the exponent is a parabola in one variable: where it opens upwards or is a line
// (h00 >= 0 on a horizontal edge, h11 >= 0 on a vertical one) its ends hold the maximum, so the
// stationary point is asked for only where it opens downwards.  Inside, a maximum that is not on
// the boundary needs h negative definite, and then lies at the mean.
NDT2D_WIDE_HD inline double box_max_exponent(double mx, double my, double h00, double h01, double h11, double x0,
                                             double x1, double y0, double y1)
{
  NDT2D_WIDE_NO_CONTRACT
  double best = exponent_at(mx, my, h00, h01, h11, x0, y0);
  if (best != best) best = HUGE_VAL;
  best = take_max(best, exponent_at(mx, my, h00, h01, h11, x0, y1));
  best = take_max(best, exponent_at(mx, my, h00, h01, h11, x1, y0));
  best = take_max(best, exponent_at(mx, my, h00, h01, h11, x1, y1));
  if (h00 < 0.0)
  {
    for (int k = 0; k < 2; ++k)
    {
      const double yc = k == 0 ? y0 : y1;
      const double q1 = yc - my;
      const double num = h01 * q1;
      const double off = -num / h00;
      const double xs = clamp_to(mx + off, x0, x1);
      best = take_max(best, exponent_at(mx, my, h00, h01, h11, xs, yc));
    }
  }
  if (h11 < 0.0)
  {
    for (int k = 0; k < 2; ++k)
    {
      const double xc = k == 0 ? x0 : x1;
      const double q0 = xc - mx;
      const double num = h01 * q0;
      const double off = -num / h11;
      const double ys = clamp_to(my + off, y0, y1);
      best = take_max(best, exponent_at(mx, my, h00, h01, h11, xc, ys));
    }
  }
  if (mx >= x0 && mx <= x1 && my >= y0 && my <= y1) best = take_max(best, 0.0);
  return best;
}

// The installed grid as ndt2d_grid_view_get shows it (stride: doubles per record).
struct GridRef
{
  const double * cells;        // [ncell + 1][stride]: {mean_x, mean_y, h00, h01, h11, ...}
  const uint32_t * occ_bits;   // bit i: cell i can score (n >= 5)
  uint32_t stride;
  uint32_t size_x, size_y;
  double cell_size, origin_x, origin_y;
};

// The image: pixel (i, j) stands for the box [x_i - g, x_i + pitch + window + g] x [y_j - g, ...]
// with x_i = origin_x + i pitch.
struct Image
{
  double origin_x, origin_y;   // grid origin - (window + pitch)
  double pitch, inv_pitch, window;
  uint32_t nx, ny;
};

// pitch = max(window, cell_size / 4) / pixels_per_tile; nx = floor((extent + window + pitch) / pitch) + 2:
// every box that touches the grid has a pixel.
NDT2D_WIDE_HD inline double pitch_of(double window, double cell_size, uint32_t pixels_per_tile)
{
  const double quarter = cell_size / 4.0;
  const double span = window > quarter ? window : quarter;
  return span / static_cast<double>(pixels_per_tile);
}

// (extent_cells * cell_size + window + pitch) / pitch, floored, + 2 -- as a double, so that the
// caller can refuse an image that is too large before anything is converted
NDT2D_WIDE_HD inline double pixels_along(uint32_t extent_cells, double cell_size, double window, double pitch)
{
  NDT2D_WIDE_NO_CONTRACT
  const double extent = static_cast<double>(extent_cells) * cell_size;
  const double reach = window + pitch;
  const double span = extent + reach;
  return floor(span / pitch) + 2.0;
}

// cells a box touches along an axis, at most
NDT2D_WIDE_HD inline double box_cells_along(double window, double pitch, double cell_size)
{
  NDT2D_WIDE_NO_CONTRACT
  const double reach = window + pitch;
  const double width = reach + 2.0 * kGuard;
  return floor(width / cell_size) + 2.0;
}

// first and last cell of [lo, hi] (both already widened by the guard) along an axis of `size`
// cells, clamped to the grid; false: none
NDT2D_WIDE_HD inline bool cell_range(double lo, double hi, double origin, double cell_size, uint32_t size, uint32_t & c0,
                                     uint32_t & c1)
{
  NDT2D_WIDE_NO_CONTRACT
  const double f0 = floor((lo - origin) / cell_size);
  const double f1 = floor((hi - origin) / cell_size);
  const double last = static_cast<double>(size) - 1.0;
  if (!(f1 >= 0.0) || !(f0 <= last)) return false;   // (NaN: none)
  c0 = f0 > 0.0 ? static_cast<uint32_t>(f0) : 0u;
  c1 = f1 < last ? static_cast<uint32_t>(f1) : size - 1u;
  return true;
}

// The value of pixel (i, j) before inflation: the largest likelihood any point of its box can have.
// *touched: the box meets a cell that can score.
NDT2D_WIDE_HD inline double pixel_value_raw(const GridRef & g, const Image & im, uint32_t i, uint32_t j, bool * touched = nullptr)
{
  NDT2D_WIDE_NO_CONTRACT
  if (touched != nullptr) *touched = false;
  const double xi = im.origin_x + static_cast<double>(i) * im.pitch;
  const double yj = im.origin_y + static_cast<double>(j) * im.pitch;
  const double reach = im.pitch + im.window;
  const double bx0 = xi - kGuard, bx1 = (xi + reach) + kGuard;
  const double by0 = yj - kGuard, by1 = (yj + reach) + kGuard;
  uint32_t cx0, cx1, cy0, cy1;
  if (!cell_range(bx0 - kGuard, bx1 + kGuard, g.origin_x, g.cell_size, g.size_x, cx0, cx1)) return 0.0;
  if (!cell_range(by0 - kGuard, by1 + kGuard, g.origin_y, g.cell_size, g.size_y, cy0, cy1)) return 0.0;
  double best = 0.0;
  for (uint32_t cy = cy0; cy <= cy1; ++cy)
  {
    // the cell inflated by the guard, cut with the box
    const double ly = g.origin_y + static_cast<double>(cy) * g.cell_size - kGuard;
    const double hy = g.origin_y + static_cast<double>(cy + 1u) * g.cell_size + kGuard;
    const double y0 = ly > by0 ? ly : by0, y1 = hy < by1 ? hy : by1;
    if (!(y0 <= y1)) continue;
    for (uint32_t cx = cx0; cx <= cx1; ++cx)
    {
      const uint32_t cell = cy * g.size_x + cx;
      if (((g.occ_bits[cell >> 5] >> (cell & 31u)) & 1u) == 0u) continue;   // n < 5: Cell::score gives 0
      const double lx = g.origin_x + static_cast<double>(cx) * g.cell_size - kGuard;
      const double hx = g.origin_x + static_cast<double>(cx + 1u) * g.cell_size + kGuard;
      const double x0 = lx > bx0 ? lx : bx0, x1 = hx < bx1 ? hx : bx1;
      if (!(x0 <= x1)) continue;
      const double * r = g.cells + static_cast<size_t>(cell) * g.stride;
      const double mx = r[0], my = r[1], h00 = r[2], h01 = r[3], h11 = r[4];
      // a non-finite record gives its candidates a NaN score, which cannot win
      if (!record_finite(mx, my, h00, h01, h11)) continue;
      const double e = box_max_exponent(mx, my, h00, h01, h11, x0, x1, y0, y1);
      const double v = exp(e);
      best = take_max(best, v);
      if (touched != nullptr) *touched = true;
    }
  }
  return best;
}

NDT2D_WIDE_HD inline double pixel_value(const GridRef & g, const Image & im, uint32_t i, uint32_t j)
{
  NDT2D_WIDE_NO_CONTRACT
  bool touched;
  const double raw = pixel_value_raw(g, im, i, j, &touched);
  if (!touched) return 0.0;
  // (the floor: a relative inflation does nothing for a value that exp() left subnormal or flushed
  // to 0, where two correctly working exp() differ by a whole unit)
  const double inflated = raw * kInflate;
  return inflated + kFloor;
}

// The pixel of a point (the lower corner of a tile's copy of a beam), or false off the image (NaN
// included): such a beam adds 0.
NDT2D_WIDE_HD inline bool pixel_of(const Image & im, double px, double py, uint32_t & i, uint32_t & j)
{
  NDT2D_WIDE_NO_CONTRACT
  const double fx = (px - im.origin_x) * im.inv_pitch;
  const double fy = (py - im.origin_y) * im.inv_pitch;
  if (!(fx >= 0.0) || !(fy >= 0.0) || !(fx < static_cast<double>(im.nx)) || !(fy < static_cast<double>(im.ny))) return false;
  i = static_cast<uint32_t>(fx);
  j = static_cast<uint32_t>(fy);
  return true;
}

// A tile's bound from the sum of its beams' pixels: the sum of n_beams terms rounds n_beams - 1
// times here and as often in the exact walk.
NDT2D_WIDE_HD inline double tile_bound(double pixel_sum, uint32_t n_beams)
{
  NDT2D_WIDE_NO_CONTRACT
  const double slack = 1.0 + static_cast<double>(n_beams + 2u) * 0x1.0p-51;
  return pixel_sum * slack;
}

}  // namespace wide
}  // namespace ndt2d

#endif  // NDT2D_WIDE_FN_H_
