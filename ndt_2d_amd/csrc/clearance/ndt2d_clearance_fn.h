// The arithmetic of the clearance map (clearance/ndt2d_clearance.hip; include/ndt2d_hip.h, "Clearance
// map"): which bytes are obstacles, the squared-distance threshold of a clearance in metres, the
// vertical distance of a cell inside a strip of 64 rows, and the row minimum of one cell.  Plain C++
// without HIP types, host and device: the kernels run it, and a stand-alone host program checks it
// against a 64-bit brute force (tests/cpp/clearance_fn_check.cpp).  Integers throughout; the one
// place metres enter is min_d2_of, in double, on the host.
#ifndef NDT2D_CLEARANCE_FN_H_
#define NDT2D_CLEARANCE_FN_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_CLEARANCE_HD __host__ __device__
#else
#define NDT2D_CLEARANCE_HD
#endif

namespace ndt2d
{
namespace clearance
{

constexpr uint32_t kFar = 0xFFFFFFFFu;     // NDT2D_CLEARANCE_FAR
constexpr uint16_t kNone = 0xFFFFu;        // g: no obstacle in the column; a strip summary: no obstacle row
constexpr uint32_t kMaxSide = 32768u;      // the widest and the tallest map
constexpr uint32_t kStrip = 64u;           // rows of a strip of the column pass: one bit each of a uint64
constexpr signed char kInscribed = 99;     // a masked cell (the nav2 costmap's "inscribed" value)

// An obstacle: a byte that is neither 0 (free) nor -1 (unknown); with unknown_is_obstacle any byte
// that is not 0.
NDT2D_CLEARANCE_HD inline bool is_obstacle(signed char value, bool unknown_is_obstacle)
{
  return value != 0 && (unknown_is_obstacle || value != -1);
}

// The cap as the kernels take it: 0 = none.  Every d2 is at most 2 * 32767^2 < 2^31, so a cap of
// 46,341 cells and above (R^2 > 2^31) removes nothing and is the same as none.
NDT2D_CLEARANCE_HD inline uint32_t effective_cap(int64_t max_cells)
{
  return max_cells > 0 && max_cells <= 46340 ? static_cast<uint32_t>(max_cells) : 0u;
}

// min_d2 of a clearance in metres: q = clearance / resolution (one double divide), ceil(q * q).
// false (refused, *out untouched): a clearance that is negative or not finite, a resolution that is
// not finite and positive, max_cells < 0, min_d2 above 2^31, or a cap R > 0 with min_d2 > R^2.
inline bool min_d2_of(double clearance_m, double resolution, int64_t max_cells, uint32_t * out)
{
  if (!(clearance_m >= 0.0) || !isfinite(clearance_m)) return false;
  if (!(resolution > 0.0) || !isfinite(resolution)) return false;
  if (max_cells < 0) return false;
  const double q = clearance_m / resolution;
  const double square = q * q;
  const double m = ceil(square);
  if (!(m <= 2147483648.0)) return false;          // (an infinite q * q lands here too)
  if (max_cells > 0)
  {
    // R^2 in double: exact below 2^53, and an R at which it is not exceeds every m that passed
    const double r = static_cast<double>(max_cells);
    if (m > r * r) return false;
  }
  *out = static_cast<uint32_t>(m);
  return true;
}

// A cell has the clearance exactly when d2 >= min_d2 (kFar always has it).
NDT2D_CLEARANCE_HD inline bool has_clearance(uint32_t d2, uint32_t min_d2) { return d2 >= min_d2; }

NDT2D_CLEARANCE_HD inline signed char masked(signed char value, uint32_t d2, uint32_t min_d2)
{
  return value == 0 && !has_clearance(d2, min_d2) ? kInscribed : value;
}

// ---- the column pass ----

NDT2D_CLEARANCE_HD inline int top_bit(uint64_t m)   // m != 0
{
  return 63 - __builtin_clzll(m);
}

NDT2D_CLEARANCE_HD inline int low_bit(uint64_t m)   // m != 0
{
  return __builtin_ctzll(m);
}

// g of row y0 + r (r < 64) of a column: `bits` has bit k set where row y0 + k is an obstacle; `up`
// is the nearest obstacle row above the strip and `down` the nearest below it (kNone: there is
// none).  Rows are below 32,768, so a distance is too and kNone is no distance.
NDT2D_CLEARANCE_HD inline uint16_t column_distance(uint64_t bits, uint32_t y0, uint32_t r, uint16_t up, uint16_t down)
{
  const uint32_t y = y0 + r;
  uint32_t best = kNone;
  const uint64_t at_or_above = bits & (~0ull >> (63u - r));
  if (at_or_above != 0)
  {
    best = r - static_cast<uint32_t>(top_bit(at_or_above));
  }
  else if (up != kNone)
  {
    best = y - up;
  }
  const uint64_t at_or_below = bits >> r;
  uint32_t other = kNone;
  if (at_or_below != 0)
  {
    other = static_cast<uint32_t>(low_bit(at_or_below));
  }
  else if (down != kNone)
  {
    other = down - y;
  }
  return static_cast<uint16_t>(other < best ? other : best);
}

// ---- the row pass ----

// d2 of cell x of a row whose vertical distances are g[width]: min over x' of (x - x')^2 + g[x']^2,
// by a scan outwards from x.  Every x' at distance dx and beyond gives at least dx^2, so the scan
// stops exactly at dx^2 >= best; under a cap R (0 = none) also at dx > R, since a cell whose exact d2
// is at most R^2 has its nearest obstacle within R columns, and every other cell is reported as kFar.
// The sum cannot overflow: dx <= 32767 and g <= 32767 (kNone is skipped), so dx^2 + g^2 <=
// 2 * 32767^2 = 2,147,352,578 < 2^31.
template <typename G>
NDT2D_CLEARANCE_HD inline uint32_t row_min(G g, uint32_t width, uint32_t x, uint32_t cap)
{
  uint32_t best = kFar;
  const uint32_t reach_left = x, reach_right = width - 1u - x;
  uint32_t reach = reach_left > reach_right ? reach_left : reach_right;
  if (cap != 0 && cap < reach) reach = cap;
  for (uint32_t dx = 0; dx <= reach; ++dx)
  {
    const uint32_t dx2 = dx * dx;
    if (dx2 >= best) break;
    if (dx <= reach_left)
    {
      const uint32_t v = g[x - dx];
      if (v != kNone)
      {
        const uint32_t cand = dx2 + v * v;
        if (cand < best) best = cand;
      }
    }
    if (dx != 0 && dx <= reach_right)
    {
      const uint32_t v = g[x + dx];
      if (v != kNone)
      {
        const uint32_t cand = dx2 + v * v;
        if (cand < best) best = cand;
      }
    }
  }
  if (cap != 0 && best > cap * cap) best = kFar;   // cap <= 46340: cap^2 < 2^31
  return best;
}

}  // namespace clearance
}  // namespace ndt2d

#endif  // NDT2D_CLEARANCE_FN_H_
