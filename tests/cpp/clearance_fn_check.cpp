// csrc/clearance/ndt2d_clearance_fn.h in a program of its own: the obstacle predicate over every byte,
// min_d2 from metres against the table of include/ndt2d_hip.h and its refusals, the column distance of
// the strips (bits, first / last obstacle row, the carry across strips -- the steps of the kernels,
// run here in plain loops) and the row minimum against a 64-bit brute force over all obstacles, with
// and without a cap, and the largest sum the row minimum can form.  Prints a line per group and "ok".
// Built by tests/test_clearance_restatement.py with the host compiler, plainly and with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ndt2d_clearance_fn.h"

namespace fn = ndt2d::clearance;

namespace
{

int failures = 0;

#define CHECK(cond)                                                    \
  do                                                                   \
  {                                                                    \
    if (!(cond))                                                       \
    {                                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// a small generator of its own (the check does not depend on the library's)
struct Lcg
{
  std::uint64_t s;
  std::uint32_t next()
  {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<std::uint32_t>(s >> 33);
  }
  double unit() { return next() / 2147483648.0; }
};

// the column pass as the three kernels run it, one column at a time
std::vector<std::uint16_t> column_pass(const std::vector<signed char> & map, std::uint32_t width, std::uint32_t height,
                                       bool unknown)
{
  const std::uint32_t n_strips = (height + fn::kStrip - 1) / fn::kStrip;
  std::vector<std::uint64_t> bits(static_cast<std::size_t>(n_strips) * width);
  std::vector<std::uint16_t> first(bits.size()), last(bits.size()), g(static_cast<std::size_t>(width) * height);
  for (std::uint32_t s = 0; s < n_strips; ++s)
  {
    for (std::uint32_t x = 0; x < width; ++x)
    {
      const std::uint32_t y0 = s * fn::kStrip;
      const std::uint32_t rows = height - y0 < fn::kStrip ? height - y0 : fn::kStrip;
      std::uint64_t m = 0;
      for (std::uint32_t r = 0; r < rows; ++r)
      {
        m |= static_cast<std::uint64_t>(fn::is_obstacle(map[static_cast<std::size_t>(y0 + r) * width + x], unknown)) << r;
      }
      const std::size_t at = static_cast<std::size_t>(s) * width + x;
      bits[at] = m;
      first[at] = m != 0 ? static_cast<std::uint16_t>(y0 + fn::low_bit(m)) : fn::kNone;
      last[at] = m != 0 ? static_cast<std::uint16_t>(y0 + fn::top_bit(m)) : fn::kNone;
    }
  }
  for (std::uint32_t x = 0; x < width; ++x)
  {
    std::uint16_t carry = fn::kNone;
    for (std::uint32_t s = 0; s < n_strips; ++s)
    {
      const std::size_t at = static_cast<std::size_t>(s) * width + x;
      const std::uint16_t own = last[at];
      last[at] = carry;
      if (own != fn::kNone) carry = own;
    }
    carry = fn::kNone;
    for (std::uint32_t s = n_strips; s-- > 0;)
    {
      const std::size_t at = static_cast<std::size_t>(s) * width + x;
      const std::uint16_t own = first[at];
      first[at] = carry;
      if (own != fn::kNone) carry = own;
    }
  }
  for (std::uint32_t s = 0; s < n_strips; ++s)
  {
    for (std::uint32_t x = 0; x < width; ++x)
    {
      const std::uint32_t y0 = s * fn::kStrip;
      const std::uint32_t rows = height - y0 < fn::kStrip ? height - y0 : fn::kStrip;
      const std::size_t at = static_cast<std::size_t>(s) * width + x;
      for (std::uint32_t r = 0; r < rows; ++r)
      {
        g[static_cast<std::size_t>(y0 + r) * width + x] = fn::column_distance(bits[at], y0, r, last[at], first[at]);
      }
    }
  }
  return g;
}

// the contract by brute force: 64-bit, over every obstacle
std::uint32_t brute(const std::vector<signed char> & map, std::uint32_t width, std::uint32_t height, bool unknown,
                    std::uint32_t x, std::uint32_t y, std::int64_t cap)
{
  std::int64_t best = -1;
  for (std::uint32_t v = 0; v < height; ++v)
  {
    for (std::uint32_t u = 0; u < width; ++u)
    {
      if (!fn::is_obstacle(map[static_cast<std::size_t>(v) * width + u], unknown)) continue;
      const std::int64_t dx = static_cast<std::int64_t>(x) - u, dy = static_cast<std::int64_t>(y) - v;
      const std::int64_t d = dx * dx + dy * dy;
      if (best < 0 || d < best) best = d;
    }
  }
  if (best < 0) return fn::kFar;
  if (cap > 0 && best > cap * cap) return fn::kFar;
  return static_cast<std::uint32_t>(best);
}

void check_map(std::uint32_t width, std::uint32_t height, double density, std::uint64_t seed, std::uint64_t * sum)
{
  Lcg rng{seed};
  const signed char values[6] = {100, -1, 1, 50, -2, 99};
  std::vector<signed char> map(static_cast<std::size_t>(width) * height, 0);
  for (signed char & c : map)
  {
    if (rng.unit() < density) c = values[rng.next() % 6];
  }
  for (int unknown = 0; unknown < 2; ++unknown)
  {
    const std::vector<std::uint16_t> g = column_pass(map, width, height, unknown != 0);
    for (std::int64_t cap : {std::int64_t(0), std::int64_t(1), std::int64_t(5), std::int64_t(46340), std::int64_t(46341)})
    {
      for (std::uint32_t y = 0; y < height; ++y)
      {
        for (std::uint32_t x = 0; x < width; ++x)
        {
          const std::uint32_t got =
            fn::row_min(g.data() + static_cast<std::size_t>(y) * width, width, x, fn::effective_cap(cap));
          const std::uint32_t want = brute(map, width, height, unknown != 0, x, y, cap);
          if (got != want)
          {
            std::printf("FAILED %ux%u seed %llu unknown %d cap %lld at (%u, %u): %u, not %u\n", width, height,
                        static_cast<unsigned long long>(seed), unknown, static_cast<long long>(cap), x, y, got, want);
            ++failures;
            return;
          }
          if (cap == 0) *sum += got == fn::kFar ? 1u : got;
        }
      }
    }
  }
}

}  // namespace

int main()
{
  // the predicate, over every byte
  int n_obstacles = 0, n_with_unknown = 0;
  for (int v = -128; v <= 127; ++v)
  {
    const signed char c = static_cast<signed char>(v);
    CHECK(fn::is_obstacle(c, false) == (v != 0 && v != -1));
    CHECK(fn::is_obstacle(c, true) == (v != 0));
    n_obstacles += fn::is_obstacle(c, false);
    n_with_unknown += fn::is_obstacle(c, true);
  }
  std::printf("obstacle bytes %d, with unknown %d\n", n_obstacles, n_with_unknown);

  // metres
  const double table[5][3] = {{0.25, 0.05, 25}, {0.3, 0.05, 36}, {0.3, 0.1, 9}, {0.15, 0.05, 9}, {1.0, 0.02, 2500}};
  for (const double * row : table)
  {
    std::uint32_t m = 12345;
    CHECK(fn::min_d2_of(row[0], row[1], 0, &m) && m == static_cast<std::uint32_t>(row[2]));
    std::printf("min_d2 %g / %g = %u\n", row[0], row[1], m);
  }
  {
    std::uint32_t m = 777;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(fn::min_d2_of(0.0, 0.05, 0, &m) && m == 0);
    m = 777;
    CHECK(!fn::min_d2_of(-0.1, 0.05, 0, &m) && !fn::min_d2_of(nan, 0.05, 0, &m) && !fn::min_d2_of(inf, 0.05, 0, &m));
    CHECK(!fn::min_d2_of(0.3, 0.0, 0, &m) && !fn::min_d2_of(0.3, -1.0, 0, &m) && !fn::min_d2_of(0.3, nan, 0, &m) &&
          !fn::min_d2_of(0.3, inf, 0, &m));
    CHECK(!fn::min_d2_of(0.3, 0.05, -1, &m));
    CHECK(!fn::min_d2_of(1e300, 1e-300, 0, &m));                      // q * q overflows to infinity
    CHECK(m == 777);                                                  // a refusal writes nothing
    CHECK(fn::min_d2_of(46340.95, 1.0, 0, &m) && m == 2147483647u);   // 46340.95^2 = 2147483646.9...
    CHECK(fn::min_d2_of(46340.95001, 1.0, 0, &m) && m == 2147483648u);  // 2^31 itself is the largest accepted
    m = 777;
    CHECK(!fn::min_d2_of(46341.0, 1.0, 0, &m) && m == 777);           // 46341^2 = 2^31 + 4,633
    // under a cap: min_d2 <= R^2 exactly
    CHECK(fn::min_d2_of(0.3, 0.05, 6, &m) && m == 36);
    m = 777;
    CHECK(!fn::min_d2_of(0.3, 0.05, 5, &m) && m == 777);
    CHECK(fn::min_d2_of(0.25, 0.05, 5, &m) && m == 25);
    CHECK(fn::effective_cap(0) == 0 && fn::effective_cap(1) == 1 && fn::effective_cap(46340) == 46340 &&
          fn::effective_cap(46341) == 0 && fn::effective_cap(std::numeric_limits<std::int64_t>::max()) == 0);
  }

  // the threshold and the mask
  CHECK(fn::has_clearance(25, 25) && !fn::has_clearance(25, 26) && fn::has_clearance(fn::kFar, fn::kFar));
  CHECK(fn::masked(0, 24, 25) == 99 && fn::masked(0, 25, 25) == 0 && fn::masked(-1, 0, 25) == -1 &&
        fn::masked(100, 0, 25) == 100 && fn::masked(0, 0, 0) == 0 && fn::masked(50, 3, 25) == 50);

  // maps at the kernels' boundaries: one strip, several strips, a strip that is not full, widths round 64
  std::uint64_t sum = 0;
  const std::uint32_t shapes[][2] = {{1, 1}, {65, 1}, {1, 65}, {63, 7}, {64, 7}, {65, 5}, {7, 63}, {7, 64}, {7, 65},
                                     {3, 129}, {5, 200}, {40, 40}};
  std::uint64_t seed = 1;
  for (const std::uint32_t * s : shapes)
  {
    for (double density : {0.0, 0.01, 0.05, 0.5, 1.0})
    {
      check_map(s[0], s[1], density, seed++, &sum);
    }
  }
  std::printf("maps checked, sum of d2 %llu\n", static_cast<unsigned long long>(sum));

  // the largest sum: a row of the widest map, the only obstacle 32,767 rows away in the first column
  {
    std::vector<std::uint16_t> g(fn::kMaxSide, fn::kNone);
    g[0] = 32767;
    const std::uint32_t far_corner = fn::row_min(g.data(), fn::kMaxSide, fn::kMaxSide - 1, 0);
    CHECK(far_corner == 2147352578u);
    CHECK(fn::row_min(g.data(), fn::kMaxSide, 0, 0) == 32767u * 32767u);
    CHECK(fn::row_min(g.data(), fn::kMaxSide, fn::kMaxSide - 1, 46340) == 2147352578u);   // 46340^2 = 2147395600
    CHECK(fn::row_min(g.data(), fn::kMaxSide, fn::kMaxSide - 1, 46339) == fn::kFar);
    std::printf("largest d2 %u\n", far_corner);
  }

  if (failures != 0) return 1;
  std::printf("ok\n");
  return 0;
}
