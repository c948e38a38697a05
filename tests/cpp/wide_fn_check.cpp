// Stand-alone check of csrc/wide/ndt2d_wide_fn.h (built and run by tests/test_wide_restatement.py,
// plainly and with -fsanitize=address,undefined): the box maximum against long double dense
// sampling of random rectangles -- definite, indefinite, zero and non-finite records; the mean
// inside the rectangle, on an edge and outside it -- and the pixels of a small grid, printed for the
// numpy restatement to compare.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "ndt2d_wide_fn.h"

namespace w = ndt2d::wide;

static int failures = 0;
#define CHECK(cond)                                                   \
  do                                                                  \
  {                                                                   \
    if (!(cond))                                                      \
    {                                                                 \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// a small generator of its own: the same numbers with every compiler
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform()
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return static_cast<double>(rng_state >> 11) * 0x1.0p-53;
}
static double between(double lo, double hi) { return lo + (hi - lo) * uniform(); }

struct Record
{
  double mx, my, h00, h01, h11;
};

static long double exponent_ld(const Record & r, long double px, long double py)
{
  const long double q0 = px - r.mx, q1 = py - r.my;
  return r.h00 * q0 * q0 + 2.0L * r.h01 * q0 * q1 + r.h11 * q1 * q1;
}

// the largest exponent over a 65 x 65 sample of the rectangle, its edges and corners included
static long double sampled_max(const Record & r, double x0, double x1, double y0, double y1)
{
  const int n = 64;
  long double best = -std::numeric_limits<long double>::infinity();
  for (int a = 0; a <= n; ++a)
  {
    const long double px = a == n ? static_cast<long double>(x1) : x0 + (static_cast<long double>(x1) - x0) * a / n;
    for (int b = 0; b <= n; ++b)
    {
      const long double py = b == n ? static_cast<long double>(y1) : y0 + (static_cast<long double>(y1) - y0) * b / n;
      const long double e = exponent_ld(r, px, py);
      if (e > best) best = e;
    }
  }
  return best;
}

// the true maximum of a NEGATIVE DEFINITE record's exponent over the rectangle, in long double
static long double definite_max(const Record & r, double x0, double x1, double y0, double y1)
{
  if (r.mx >= x0 && r.mx <= x1 && r.my >= y0 && r.my <= y1) return 0.0L;
  long double best = -std::numeric_limits<long double>::infinity();
  const double ys[2] = {y0, y1}, xs[2] = {x0, x1};
  for (double yc : ys)
  {
    long double px = r.mx - static_cast<long double>(r.h01) * (static_cast<long double>(yc) - r.my) / r.h00;
    px = px < x0 ? x0 : (px > x1 ? x1 : px);
    const long double e = exponent_ld(r, px, yc);
    if (e > best) best = e;
  }
  for (double xc : xs)
  {
    long double py = r.my - static_cast<long double>(r.h01) * (static_cast<long double>(xc) - r.mx) / r.h11;
    py = py < y0 ? y0 : (py > y1 ? y1 : py);
    const long double e = exponent_ld(r, xc, py);
    if (e > best) best = e;
  }
  return best;
}

enum Kind { kDefinite, kIndefinite, kSemidefinite, kPositive };

static Record make_record(Kind kind, double mx, double my)
{
  // h = R diag(a, b) R^T with a rotation of a random angle
  const double t = between(-3.2, 3.2), c = std::cos(t), s = std::sin(t);
  double a = -between(0.5, 100.0), b = -between(0.5, 100.0);
  if (kind == kIndefinite) b = -b;
  if (kind == kSemidefinite) b = 0.0;
  if (kind == kPositive)
  {
    a = -a;
    b = -b;
  }
  return Record{mx, my, a * c * c + b * s * s, (a - b) * c * s, a * s * s + b * c * c};
}

int main()
{
  const double slack = 0x1.0p-41;   // below log(1 + 2^-40): what the inflation of a pixel's value covers
  long double worst_excess = 0.0L, worst_value_excess = 0.0L, least_margin = 1.0L;
  int n_inside = 0, n_edge = 0, n_outside = 0;
  for (int trial = 0; trial < 6000; ++trial)
  {
    const double x0 = between(-1.0, 1.0), y0 = between(-1.0, 1.0);
    const double x1 = x0 + between(0.0, 0.6), y1 = y0 + between(0.0, 0.6);
    // the mean: inside, on an edge (exactly), outside
    double mx, my;
    const int where = trial % 3;
    if (where == 0)
    {
      mx = between(x0, x1);
      my = between(y0, y1);
      if (!(mx >= x0 && mx <= x1 && my >= y0 && my <= y1)) continue;
      ++n_inside;
    }
    else if (where == 1)
    {
      const int edge = (trial / 3) % 4;
      mx = edge == 0 ? x0 : (edge == 1 ? x1 : between(x0, x1));
      my = edge == 2 ? y0 : (edge == 3 ? y1 : between(y0, y1));
      if (!(mx >= x0 && mx <= x1 && my >= y0 && my <= y1)) continue;
      ++n_edge;
    }
    else
    {
      mx = uniform() < 0.5 ? x0 - between(0.01, 0.8) : (uniform() < 0.5 ? x1 + between(0.01, 0.8) : between(x0, x1));
      my = between(y0 - 0.8, y1 + 0.8);
      if (mx >= x0 && mx <= x1 && my >= y0 && my <= y1) continue;
      ++n_outside;
    }
    const Kind kind = static_cast<Kind>((trial / 12) % 4);
    const Record r = make_record(kind, mx, my);
    CHECK(w::record_finite(r.mx, r.my, r.h00, r.h01, r.h11));
    const double got = w::box_max_exponent(r.mx, r.my, r.h00, r.h01, r.h11, x0, x1, y0, y1);
    const long double sampled = sampled_max(r, x0, x1, y0, y1);
    // never below a sampled value (beyond what the inflation covers)
    CHECK(static_cast<long double>(got) + slack >= sampled);
    if (static_cast<long double>(got) + slack - sampled < least_margin) least_margin = static_cast<long double>(got) + slack - sampled;
    // ... and a point of the rectangle's own: never above the exponent's range over it
    if (kind == kDefinite)
    {
      const long double truth = definite_max(r, x0, x1, y0, y1);
      CHECK(sampled <= truth + 1e-15L);
      const long double excess = static_cast<long double>(got) - truth;
      CHECK(excess <= 1e-12L && excess >= -1e-12L);   // rounding only
      if (excess > worst_excess) worst_excess = excess;
      const long double value_excess = static_cast<long double>(std::exp(got) * w::kInflate) / expl(truth) - 1.0L;
      CHECK(value_excess >= 0.0L && value_excess <= 0x1.0p-40L + 1e-12L);
      if (value_excess > worst_value_excess) worst_value_excess = value_excess;
      if (mx >= x0 && mx <= x1 && my >= y0 && my <= y1) CHECK(got == 0.0);
    }
  }
  CHECK(n_inside > 1000 && n_edge > 1000 && n_outside > 500);
  std::printf("excess of the exponent over the true maximum, definite records: %.3Le at most\n", worst_excess);
  std::printf("excess of the inflated value over the true maximum's: %.3Le at most (2^-40 = %.3e)\n", worst_value_excess, 0x1.0p-40);
  std::printf("excess margin over the samples, all records: %.3Le at least\n", least_margin);

  // the zero record: every point scores exp(0)
  CHECK(w::box_max_exponent(0.3, 0.2, 0.0, 0.0, 0.0, -1.0, 1.0, -1.0, 1.0) == 0.0);
  CHECK(w::box_max_exponent(5.0, 5.0, 0.0, 0.0, 0.0, -1.0, 1.0, -1.0, 1.0) == 0.0);
  // a degenerate rectangle: one point
  CHECK(w::box_max_exponent(0.0, 0.0, -2.0, 0.0, -3.0, 1.0, 1.0, 1.0, 1.0) == -5.0);
  // non-finite records are told apart, whichever entry it is
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int k = 0; k < 5; ++k)
  {
    for (double bad : {nan, inf, -inf})
    {
      double v[5] = {0.1, 0.2, -3.0, 0.5, -4.0};
      v[k] = bad;
      CHECK(!w::record_finite(v[0], v[1], v[2], v[3], v[4]));
    }
  }
  // products that overflow against each other count as +inf, never as nothing
  CHECK(w::box_max_exponent(0.0, 0.0, 1e308, -1e308, 1e308, 1.0, 2.0, 1.0, 2.0) == inf);

  // geometry
  CHECK(w::pitch_of(0.07, 0.25, 2) == 0.07 / 2.0 && w::pitch_of(0.01, 0.25, 1) == 0.0625);
  CHECK(w::box_cells_along(0.07, 0.035, 0.25) == 2.0 && w::box_cells_along(1.4, 0.7, 0.25) == 10.0);
  CHECK(w::tile_bound(1.0, 100) > 1.0 && w::tile_bound(0.0, 100) == 0.0);

  // a grid of 3 x 2 cells of 0.25 m at (-0.3, 0.1): a definite cell, an indefinite one, a cell with
  // n = 4, a cell with a NaN mean, a zero record and a cell with a clamped-eigenvalue record
  const double cells6[6][6] = {{-0.21, 0.19, 310.0, -45.0, 120.0, 9.0},   {0.07, 0.22, 80.0, 130.0, -60.0, 7.0},
                               {0.33, 0.3, 200.0, 0.0, 200.0, 4.0},       {nan, 0.45, 100.0, 0.0, 100.0, 12.0},
                               {0.1, 0.5, 0.0, 0.0, 0.0, 5.0},            {0.36, 0.52, 4.0e7, 1.2e7, 3.64e6, 30.0}};
  std::vector<double> cells(7 * 8, 0.0);
  uint32_t occ = 0;
  for (int c = 0; c < 6; ++c)
  {
    std::printf("C %a %a %a %a %a %a\n", cells6[c][0], cells6[c][1], cells6[c][2], cells6[c][3], cells6[c][4], cells6[c][5]);
    cells[8 * c + 0] = cells6[c][0];
    cells[8 * c + 1] = cells6[c][1];
    for (int k = 0; k < 3; ++k) cells[8 * c + 2 + k] = -0.5 * cells6[c][2 + k];
    if (cells6[c][5] >= 5.0) occ |= 1u << c;
  }
  const w::GridRef g{cells.data(), &occ, 8, 3, 2, 0.25, -0.3, 0.1};
  w::Image im{};
  im.window = 0.07;
  im.pitch = w::pitch_of(im.window, g.cell_size, 2);
  im.inv_pitch = 1.0 / im.pitch;
  im.origin_x = g.origin_x - (im.window + im.pitch);
  im.origin_y = g.origin_y - (im.window + im.pitch);
  im.nx = static_cast<uint32_t>(w::pixels_along(g.size_x, g.cell_size, im.window, im.pitch));
  im.ny = static_cast<uint32_t>(w::pixels_along(g.size_y, g.cell_size, im.window, im.pitch));
  int n_zero = 0, n_one = 0;
  for (uint32_t j = 0; j < im.ny; ++j)
  {
    for (uint32_t i = 0; i < im.nx; ++i)
    {
      const double v = w::pixel_value(g, im, i, j);
      CHECK(v >= w::pixel_value_raw(g, im, i, j) && v >= 0.0);
      n_zero += v == 0.0;
      n_one += v == w::kInflate;
      std::printf("P %u %u %a\n", i, j, v);
      // the point of the pixel's own lower corner finds the pixel
      uint32_t pi, pj;
      CHECK(w::pixel_of(im, im.origin_x + (i + 0.5) * im.pitch, im.origin_y + (j + 0.5) * im.pitch, pi, pj) && pi == i && pj == j);
    }
  }
  CHECK(n_zero > 0 && n_one > 0);
  uint32_t pi, pj;
  CHECK(!w::pixel_of(im, nan, 0.2, pi, pj) && !w::pixel_of(im, 0.0, inf, pi, pj) && !w::pixel_of(im, -5.0, 0.2, pi, pj));
  CHECK(!w::pixel_of(im, im.origin_x + im.nx * im.pitch + 1e-6, 0.2, pi, pj));

  if (failures != 0)
  {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
