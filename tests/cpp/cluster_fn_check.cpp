// Stand-alone check of ndt_2d_amd/csrc/cluster/ndt2d_cluster_fn.h: the keys at the bin edges on both
// sides of 0, the heading at -pi, pi, 3 pi and the last double below pi, every left-out reason, q at
// 0, 2^-41, 2^-40 and 1, the neighbour list (26 entries, the heading's wrap, n_theta of 1 and 2) and
// the rank order.  Built with the host compiler (once more with -fsanitize=address,undefined) and
// run directly; no device, no library.  Prints one line per designed sample
//   "K <x hex> <y hex> <theta hex> <w hex> <cell_x hex> <cell_y hex> <n_theta> <kx> <ky> <kt> <q> <hash>"
//   "A <theta hex> <normalised hex>"
//   "N <kx> <ky> <kt> <n_theta> <26 x (kx ky kt)>"
// for tests/test_cluster_restatement.py to compare with the restatement bit for bit; exits non-zero
// when a check fails.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <tuple>

#include "ndt2d_cluster_fn.h"

namespace F = ndt2d::cluster;

namespace
{

int failures = 0;

void check(bool ok, const char * what)
{
  if (!ok)
  {
    if (failures < 20) std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

struct SplitMix64
{
  uint64_t s;
  uint64_t next()
  {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double unit() { return static_cast<double>(next() >> 11) * 1.1102230246251565e-16; }
};

F::Key sample(double x, double y, double theta, double w, const F::Bins & b)
{
  const F::Key k = F::key_of(x, y, theta, w, b);
  const uint64_t q = k.kt >= 0 ? F::mass_q(w) : 0;
  std::printf("K %a %a %a %a %a %a %d %d %d %d %" PRIu64 " %" PRIu32 "\n", x, y, theta, w, b.cell_x, b.cell_y,
              b.n_theta, k.kx, k.ky, k.kt, q, F::key_hash(k));
  return k;
}

double angle(double theta)
{
  const double t = F::normalise_angle(theta);
  std::printf("A %a %a\n", theta, t);
  check(t >= -F::kPi && t < F::kPi, "a normalised heading lies in [-pi, pi)");
  return t;
}

void neighbour_list(const F::Key & k, int32_t n_theta)
{
  std::printf("N %d %d %d %d", k.kx, k.ky, k.kt, n_theta);
  std::set<std::tuple<int32_t, int32_t, int32_t>> seen;
  for (int j = 0; j < F::kNeighbours; ++j)
  {
    const F::Key o = F::neighbour(k, j, n_theta);
    std::printf(" %d %d %d", o.kx, o.ky, o.kt);
    check(o.kt >= 0 && o.kt < n_theta, "a neighbour's heading bin lies in 0 .. n_theta - 1");
    check(std::abs(o.kx - k.kx) <= 1 && std::abs(o.ky - k.ky) <= 1, "a neighbour is one bin away at most");
    seen.insert(std::make_tuple(o.kx, o.ky, o.kt));
  }
  std::printf("\n");
  const bool has_self = seen.count(std::make_tuple(k.kx, k.ky, k.kt)) != 0;
  if (n_theta >= 3)
  {
    check(seen.size() == 26 && !has_self, "26 distinct neighbours, the key itself not among them");
  }
  else if (n_theta == 2)
  {
    check(seen.size() == 17 && !has_self, "n_theta 2: 8 in the plane and the twin's 9");
  }
  else
  {
    check(seen.size() == 9 && has_self, "n_theta 1: the plane's 8 and the key itself");
  }
}

}  // namespace

int main()
{
  const F::Bins def{0.5, 0.5, 24};
  const double below_pi = std::nextafter(F::kPi, 0.0);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

  // the bin edges on both sides of 0: floor, so -0.25 and +0.25 are keys -1 and 0
  check(sample(-0.25, 0.25, 0.0, 0.5, def).kx == -1, "x = -0.25 is bin -1");
  check(sample(0.25, -0.25, 0.0, 0.5, def).kx == 0, "x = +0.25 is bin 0");
  check(sample(0.0, -0.0, 0.0, 0.5, def).kx == 0, "x = 0 is bin 0");
  check(sample(-0.0, 0.0, 0.0, 0.5, def).ky == 0, "y = 0 is bin 0");
  check(sample(std::nextafter(0.0, -1.0), 0.5, 0.0, 0.5, def).kx == -1, "the last double below 0 is bin -1");
  check(sample(0.5, std::nextafter(0.5, 0.0), 0.0, 0.5, def).kx == 1, "x = 0.5 is bin 1");
  check(sample(std::nextafter(0.5, 0.0), 0.5, 0.0, 0.5, def).kx == 0, "the last double below 0.5 is bin 0");
  check(sample(-0.5, std::nextafter(-0.5, -1.0), 0.0, 0.5, def).kx == -1, "x = -0.5 is bin -1");
  check(sample(std::nextafter(-0.5, -1.0), -0.5, 0.0, 0.5, def).kx == -2, "the first double below -0.5 is bin -2");
  for (const double cell : {0.1, 0.25, 0.3, 1.0, 7.5})
  {
    const F::Bins b{cell, 2.0 * cell, 24};
    for (const int e : {-3, -1, 0, 1, 2, 1000})
    {
      const double edge = e * cell;
      sample(edge, edge, 0.1, 0.25, b);
      sample(std::nextafter(edge, -1e9), std::nextafter(edge, 1e9), 0.1, 0.25, b);
    }
  }

  // the heading
  check(angle(-F::kPi) == -F::kPi, "-pi stays");
  check(angle(F::kPi) == -F::kPi, "pi goes to -pi");
  angle(3.0 * F::kPi);
  check(angle(below_pi) == below_pi, "the last double below pi stays");
  angle(-3.0 * F::kPi);
  angle(std::nextafter(-F::kPi, -4.0));
  angle(F::kTwoPi);
  angle(-F::kTwoPi);
  angle(1e9);
  angle(-1e300);
  angle(0.0);
  for (const int32_t n_theta : {1, 2, 3, 24, 360})
  {
    const F::Bins b{0.5, 0.5, n_theta};
    check(sample(0.1, 0.1, -F::kPi, 0.5, b).kt == 0, "-pi is heading bin 0");
    check(sample(0.1, 0.1, F::kPi, 0.5, b).kt == 0, "pi is heading bin 0");
    check(sample(0.1, 0.1, below_pi, 0.5, b).kt == n_theta - 1, "the last double below pi is the last heading bin");
    sample(0.1, 0.1, 3.0 * F::kPi, 0.5, b);
    sample(0.1, 0.1, 0.0, 0.5, b);
    sample(0.1, 0.1, std::nextafter(0.0, -1.0), 0.5, b);
  }
  SplitMix64 rng{11};
  for (int i = 0; i < 40; ++i)
  {
    const F::Bins b{0.05 + rng.unit(), 0.05 + rng.unit(), 1 + static_cast<int32_t>(rng.next() % 40)};
    const F::Key k = sample(200.0 * rng.unit() - 100.0, 200.0 * rng.unit() - 100.0, 40.0 * rng.unit() - 20.0, rng.unit(), b);
    check(k.kt >= 0 && k.kt < b.n_theta, "a random heading bin lies in 0 .. n_theta - 1");
  }

  // every left-out reason
  check(sample(nan, 0.0, 0.0, 0.5, def).kt < 0, "x NaN is left out");
  check(sample(0.0, inf, 0.0, 0.5, def).kt < 0, "y infinite is left out");
  check(sample(0.0, 0.0, -inf, 0.5, def).kt < 0, "theta infinite is left out");
  check(sample(0.0, 0.0, nan, 0.5, def).kt < 0, "theta NaN is left out");
  check(sample(0.5 * F::kKeyLimit, 0.0, 0.0, 0.5, def).kt < 0, "x / cell = 2^30 is left out");
  check(sample(0.0, -0.5 * F::kKeyLimit, 0.0, 0.5, def).kt < 0, "y / cell = -2^30 is left out");
  check(sample(std::nextafter(0.5 * F::kKeyLimit, 0.0), 0.0, 0.0, 0.5, def).kx == (1 << 30) - 1, "the last x below the limit is kept");
  check(sample(std::nextafter(-0.5 * F::kKeyLimit, 0.0), 0.0, 0.0, 0.5, def).kx == -(1 << 30), "the first x above the negative limit is kept");
  check(sample(1e300, 0.0, 0.0, 0.5, F::Bins{1e-300, 0.5, 24}).kt < 0, "a quotient that overflows is left out");
  check(sample(0.0, 0.0, 0.0, nan, def).kt < 0, "a NaN weight is left out");
  check(sample(0.0, 0.0, 0.0, -1e-300, def).kt < 0, "a negative weight is left out");
  check(sample(0.0, 0.0, 0.0, std::nextafter(1.0, 2.0), def).kt < 0, "a weight above 1 is left out");
  check(sample(0.0, 0.0, 0.0, inf, def).kt < 0, "an infinite weight is left out");
  check(sample(0.0, 0.0, 0.0, -0.0, def).kt >= 0, "a weight of -0 counts");

  // q
  check(F::mass_q(0.0) == 0, "q(0) = 0");
  check(F::mass_q(std::ldexp(1.0, -41)) == 0, "q(2^-41) = 0");
  check(F::mass_q(std::ldexp(1.0, -40)) == 1, "q(2^-40) = 1");
  check(F::mass_q(std::nextafter(std::ldexp(1.0, -40), 0.0)) == 0, "q below 2^-40 = 0");
  check(F::mass_q(1.0) == (1ull << 40), "q(1) = 2^40");
  check(F::mass_q(0.6) == 659706976665ull, "q(0.6) = trunc(0.6 2^40)");
  for (const double w : {0.0, std::ldexp(1.0, -41), std::ldexp(1.0, -40), 1.0, 0.6, 0.4, 1.0 / 3.0, 1e-5})
  {
    sample(0.3, 0.3, 0.3, w, def);
  }

  // the neighbours
  neighbour_list(F::Key{0, 0, 0}, 24);
  neighbour_list(F::Key{-1, 5, 23}, 24);
  neighbour_list(F::Key{(1 << 30) - 1, -(1 << 30), 1}, 3);
  neighbour_list(F::Key{2, -3, 0}, 3);
  neighbour_list(F::Key{2, -3, 0}, 2);
  neighbour_list(F::Key{2, -3, 1}, 2);
  neighbour_list(F::Key{2, -3, 0}, 1);
  {
    // the wrap: bin 0's heading neighbours are n_theta - 1 and 1
    std::set<int32_t> kts;
    for (int j = 0; j < F::kNeighbours; ++j) kts.insert(F::neighbour(F::Key{0, 0, 0}, j, 24).kt);
    check(kts == std::set<int32_t>({23, 0, 1}), "heading bin 0 wraps to n_theta - 1");
    kts.clear();
    for (int j = 0; j < F::kNeighbours; ++j) kts.insert(F::neighbour(F::Key{0, 0, 23}, j, 24).kt);
    check(kts == std::set<int32_t>({22, 23, 0}), "heading bin n_theta - 1 wraps to 0");
  }

  // the rank order: Q descending, then label ascending; total and strict
  check(F::ranks_before(5, 9, 4, 1), "the heavier cluster is first");
  check(!F::ranks_before(4, 1, 5, 9), "the lighter cluster is not");
  check(F::ranks_before(5, 1, 5, 9), "equal Q: the lower label is first");
  check(!F::ranks_before(5, 9, 5, 1), "equal Q: the higher label is not");
  check(!F::ranks_before(5, 9, 5, 9), "a cluster is not before itself");
  check(F::ranks_before(0, 3, 0, 0xffffffffu), "any cluster is before the empty entry");
  check(F::ranks_before(1ull << 63, 7, (1ull << 63) - 1, 0), "Q is compared as 64 bits");

  check(F::table_size(0) == 64 && F::table_size(32) == 64 && F::table_size(33) == 128 && F::table_size(1000000) == 2097152,
        "the table is a power of two, at least 64 and at least 2 n");

  if (failures != 0)
  {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
