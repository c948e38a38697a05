// Stand-alone check of ndt_2d_amd/csrc/seed/ndt2d_seed_fn.h and of particles/ndt2d_philox.h under
// it: Philox against Random123's known answers, the uniforms and the pick of a free cell against
// integer arithmetic (the double product of the pick restated as a round-to-nearest-even of a
// 128-bit integer), the cell -> pose arithmetic against long double and the occupancy grid's own
// cell rule.  (The table's compaction: tests/cpp/compact_fn_check.cpp.)  Built with the host
// compiler (once more with -fsanitize=address,undefined) and run directly; no device, no library.
// Prints one line per designed sample
// ("P <seed> <step> <index> <x hex> <y hex> <theta hex> <inject hex>") for
// tests/test_seed_restatement.py to compare with the restatement bit for bit; exits non-zero when a
// check fails.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ndt2d_seed_fn.h"

namespace P = ndt2d::particles;
namespace S = ndt2d::seed;

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
};

int bit_length(unsigned __int128 v)
{
  int n = 0;
  while (v != 0)
  {
    ++n;
    v >>= 1;
  }
  return n;
}

// trunc(fl(bits * 2^-53 * n_free)) in integers: the exact product rounded to 53 significant bits,
// ties to even, then shifted down
uint64_t pick_in_integers(uint64_t bits, uint64_t n_free)
{
  unsigned __int128 p = static_cast<unsigned __int128>(bits) * n_free;
  const int len = bit_length(p);
  if (len > 53)
  {
    const int sh = len - 53;
    const unsigned __int128 one = 1;
    const unsigned __int128 rem = p & ((one << sh) - 1), half = one << (sh - 1);
    unsigned __int128 q = p >> sh;
    if (rem > half || (rem == half && (q & 1) != 0)) ++q;
    p = q << sh;
  }
  const uint64_t k = static_cast<uint64_t>(p >> 53);
  return k < n_free - 1 ? k : n_free - 1;
}

}  // namespace

int main()
{
  // ---- Philox4x32-10: Random123's kat_vectors as (seed, index, step) ----
  {
    struct Kat
    {
      uint64_t seed, index, step;
      uint32_t out[4];
    };
    const Kat kat[] = {{0, 0, 0, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
                       {~0ull, ~0ull, ~0ull, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
                       {0x299f31d0a4093822ull, 0x85a308d3243f6a88ull, 0x0370734413198a2eull,
                        {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}}};
    for (const Kat & k : kat)
    {
      uint32_t w[4];
      P::philox4x32_10(k.seed, k.index, k.step, w);
      check(w[0] == k.out[0] && w[1] == k.out[1] && w[2] == k.out[2] && w[3] == k.out[3], "philox: known answer");
    }
  }

  // ---- the uniforms: designed words at both ends, random words, against integers ----
  SplitMix64 rng{2024};
  check(P::uniform53(0u, 0u) == 0.0, "uniform53: all-zero words");
  check(P::uniform53(31u, 63u) == 0.0, "uniform53: the dropped low bits");
  check(P::uniform53(~0u, ~0u) == 1.0 - std::ldexp(1.0, -53) && P::uniform53(~0u, ~0u) < 1.0, "uniform53: all-one words");
  check(P::uniform24(0u) == std::ldexp(1.0, -25) && P::uniform24(255u) == std::ldexp(1.0, -25), "uniform24: the smallest value");
  check(P::uniform24(~0u) == 1.0 - std::ldexp(1.0, -25) && P::uniform24(~0u) < 1.0, "uniform24: the largest value");
  for (int it = 0; it < 200000; ++it)
  {
    const uint32_t a = static_cast<uint32_t>(rng.next()), b = static_cast<uint32_t>(rng.next());
    const uint64_t bits = (static_cast<uint64_t>(a >> 5) << 26) + (b >> 6);
    const double u = P::uniform53(a, b);
    check(u >= 0.0 && u < 1.0 && static_cast<uint64_t>(std::ldexp(u, 53)) == bits && std::ldexp(u, 53) == std::floor(std::ldexp(u, 53)),
          "uniform53: the 53 bits");
    const double v = P::uniform24(a);
    check(v > 0.0 && v < 1.0 && static_cast<long>(std::ldexp(v, 25)) == 2 * static_cast<long>(a >> 8) + 1, "uniform24: (2 k + 1) 2^-25");
  }

  // ---- the pick ----
  {
    const uint64_t sizes[] = {1, 2, 3, 5, 63, 64, 65, 1000, 90000, 641601, (1ull << 30) - 1, 1ull << 30, (1ull << 31) - 1};
    for (uint64_t f : sizes)
    {
      check(S::pick(0.0, f) == 0, "pick: u = 0");
      check(S::pick(P::uniform53(~0u, ~0u), f) == f - 1, "pick: all-one words take the last cell");
      check(S::pick(1.0, f) == f - 1, "pick: the clamp to F - 1");
      check(S::pick(P::uniform53(~0u, ~0u), f) == pick_in_integers((1ull << 53) - 1, f), "pick: all-one words in integers");
      for (int it = 0; it < 20000; ++it)
      {
        const uint32_t a = static_cast<uint32_t>(rng.next()), b = static_cast<uint32_t>(rng.next());
        const uint64_t bits = (static_cast<uint64_t>(a >> 5) << 26) + (b >> 6);
        const uint64_t k = S::pick(P::uniform53(a, b), f);
        check(k < f && k == pick_in_integers(bits, f), "pick: against integers");
      }
      // products next to an integer: bits = ceil(j 2^53 / f) and its neighbour below
      for (uint64_t j = 1; j < f && j < 2000; ++j)
      {
        const unsigned __int128 num = (static_cast<unsigned __int128>(j) << 53) + f - 1;
        const uint64_t bits = static_cast<uint64_t>(num / f);
        for (uint64_t bb : {bits - 1, bits})
        {
          if (bb >= (1ull << 53)) continue;
          const double u = static_cast<double>(bb) * P::kInv53;
          check(S::pick(u, f) == pick_in_integers(bb, f), "pick: next to an integer");
        }
      }
    }
  }

  // ---- cell -> pose ----
  {
    struct Geo
    {
      double origin, resolution;
    };
    const Geo geos[] = {{0.0, 1.0}, {-3.35, 0.05}, {-10.25, 0.05}, {1.7, 0.1}, {-47.5, 0.25}, {-0.3, 0.3}, {12.345, 0.025}};
    const uint32_t cells[] = {0, 1, 2, 62, 63, 64, 255, 256, 300, 800, 4095, 46339};
    const uint32_t designed[] = {0u, 255u, 256u, 0x7fffffffu, 0x80000000u, 0xffffff00u, ~0u};
    for (const Geo & g : geos)
    {
      for (uint32_t c : cells)
      {
        for (int it = 0; it < 2000; ++it)
        {
          const uint32_t w = it < 7 ? designed[it] : static_cast<uint32_t>(rng.next());
          const double u = P::uniform24(w);
          const double p = S::coordinate(g.origin, c, u, g.resolution);
          const long double exact = static_cast<long double>(g.origin) +
                                    (static_cast<long double>(c) + static_cast<long double>(u)) * static_cast<long double>(g.resolution);
          const double scale = std::fmax(std::fabs(g.origin), std::fabs(p));
          check(std::fabs(static_cast<double>(static_cast<long double>(p) - exact)) <= 2.0 * scale * 2.3e-16 + 1e-300,
                "coordinate: within two roundings of the exact value");
          // the occupancy grid's own rule puts the pose back into its cell
          check(static_cast<long>((p - g.origin) / g.resolution) == static_cast<long>(c), "coordinate: falls back into its cell");
        }
      }
    }
    check(S::heading(P::uniform24(0u)) > -S::kPi && S::heading(P::uniform24(~0u)) < S::kPi, "heading: in (-pi, pi)");
    check(S::heading(0.5) == 0.0, "heading: the middle");
    double last = -4.0;
    for (uint32_t k = 0; k < (1u << 24); k += 4099)
    {
      const double t = S::heading(P::uniform24(k << 8));
      check(t > last && t >= -S::kPi && t < S::kPi, "heading: monotone, in range");
      last = t;
    }
  }

  // ---- whole samples on a designed map, printed for the restatement ----
  {
    const uint32_t W = 37, H = 23;
    std::vector<uint32_t> table;
    for (uint32_t y = 0; y < H; ++y)
    {
      for (uint32_t x = 0; x < W; ++x)
      {
        if ((x * 7 + y * 13) % 5 != 0) table.push_back(y * W + x);
      }
    }
    const S::Geometry g{-3.35, 1.7, 0.05, W};
    struct Case
    {
      uint64_t seed, step, index;
    };
    std::vector<Case> todo = {{0, 0, 0}, {~0ull, ~0ull, ~0ull}, {0x299f31d0a4093822ull, 0x0370734413198a2eull, 0x85a308d3243f6a88ull},
                              {1, 1, 0}, {1, 1, 1}, {7, 2, (1ull << 32) - 1}, {7, 2, 1ull << 32}, {7, ~0ull, 5}};
    for (uint64_t i = 0; i < 24; ++i) todo.push_back(Case{rng.next(), rng.next(), rng.next()});
    for (const Case & c : todo)
    {
      const S::Sample s = S::sample(c.seed, c.step, c.index, table.data(), table.size(), g);
      uint32_t a[4], b[4];
      P::philox4x32_10(c.seed, c.index, c.step, a);
      P::philox4x32_10(c.seed, c.index, c.step + 1, b);
      const uint32_t cell = table[S::pick(P::uniform53(a[0], a[1]), table.size())];
      check(s.x == S::coordinate(g.origin_x, cell % W, P::uniform24(a[2]), g.resolution) &&
              s.y == S::coordinate(g.origin_y, cell / W, P::uniform24(a[3]), g.resolution) &&
              s.theta == S::heading(P::uniform24(b[0])) && s.inject == P::uniform53(b[1], b[2]),
            "sample: the composition of its parts");
      check(static_cast<long>((s.x - g.origin_x) / g.resolution) == static_cast<long>(cell % W) &&
              static_cast<long>((s.y - g.origin_y) / g.resolution) == static_cast<long>(cell / W),
            "sample: in its cell");
      std::printf("P %" PRIu64 " %" PRIu64 " %" PRIu64 " %a %a %a %a\n", c.seed, c.step, c.index, s.x, s.y, s.theta, s.inject);
    }
  }

  if (failures != 0)
  {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
