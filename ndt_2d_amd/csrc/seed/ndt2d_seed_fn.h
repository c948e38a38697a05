// The arithmetic of global localisation's seeder (seed/ndt2d_seed.hip): Philox4x32-10, the uniforms
// made from its words, the pick of a free cell, the cell -> pose arithmetic and the rank of a lane in
// the order-preserving compaction -- the contract of include/ndt2d_hip.h ("Global localisation").
// Plain C++ without HIP types, host and device: every thread of the kernels runs it, and a
// stand-alone host program checks it (tests/cpp/seed_fn_check.cpp).  Every operation is written out
// in the order a restatement has to follow (tests/seed_restatement.py); a sum and a product that
// must round separately are separate statements under a contraction-off pragma, whatever the flags
// of the translation unit.
#ifndef NDT2D_SEED_FN_H_
#define NDT2D_SEED_FN_H_

#include <stdint.h>

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
constexpr double kInv53 = 1.1102230246251565e-16;    // 2^-53
constexpr double kInv24 = 5.9604644775390625e-08;    // 2^-24

// Philox4x32-10 (Salmon et al., SC'11): key = seed, counter = {index, step}: the convention of
// ndt2d_pf_noise_launch and ndt2d_resample_uniforms_launch.
NDT2D_SEED_HD inline void philox4x32_10(uint64_t seed, uint64_t index, uint64_t step, uint32_t out[4])
{
  uint32_t c0 = static_cast<uint32_t>(index), c1 = static_cast<uint32_t>(index >> 32);
  uint32_t c2 = static_cast<uint32_t>(step), c3 = static_cast<uint32_t>(step >> 32);
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  for (int r = 0; r < 10; ++r)
  {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t hi0 = static_cast<uint32_t>(p0 >> 32), lo0 = static_cast<uint32_t>(p0);
    const uint32_t hi1 = static_cast<uint32_t>(p1 >> 32), lo1 = static_cast<uint32_t>(p1);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// 53 random bits -> [0, 1) on the 2^-53 grid: 27 bits of `hi` above 26 bits of `lo` (the
// resampler's uniform).  Integer -> double and the product are both exact.
NDT2D_SEED_HD inline double uniform53(uint32_t hi, uint32_t lo)
{
  const uint64_t bits = (static_cast<uint64_t>(hi >> 5) << 26) + static_cast<uint64_t>(lo >> 6);
  return static_cast<double>(bits) * kInv53;
}

// 24 random bits -> (0, 1): ((w >> 8) + 0.5) 2^-24, exact in double; never 0, never 1.
NDT2D_SEED_HD inline double uniform24(uint32_t w)
{
  const double k = static_cast<double>(w >> 8);
  const double half = k + 0.5;   // exact: k < 2^24
  return half * kInv24;          // exact: a power of two
}

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
  philox4x32_10(seed, index, step, a);
  philox4x32_10(seed, index, step + 1, b);
  const uint32_t cell = free_cells[pick(uniform53(a[0], a[1]), n_free)];
  const uint32_t cy = cell / g.width;
  const uint32_t cx = cell - cy * g.width;
  Sample s;
  s.x = coordinate(g.origin_x, cx, uniform24(a[2]), g.resolution);
  s.y = coordinate(g.origin_y, cy, uniform24(a[3]), g.resolution);
  s.theta = heading(uniform24(b[0]));
  s.inject = uniform53(b[1], b[2]);
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

NDT2D_SEED_HD inline uint32_t popcount64(uint64_t v)
{
  v = v - ((v >> 1) & 0x5555555555555555ull);
  v = (v & 0x3333333333333333ull) + ((v >> 2) & 0x3333333333333333ull);
  v = (v + (v >> 4)) & 0x0f0f0f0f0f0f0f0full;
  return static_cast<uint32_t>((v * 0x0101010101010101ull) >> 56);
}

// The free lanes of a 64-lane ballot below `lane`: the lane's rank among its wave's free cells.
NDT2D_SEED_HD inline uint32_t rank_in_wave(uint64_t ballot, uint32_t lane)
{
  return popcount64(ballot & ((1ull << lane) - 1ull));
}

}  // namespace seed
}  // namespace ndt2d

#endif  // NDT2D_SEED_FN_H_
