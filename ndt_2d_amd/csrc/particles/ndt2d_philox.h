// The particle filter's counter-based random words: Philox4x32-10 and the uniforms made from its
// words.  One stream for every unit that draws: ndt2d_pf_noise_launch (ndt2d_motion.hip, which keeps
// its own word -> float conversion), ndt2d_resample_uniforms_launch and the resampler's draws
// (resample/ndt2d_resample.hip), the seeder's samples (seed/ndt2d_seed_fn.h).  Plain C++ without HIP
// types, host and device; tests/cpp/seed_fn_check.cpp checks it against Random123's known answers.
#ifndef NDT2D_PHILOX_H_
#define NDT2D_PHILOX_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_PARTICLES_HD __host__ __device__
#else
#define NDT2D_PARTICLES_HD
#endif

namespace ndt2d
{
namespace particles
{

constexpr double kInv53 = 1.1102230246251565e-16;    // 2^-53
constexpr double kInv24 = 5.9604644775390625e-08;    // 2^-24

// Philox4x32-10 (Salmon et al., SC'11): key = seed, counter = {index, step}.
NDT2D_PARTICLES_HD inline void philox4x32_10(uint64_t seed, uint64_t index, uint64_t step, uint32_t out[4])
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

// 53 random bits -> [0, 1) on the 2^-53 grid: 27 bits of `hi` above 26 bits of `lo`.  Integer ->
// double and the product are both exact.
NDT2D_PARTICLES_HD inline double uniform53(uint32_t hi, uint32_t lo)
{
  const uint64_t bits = (static_cast<uint64_t>(hi >> 5) << 26) + static_cast<uint64_t>(lo >> 6);
  return static_cast<double>(bits) * kInv53;
}

// 24 random bits -> (0, 1): ((w >> 8) + 0.5) 2^-24, exact in double; never 0, never 1.
NDT2D_PARTICLES_HD inline double uniform24(uint32_t w)
{
  const double k = static_cast<double>(w >> 8);
  const double half = k + 0.5;   // exact: k < 2^24
  return half * kInv24;          // exact: a power of two
}

}  // namespace particles
}  // namespace ndt2d

#endif  // NDT2D_PHILOX_H_
