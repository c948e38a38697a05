// Which patch columns and rows of a lattice can hold a lane "near" a cell boundary for one beam
// (ndt2d_lane_fn.h: kNearUnits, near_boundary()): the 64-bit word the large search's table
// pre-kernel leaves beside every beam's K.  Plain integer C++, no HIP header: the pre-kernel
// and the host check (tests/cpp/near_bits_check.cpp) compile the same lines.
//
// The search adds K (per beam) and D (per lane) as ONE integer in an f64 mantissa,
//   K = 2^52 + ky * 2^24 + kx (+ kNearBias),   D = dy * 2^24 + dx,   dx, dy signed,
// and a lane is near when a 16-bit fraction of the sum, biased by kNearUnits, is below
// 2 * kNearUnits: bits 0..15 on x, bits 24..39 on y.  The x fraction of the sum is that of
// kx + dx.  The y fraction is that of ky + dy PLUS the carry (or borrow) out of the 24-bit x
// field, floor((kx + dx) / 2^24), so a row's bit looks at every carry the lattice's x offsets
// can produce -- the sum is not two independent axes.
#ifndef NDT2D_NEAR_BITS_H_
#define NDT2D_NEAR_BITS_H_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NDT2D_NEAR_HD __host__ __device__
#else
#define NDT2D_NEAR_HD
#endif

namespace ndt2d
{

constexpr uint32_t kNearUnits = 4;     // guard band around cell boundaries, in 2^-16 cells
constexpr uint32_t kNearPatch = 8;     // lattice steps per patch column / row (kPatch)
constexpr uint32_t kNearColumns = 32;  // bits per axis: lattices of up to 256 steps
constexpr uint64_t kNearAll = ~0ull;   // "every lane may be near": the per-lane test decides

// A lattice offset in fixed-point units, as the lanes round it (packed_offset()).
NDT2D_NEAR_HD inline double near_offset_units(double d, double inv_scaled) { return rint(d * inv_scaled); }

// Carry of kx + d out of the 24-bit x field: floor((kx + d) / 2^24), d of either sign.
NDT2D_NEAR_HD inline int32_t near_x_carry(uint32_t kx24, int32_t d)
{
  return static_cast<int32_t>((static_cast<int64_t>(kx24) + d + (int64_t{1} << 32)) >> 24) - 256;
}

// Does fraction + f[i], modulo 2^16, fall below 2 * kNearUnits for one of the kNearPatch
// 16-bit offset fractions f[]?  (The least of the sums is below it or none is.)
template <typename Fractions>
NDT2D_NEAR_HD inline bool near_possible(uint32_t fraction, Fractions f)
{
  uint32_t least = 0xffffu;
  for (uint32_t i = 0; i < kNearPatch; ++i)
  {
    const uint32_t s = (fraction + f[i]) & 0xffffu;
    least = s < least ? s : least;
  }
  return least < 2u * kNearUnits;
}

// near_bits(t, b): bit px -- some lattice step ix of patch column px, [8 px, 8 px + 7] clipped to
// n_lin, puts a lane within the guard band on x for the beam whose K has the low 48 mantissa bits
// k48; bit 32 + py -- the same for row py on y, for some x step of the lattice.
//   fractions[i] = offset_i & 0xffff for i < n_lin, offset_i = near_offset_units(dlin[i], inv_scaled)
//                  as an integer, the last one repeated up to a multiple of kNearPatch (the
//                  shadow lanes of an edge patch repeat the last candidate);
//   d_min, d_max = the least and the greatest offset_i.
// More than kNearColumns columns: every bit set.
template <typename Fractions>
NDT2D_NEAR_HD inline uint64_t near_bits(uint64_t k48, Fractions fractions, uint32_t n_lin, int32_t d_min,
                                        int32_t d_max)
{
  if (n_lin > kNearPatch * kNearColumns) return kNearAll;
  const uint32_t columns = (n_lin + kNearPatch - 1u) / kNearPatch;
  const uint32_t kx24 = static_cast<uint32_t>(k48) & 0xffffffu;
  const uint32_t fx = static_cast<uint32_t>(k48) & 0xffffu;
  const uint32_t fy = static_cast<uint32_t>(k48 >> 24) & 0xffffu;
  // the carry grows with d: the lattice's x steps produce those of d_min and d_max (and,
  // were the steps wider than the field, the ones between)
  const int32_t carry_lo = near_x_carry(kx24, d_min), carry_hi = near_x_carry(kx24, d_max);
  uint32_t x_bits = 0, y_bits = 0;
  for (uint32_t col = 0; col < columns; ++col)
  {
    const Fractions f = fractions + col * kNearPatch;
    if (near_possible(fx, f)) x_bits |= 1u << col;
    if (near_possible(fy + static_cast<uint32_t>(carry_lo), f)) y_bits |= 1u << col;
  }
  // (a beam at the edge of the x field, the only one whose lanes differ in their carry: in a
  // pass of its own, so that the pass above is the same work for every beam)
  for (int32_t carry = carry_lo + 1; carry <= carry_hi; ++carry)
  {
    for (uint32_t col = 0; col < columns; ++col)
    {
      if (near_possible(fy + static_cast<uint32_t>(carry), fractions + col * kNearPatch)) y_bits |= 1u << col;
    }
  }
  return (static_cast<uint64_t>(y_bits) << 32) | x_bits;
}

}  // namespace ndt2d

#endif  // NDT2D_NEAR_BITS_H_
