// near_bits() (csrc/ndt2d_near_bits.h), the word the large search's table pre-kernel leaves beside
// every beam's K, against the per-lane test of lane_beams (csrc/ndt2d_lane_fn.h) restated here on
// the host exactly as the kernel has it: ONE f64 addition K + D, the x fraction in bytes 0, 1 of
// the sum and the y fraction in bytes 3, 4, each compared with 2 * kNearUnits.  For designed K and
// lattices, bit px must be the OR of the lanes' x test over the steps of patch column px, and bit
// 32 + py the OR of their y test over the steps of patch row py and EVERY x step of the lattice
// (the y fraction takes the carry out of the x field).  A program of its own, no GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ndt2d_near_bits.h"

namespace
{

constexpr double kTwo24 = 16777216.0;
constexpr double kTwo52 = 4503599627370496.0;

int failures = 0;
long long checked_bits = 0, set_bits = 0, lanes_near_x = 0, lanes_near_y = 0, carry_beams = 0;

// lane_beams: s = o.z + dxy; lo, hi = the words of s; near_boundary(lo) | near_boundary(fy),
// fy = v_perm_b32(hi, lo, 0x0c0c0403) = lo.byte3 | hi.byte0 << 8
void lane_near(double K, double dxy, bool * near_x, bool * near_y)
{
  const double s = K + dxy;
  uint64_t u;
  std::memcpy(&u, &s, sizeof u);
  const uint32_t lo = static_cast<uint32_t>(u), hi = static_cast<uint32_t>(u >> 32);
  const uint32_t fy = (lo >> 24) | ((hi & 0xffu) << 8);
  *near_x = (lo & 0xffffu) < 2u * ndt2d::kNearUnits;
  *near_y = fy < 2u * ndt2d::kNearUnits;
}

struct Lattice
{
  uint32_t n_lin;
  double inv_scaled;
  std::vector<double> dlin;
  std::vector<double> units;        // near_offset_units of every step, as packed_offset() takes them
  std::vector<uint16_t> fractions;  // what the pre-kernel's block makes: 256 entries
  int32_t d_min, d_max;
};

Lattice make_lattice(uint32_t n_lin, double resolution, double inv_scaled)
{
  Lattice l;
  l.n_lin = n_lin;
  l.inv_scaled = inv_scaled;
  for (uint32_t i = 0; i < n_lin; ++i) l.dlin.push_back((static_cast<double>(i) - 0.5 * n_lin) * resolution);
  for (uint32_t i = 0; i < n_lin; ++i) l.units.push_back(ndt2d::near_offset_units(l.dlin[i], inv_scaled));
  l.d_min = INT32_MAX;
  l.d_max = INT32_MIN;
  for (uint32_t i = 0; i < ndt2d::kNearPatch * ndt2d::kNearColumns; ++i)
  {
    const int32_t u = static_cast<int32_t>(l.units[i < n_lin ? i : n_lin - 1]);
    l.fractions.push_back(static_cast<uint16_t>(static_cast<uint32_t>(u)));
    if (i < n_lin && u < l.d_min) l.d_min = u;
    if (i < n_lin && u > l.d_max) l.d_max = u;
  }
  return l;
}

void check_beam(const Lattice & l, uint64_t k48)
{
  const double K = kTwo52 + static_cast<double>(k48);
  const uint64_t bits = ndt2d::near_bits(k48, l.fractions.data(), l.n_lin, l.d_min, l.d_max);
  if (l.n_lin > ndt2d::kNearPatch * ndt2d::kNearColumns)
  {
    if (bits != ndt2d::kNearAll)
    {
      ++failures;
      std::printf("FAILED n_lin %u: %016llx, not all ones\n", l.n_lin, static_cast<unsigned long long>(bits));
    }
    return;
  }
  const uint32_t columns = (l.n_lin + ndt2d::kNearPatch - 1) / ndt2d::kNearPatch;
  uint32_t x_lanes = 0, y_lanes = 0;
  bool carries[3] = {false, false, false};
  for (uint32_t ix = 0; ix < l.n_lin; ++ix)
  {
    // (the carry this x step sends into the y field, counted for the summary line)
    const double x_field = static_cast<double>(k48 & 0xffffffu) + l.units[ix];
    carries[x_field < 0.0 ? 0 : (x_field < kTwo24 ? 1 : 2)] = true;
    for (uint32_t iy = 0; iy < l.n_lin; ++iy)
    {
      bool nx, ny;
      lane_near(K, l.units[iy] * kTwo24 + l.units[ix], &nx, &ny);   // packed_offset()
      if (nx) x_lanes |= 1u << (ix / ndt2d::kNearPatch), ++lanes_near_x;
      if (ny) y_lanes |= 1u << (iy / ndt2d::kNearPatch), ++lanes_near_y;
    }
  }
  if (carries[0] + carries[1] + carries[2] > 1) ++carry_beams;
  const uint64_t expected = (static_cast<uint64_t>(y_lanes) << 32) | x_lanes;
  checked_bits += 2 * columns;
  set_bits += __builtin_popcountll(expected);
  if (bits != expected)
  {
    ++failures;
    if (failures <= 20)
    {
      std::printf("FAILED n_lin %u inv_scaled %.1f k48 %012llx: near_bits %016llx, lanes %016llx\n", l.n_lin,
                  l.inv_scaled, static_cast<unsigned long long>(k48), static_cast<unsigned long long>(bits),
                  static_cast<unsigned long long>(expected));
    }
  }
}

}  // namespace

int main()
{
  // cfg-1: 0.25 m cells, one map cell per grid cell, 0.05 m steps; cfg-2: 4 x 4 sub-cells, 0.02 m steps
  const double scales[2][2] = {{0.05, 4.0 * 65536.0}, {0.02, 4.0 * 65536.0 * 4.0}};
  const uint32_t sizes[7] = {8, 21, 100, 101, 255, 256, 257};
  const uint32_t fractions[12] = {0, 3, 4, 5, 0xfff8, 0xfff9, 0xfffa, 0xfffb, 0xfffc, 0xfffd, 0xfffe, 0xffff};
  int beams = 0;
  for (const auto & scale : scales)
  {
    for (const uint32_t n_lin : sizes)
    {
      const Lattice l = make_lattice(n_lin, scale[0], scale[1]);
      std::vector<uint64_t> ks;
      // the designed fractions on both axes, in the middle of the map
      for (const uint32_t fx : fractions)
      {
        for (const uint32_t fy : fractions) ks.push_back((uint64_t{0x50} << 40) | (uint64_t{fy} << 24) | (0x40u << 16) | fx);
      }
      // fractions that put a chosen step exactly on, one unit inside and one unit outside either
      // end of the band, on x, on y and on both
      const uint32_t steps[4] = {0, n_lin / 2, n_lin - 2, n_lin - 1};
      for (const uint32_t step : steps)
      {
        for (const int32_t at : {-1, 0, 1, 6, 7, 8})
        {
          const uint32_t f = (static_cast<uint32_t>(at) - l.fractions[step < l.fractions.size() ? step : l.fractions.size() - 1]) & 0xffffu;
          ks.push_back((uint64_t{0x50} << 40) | (uint64_t{0x1234} << 24) | (0x40u << 16) | f);
          ks.push_back((uint64_t{0x50} << 40) | (uint64_t{f} << 24) | (0x40u << 16) | 0x4321u);
          ks.push_back((uint64_t{0x50} << 40) | (uint64_t{f} << 24) | (0x40u << 16) | f);
        }
      }
      // x fields whose sum with some step leaves the 24 bits -- a borrow at the low end, a carry at
      // the high end, for some steps of the lattice and not for others -- with y fractions that
      // the carry moves into and out of the band
      for (const uint32_t kx : {0x000000u, 0x000003u, 0x000400u, 0xfffffdu, 0xfffc00u, 0xffffffu})
      {
        for (const uint32_t fy : {0u, 1u, 7u, 8u, 9u, 0xfff7u, 0xfff8u, 0xffffu})
        {
          ks.push_back((uint64_t{0x50} << 40) | (uint64_t{fy} << 24) | kx);
          const uint32_t f = (fy - l.fractions[n_lin / 2]) & 0xffffu;
          ks.push_back((uint64_t{0x50} << 40) | (uint64_t{f} << 24) | kx);
        }
      }
      for (const uint64_t k48 : ks) check_beam(l, k48);
      beams += static_cast<int>(ks.size());
    }
  }
  std::printf("%d beams, %lld bits checked, %lld set, %lld lanes near on x, %lld on y, %d beams with two carries\n",
              beams, checked_bits, set_bits, lanes_near_x, lanes_near_y, static_cast<int>(carry_beams));
  if (set_bits == 0 || carry_beams == 0 || set_bits == checked_bits) ++failures, std::printf("FAILED: a vacuous run\n");
  std::printf(failures == 0 ? "OK\n" : "FAILED %d\n", failures);
  return failures == 0 ? 0 : 1;
}
