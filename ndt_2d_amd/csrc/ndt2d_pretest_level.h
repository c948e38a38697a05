// The large search's patch pre-test, made aware of the wave's skip levels (ndt2d_lane_fn.h:
// patch_box_word / strip_box_word, ndt2d_match_lane.hip: the chunk loop).  Plain integer C++, no
// HIP header: the search kernels and the host check (tests/cpp/pretest_level_check.cpp) compile
// the same lines.
//
// A map byte is (level << 2) | flags, level 0 .. 63 (map_byte()).  The pre-test ORs the bytes of
// the box a patch's 64 candidates can reach with one beam, four (or eight) columns side by side
// in a word, columns beyond the box and the flag bits masked away.  The OR of bytes is >= every
// one of them, so the OR of the word's own bytes is an upper bound of the highest level in the
// box, in the byte's layout.  A lane is live for a beam only if its map byte is >= the lane's
// skip level (SkipState::skip_level, the same layout); with L = the least skip level of the
// wave's lanes, a beam whose bound is below L has no live lane, whatever the lanes hold.
#ifndef NDT2D_PRETEST_LEVEL_H_
#define NDT2D_PRETEST_LEVEL_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NDT2D_PRETEST_HD __host__ __device__
#else
#define NDT2D_PRETEST_HD
#endif

namespace ndt2d
{

constexpr uint32_t kLevelShift = 2;          // a byte's level sits in bits 2..7
constexpr uint32_t kLevelBits = 0xfcu;
constexpr uint32_t kLevelColumns = 0xfcfcfcfcu;
// The lowest skip level a lane can hold (skip_state() clamps to 1 .. 63), in the byte's layout:
// what every lane holds before its first term.  Against it the level test is the plain
// "any byte of the box non-zero" test.
constexpr uint32_t kLowestSkipLevel = 1u << kLevelShift;

// Upper bound of the highest level byte among the columns of a masked OR word: the OR of its bytes.
NDT2D_PRETEST_HD inline uint32_t pretest_level_bound(uint32_t masked_or)
{
  const uint32_t halves = masked_or | (masked_or >> 16);
  return (halves | (halves >> 8)) & kLevelBits;
}

// ... of the strip test's two words (columns 0..3 and 4..7).
NDT2D_PRETEST_HD inline uint32_t pretest_level_bound(uint32_t masked_or_lo, uint32_t masked_or_hi)
{
  return pretest_level_bound(masked_or_lo | masked_or_hi);
}

// Can a lane whose skip level is at least `level` (level << 2, flag bits clear) be live in a box
// with this bound?  Bound 0 (nothing reachable) never passes; 63 << 2 (no claim) always does.
NDT2D_PRETEST_HD inline bool pretest_level_passes(uint32_t bound, uint32_t level)
{
  return bound >= (level > kLowestSkipLevel ? level : kLowestSkipLevel);
}

}  // namespace ndt2d

#endif  // NDT2D_PRETEST_LEVEL_H_
