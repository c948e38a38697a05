// pretest_level_bound() / pretest_level_passes() (csrc/ndt2d_pretest_level.h), the large search's
// pre-test against the wave's lowest skip level, checked against the plain maximum of a box's level
// bytes.  The kernel ORs the rows of the box into a word, masks the flag bits and the columns
// beyond the box, and folds the word's bytes: for words made the same way here,
//   the bound is never below the highest level byte of the box (so a beam the true maximum would
//   keep is never pruned), it equals it when one byte of the box is non-zero, level 63 passes
//   every skip level and an empty box passes none.
// A program of its own, no GPU.
#include <cstdint>
#include <cstdio>

#include "ndt2d_pretest_level.h"

namespace
{

int failures = 0;
long long words = 0, passes_bound = 0, passes_true = 0, kept_for_the_or = 0;

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rng()   // xorshift64*
{
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545f4914f6cdd1dull;
}

void fail(const char * what, uint32_t a, uint32_t b, uint32_t c)
{
  if (++failures <= 10) std::printf("FAILED %s: %08x %08x %08x\n", what, a, b, c);
}

// the highest level byte (flag bits clear) among the columns the mask keeps
uint32_t true_maximum(const uint8_t * bytes, int n, int rows, int span)
{
  uint32_t m = 0;
  for (int r = 0; r < rows; ++r)
  {
    for (int col = 0; col <= span; ++col)
    {
      const uint32_t b = bytes[r * n + col] & ndt2d::kLevelBits;
      m = b > m ? b : m;
    }
  }
  return m;
}

// every skip level a lane can hold, in the byte's layout, against one box
void check_box(uint32_t bound, uint32_t maximum, uint32_t w0, uint32_t w1)
{
  ++words;
  if (bound < maximum) fail("bound below the maximum", bound, maximum, w0);
  if ((bound & ~ndt2d::kLevelBits) != 0u) fail("bound outside the level bits", bound, w0, w1);
  if ((maximum == 0u) != (bound == 0u)) fail("empty box", bound, maximum, w0);
  for (uint32_t level = 1; level <= 63; ++level)
  {
    const uint32_t l = level << ndt2d::kLevelShift;
    const bool by_bound = ndt2d::pretest_level_passes(bound, l);
    const bool by_maximum = maximum != 0u && maximum >= l;
    passes_bound += by_bound;
    passes_true += by_maximum;
    kept_for_the_or += by_bound && !by_maximum;
    if (by_maximum && !by_bound) fail("pruned a beam the maximum keeps", bound, maximum, l);
    if (maximum == (63u << ndt2d::kLevelShift) && !by_bound) fail("level 63 must pass", bound, maximum, l);
    if (maximum == 0u && by_bound) fail("level 0 must fail", bound, maximum, l);
  }
  // (below the lowest skip level the test is the any-non-zero test)
  if (ndt2d::pretest_level_passes(bound, 0u) != (maximum != 0u)) fail("level 0 threshold", bound, maximum, 0);
  if (ndt2d::pretest_level_passes(bound, ndt2d::kLowestSkipLevel) != (maximum != 0u)) fail("lowest level", bound, maximum, 4);
}

// patch_box_word: up to four rows of four bytes, columns 0 .. span kept
void patch_box(const uint8_t (&bytes)[16], int rows, int span)
{
  uint32_t any = 0;
  for (int r = 0; r < rows; ++r)
  {
    uint32_t w = 0;
    for (int col = 0; col < 4; ++col) w |= static_cast<uint32_t>(bytes[r * 4 + col]) << (8 * col);
    any |= w;
  }
  const uint32_t columns = span >= 3 ? ndt2d::kLevelColumns : (ndt2d::kLevelColumns >> (8 * (3 - span)));
  const uint32_t word = any & columns;
  check_box(ndt2d::pretest_level_bound(word), true_maximum(bytes, 4, rows, span), word, 0u);
}

// strip_box_word: up to eight rows of eight bytes in two words, columns 0 .. span_x kept
void strip_box(const uint8_t (&bytes)[64], int rows, int span_x)
{
  uint32_t any_lo = 0, any_hi = 0;
  for (int r = 0; r < rows; ++r)
  {
    for (int col = 0; col < 4; ++col)
    {
      any_lo |= static_cast<uint32_t>(bytes[r * 8 + col]) << (8 * col);
      any_hi |= static_cast<uint32_t>(bytes[r * 8 + 4 + col]) << (8 * col);
    }
  }
  const uint64_t columns = 0xfcfcfcfcfcfcfcfcull >> (8 * (7 - span_x));
  const uint32_t lo = any_lo & static_cast<uint32_t>(columns), hi = any_hi & static_cast<uint32_t>(columns >> 32);
  const uint32_t bound = ndt2d::pretest_level_bound(lo, hi);
  if (bound != ndt2d::pretest_level_bound(lo | hi)) fail("two words against their OR", bound, lo, hi);
  check_box(bound, true_maximum(bytes, 8, rows, span_x), lo, hi);
}

}  // namespace

int main()
{
  // every single non-zero byte, in every column and row of both boxes: the bound is the byte's level
  long long singles = 0;
  for (uint32_t value = 1; value < 256; ++value)
  {
    for (int at = 0; at < 16; ++at)
    {
      uint8_t bytes[16] = {};
      bytes[at] = static_cast<uint8_t>(value);
      uint32_t any = 0;
      for (int i = 0; i < 16; ++i) any |= static_cast<uint32_t>(bytes[i]) << (8 * (i & 3));
      const uint32_t bound = ndt2d::pretest_level_bound(any & ndt2d::kLevelColumns);
      if (bound != (value & ndt2d::kLevelBits)) fail("single byte", bound, value, static_cast<uint32_t>(at));
      for (int span = 0; span <= 3; ++span) patch_box(bytes, 4, span);
      ++singles;
    }
    for (int at = 0; at < 64; ++at)
    {
      uint8_t bytes[64] = {};
      bytes[at] = static_cast<uint8_t>(value);
      for (int span = 0; span <= 7; ++span) strip_box(bytes, 8, span);
      ++singles;
    }
  }
  // the issue's own pair: levels 5 and 2 with their flag bits (bytes 20 | 3 and 8 | 3): OR 28 | 3 --
  // kept at level 6 and 7 although the maximum is 5, pruned from level 8
  {
    uint8_t bytes[16] = {};
    bytes[1] = 20;
    bytes[6] = 11;
    uint32_t any = (20u << 8) | (11u << 16);
    const uint32_t bound = ndt2d::pretest_level_bound(any & ndt2d::kLevelColumns);
    if (bound != 28u) fail("20 | 11", bound, any, 0);
    if (!ndt2d::pretest_level_passes(bound, 24u) || !ndt2d::pretest_level_passes(bound, 28u)) fail("20 | 11 kept", bound, 24, 28);
    if (ndt2d::pretest_level_passes(bound, 32u)) fail("20 | 11 pruned", bound, 32, 0);
    patch_box(bytes, 4, 3);
  }
  // random boxes: sparse ones (most bytes 0, as in a map) and dense ones, every span and row count
  for (int i = 0; i < 400000; ++i)
  {
    uint8_t bytes[64];
    const uint64_t density = rng() % 5;   // 0: dense ... 4: one byte in sixteen
    for (int k = 0; k < 64; ++k)
    {
      const uint64_t r = rng();
      bytes[k] = (r >> 8) % (1ull << density) == 0 ? static_cast<uint8_t>(r) : 0;
    }
    uint8_t first[16];
    for (int k = 0; k < 16; ++k) first[k] = bytes[k];
    patch_box(first, 1 + static_cast<int>(rng() % 4), static_cast<int>(rng() % 4));
    strip_box(bytes, 1 + static_cast<int>(rng() % 8), static_cast<int>(rng() % 8));
  }
  // ... and random masked OR words as such, against the maximum of their own bytes
  for (int i = 0; i < 3000000; ++i)
  {
    const uint32_t word = static_cast<uint32_t>(rng()) & static_cast<uint32_t>(rng() >> 32) & ndt2d::kLevelColumns;
    uint32_t maximum = 0;
    for (int col = 0; col < 4; ++col)
    {
      const uint32_t b = (word >> (8 * col)) & 0xffu;
      maximum = b > maximum ? b : maximum;
    }
    check_box(ndt2d::pretest_level_bound(word), maximum, word, 0u);
  }
  std::printf("%lld words, %lld single-byte boxes, %lld (word, level) pairs pass by the bound, %lld by the maximum, %lld kept for the OR alone\n",
              words, singles, passes_bound, passes_true, kept_for_the_or);
  std::printf(failures == 0 ? "OK\n" : "FAILED\n");
  return failures == 0 ? 0 : 1;
}
