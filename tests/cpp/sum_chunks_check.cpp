// Host-only check of the chunk plan the batched searches share (ndt_2d_amd/csrc/batch/ndt2d_sum_chunks.h):
// the values worked out by hand from the small-lattice search's default plan (groups of four beams,
// chunks of five groups, at most eight chunks) at the beam counts the tests use, and -- for every
// count up to 4,096 -- the plan transcribed from ndt2d_match_small.hip small_plan.
#include <cstdint>
#include <cstdio>

#include "ndt2d_sum_chunks.h"

// small_plan's own arithmetic (kSmallUnroll = 4, best_c = ceil(groups / 5) clamped to 1 .. 8)
static uint32_t small_plan_chunks(uint32_t n_beams)
{
  const uint32_t groups = (n_beams + 4 - 1) / 4;
  uint32_t best_c = (groups + 4) / 5;
  if (best_c > 8) best_c = 8;
  if (best_c < 1) best_c = 1;
  const uint32_t chunk_groups = (groups + best_c - 1) / best_c;
  return (groups + chunk_groups - 1) / chunk_groups;
}

int main()
{
  const uint32_t cases[6][2] = {{1, 1}, {4, 1}, {5, 1}, {100, 5}, {720, 8}, {1500, 8}};
  int bad = 0;
  for (const auto & c : cases)
  {
    const uint32_t got = ndt2d::sum_chunks(c[0]);
    std::printf("beams %u: chunks %u (expected %u)\n", c[0], got, c[1]);
    if (got != c[1]) ++bad;
  }
  for (uint32_t n = 1; n <= 4096; ++n)
  {
    if (ndt2d::sum_chunks(n) != small_plan_chunks(n) || ndt2d::sum_chunks(n) > ndt2d::kMaxSumChunks) ++bad;
  }
  if (ndt2d::kGroupBeams != 4 || ndt2d::kMaxSumChunks != 8) ++bad;
  std::printf(bad == 0 ? "OK\n" : "FAILED\n");
  return bad == 0 ? 0 : 1;
}
