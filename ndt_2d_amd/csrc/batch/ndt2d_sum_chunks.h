// The partial sums of a lattice candidate's score in the batched searches (closure/, starts/, scans/):
// the beam chunks of the small-lattice search's default plan (ndt2d_match_small.hip small_plan:
// groups of four beams, chunks of five groups, at most eight chunks), a function of the beam
// count alone.  Plain C++: host code and a stand-alone check include it without the HIP headers.
#ifndef NDT2D_SUM_CHUNKS_H_
#define NDT2D_SUM_CHUNKS_H_

#include <stdint.h>

namespace ndt2d
{

constexpr uint32_t kGroupBeams = 4;           // the small-lattice search's look-up group
constexpr uint32_t kMaxSumChunks = 8;

inline uint32_t sum_chunks(uint32_t n_beams)
{
  const uint32_t groups = (n_beams + kGroupBeams - 1) / kGroupBeams;
  uint32_t best_c = (groups + 4) / 5;
  if (best_c > kMaxSumChunks) best_c = kMaxSumChunks;
  if (best_c < 1) best_c = 1;
  const uint32_t chunk_groups = (groups + best_c - 1) / best_c;
  return chunk_groups == 0 ? 1u : (groups + chunk_groups - 1) / chunk_groups;
}

}  // namespace ndt2d

#endif  // NDT2D_SUM_CHUNKS_H_
