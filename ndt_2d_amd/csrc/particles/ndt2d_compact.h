// Order-preserving compaction without atomics, for 256-thread blocks of four waves: a tile is the
// 256 items of one block.  Three device functions, one for each launch of the unit that compacts; the
// unit's kernels supply the flag and what is done with the rank:
//
//   tile_count      flagged items of this tile: one ballot and one popcount per wave
//   scan_tile_sums  exclusive scan of the tile counts in ONE block: a chunk of tiles per thread
//                   (particles/ndt2d_compact_fn.h), a fixed doubling tree over the 256 chunk sums in LDS
//   tile_rank       the same ballots again: a lane's rank is its tile's offset plus its waves' counts
//                   before it plus the popcount of the ballot bits below it (tile_rank_inclusive: up
//                   to and including it)
//
// Every thread of the block calls them (they hold block barriers).  Integer sums: any order gives the
// same counts.
#ifndef NDT2D_COMPACT_H_
#define NDT2D_COMPACT_H_

#include <hip/hip_runtime.h>

#include "particles/ndt2d_compact_fn.h"

namespace ndt2d
{
namespace particles
{

constexpr int kCompactBlock = 256;
constexpr int kCompactWaves = kCompactBlock / 64;

__device__ __forceinline__ void tile_count(bool flag, uint32_t * __restrict__ sums)
{
  __shared__ uint32_t sh[kCompactWaves];
  const uint32_t c = static_cast<uint32_t>(__popcll(__ballot(flag)));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// sums[b] -> the flagged items in the tiles before b; returns the total, valid in the last thread
__device__ __forceinline__ uint32_t scan_tile_sums(uint32_t * sums, uint32_t n_tiles)
{
  __shared__ uint32_t sh[kCompactBlock];
  const uint32_t t = threadIdx.x;
  const Chunk c = scan_chunk(t, n_tiles);
  uint32_t mine = 0;
  for (uint32_t b = c.lo; b < c.hi; ++b) mine += sums[b];
  sh[t] = mine;
  __syncthreads();
  for (uint32_t d = 1; d < kCompactBlock; d <<= 1)
  {
    const uint32_t add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  uint32_t run = sh[t] - mine;
  for (uint32_t b = c.lo; b < c.hi; ++b)
  {
    const uint32_t s = sums[b];
    sums[b] = run;
    run += s;
  }
  return sh[t];
}

template <bool kInclusive>
__device__ __forceinline__ uint32_t tile_rank_of(bool flag, const uint32_t * __restrict__ sums)
{
  __shared__ uint32_t sh[kCompactWaves];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long ballot = __ballot(flag);
  if (lane == 0) sh[wave] = static_cast<uint32_t>(__popcll(ballot));
  __syncthreads();
  if (!kInclusive && !flag) return 0;   // (nobody asks: a wave without a flagged item loads nothing)
  uint32_t rank = sums[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) rank += sh[w];
  return rank + (kInclusive ? rank_in_wave_inclusive(ballot, lane) : rank_in_wave(ballot, lane));
}

// the flagged items before this thread's (meaningful where `flag` is set)
__device__ __forceinline__ uint32_t tile_rank(bool flag, const uint32_t * __restrict__ sums)
{
  return tile_rank_of<false>(flag, sums);
}

// the flagged items up to and including this thread's, in every thread
__device__ __forceinline__ uint32_t tile_rank_inclusive(bool flag, const uint32_t * __restrict__ sums)
{
  return tile_rank_of<true>(flag, sums);
}

}  // namespace particles
}  // namespace ndt2d

#endif  // NDT2D_COMPACT_H_
