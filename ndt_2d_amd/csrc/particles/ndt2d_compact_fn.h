// The integer arithmetic of the order-preserving compaction (particles/ndt2d_compact.h): a lane's
// rank among the set bits of its wave's ballot, and the chunk of tiles a thread of the one-block scan
// takes.  Plain C++ without HIP types, host and device; tests/cpp/compact_fn_check.cpp checks it.
#ifndef NDT2D_COMPACT_FN_H_
#define NDT2D_COMPACT_FN_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_COMPACT_HD __host__ __device__
#else
#define NDT2D_COMPACT_HD
#endif

namespace ndt2d
{
namespace particles
{

constexpr uint32_t kScanThreads = 256;   // the scan's one block

NDT2D_COMPACT_HD inline uint32_t popcount64(uint64_t v)
{
  v = v - ((v >> 1) & 0x5555555555555555ull);
  v = (v & 0x3333333333333333ull) + ((v >> 2) & 0x3333333333333333ull);
  v = (v + (v >> 4)) & 0x0f0f0f0f0f0f0f0full;
  return static_cast<uint32_t>((v * 0x0101010101010101ull) >> 56);
}

// The set lanes of a 64-lane ballot below `lane`: the lane's exclusive rank in its wave.
NDT2D_COMPACT_HD inline uint32_t rank_in_wave(uint64_t ballot, uint32_t lane)
{
  return popcount64(ballot & ((1ull << lane) - 1ull));
}

// ... up to and including `lane`: the inclusive rank.
NDT2D_COMPACT_HD inline uint32_t rank_in_wave_inclusive(uint64_t ballot, uint32_t lane)
{
  return popcount64(ballot & (~0ull >> (63u - lane)));
}

struct Chunk
{
  uint32_t lo, hi;
};

// The tiles [lo, hi) of thread t (0 .. 255) of the scan over n_tiles tiles: ceil(n_tiles / 256) a
// thread, the last chunks short or empty.  t * chunk is taken in 64 bits: it passes 2^32 for large
// n_tiles.
NDT2D_COMPACT_HD inline Chunk scan_chunk(uint32_t t, uint32_t n_tiles)
{
  const uint32_t chunk = n_tiles / kScanThreads + (n_tiles % kScanThreads != 0 ? 1u : 0u);
  const uint64_t lo64 = static_cast<uint64_t>(t) * chunk;
  Chunk c;
  c.lo = lo64 < n_tiles ? static_cast<uint32_t>(lo64) : n_tiles;
  c.hi = n_tiles - c.lo > chunk ? c.lo + chunk : n_tiles;
  return c;
}

}  // namespace particles
}  // namespace ndt2d

#endif  // NDT2D_COMPACT_FN_H_
