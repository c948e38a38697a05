// Stand-alone check of ndt_2d_amd/csrc/particles/ndt2d_compact_fn.h: the popcount and the ranks of a
// lane in its wave's ballot against the compiler's builtin, the chunks of the one-block scan (they
// tile [0, n_tiles) exactly, up to n_tiles = 2^32 - 1), and the order-preserving compaction (tile
// counts, exclusive scan, ranks from ballots) run serially over random maps against a plain loop,
// with the seeder's free flag (seed/ndt2d_seed_fn.h) as the predicate.  Built with the host compiler
// (once more with -fsanitize=address,undefined) and run directly; no device, no library.  Exits
// non-zero when a check fails.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "particles/ndt2d_compact_fn.h"
#include "seed/ndt2d_seed_fn.h"

namespace P = ndt2d::particles;
namespace S = ndt2d::seed;

namespace
{

int failures = 0;

void check(bool ok, const char * what)
{
  if (!ok)
  {
    if (failures < 20) std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

struct SplitMix64
{
  uint64_t s;
  uint64_t next()
  {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

// The three launches of the table build, serially: 256 cells a tile, 64 lanes a wave.
std::vector<uint32_t> compact_as_launched(const std::vector<signed char> & map, uint32_t width,
                                          uint32_t x0, uint32_t y0, uint32_t w, uint32_t h)
{
  const uint32_t n = w * h, n_tiles = (n + 255) / 256;
  std::vector<uint64_t> ballots(static_cast<size_t>(n_tiles) * 4, 0);
  std::vector<uint32_t> sums(n_tiles, 0);
  for (uint32_t i = 0; i < n; ++i)
  {
    if (S::is_free(map[S::region_cell(i, x0, y0, w, width)])) ballots[i / 64] |= 1ull << (i % 64);
  }
  for (uint32_t t = 0; t < n_tiles; ++t)
  {
    for (int wv = 0; wv < 4; ++wv) sums[t] += P::popcount64(ballots[4 * t + wv]);
  }
  uint32_t run = 0;
  for (uint32_t t = 0; t < n_tiles; ++t)
  {
    const uint32_t c = sums[t];
    sums[t] = run;
    run += c;
  }
  std::vector<uint32_t> out(run, 0xffffffffu);
  for (uint32_t i = 0; i < n; ++i)
  {
    const uint32_t tile = i / 256, wave = (i % 256) / 64, lane = i % 64;
    const uint64_t ballot = ballots[4 * tile + wave];
    if (((ballot >> lane) & 1) == 0) continue;
    uint32_t rank = sums[tile];
    for (uint32_t wv = 0; wv < wave; ++wv) rank += P::popcount64(ballots[4 * tile + wv]);
    rank += P::rank_in_wave(ballot, lane);
    check(rank < out.size() && out[rank] == 0xffffffffu, "compaction: a rank outside the table or taken twice");
    if (rank < out.size()) out[rank] = S::region_cell(i, x0, y0, w, width);
  }
  return out;
}

}  // namespace

int main()
{
  SplitMix64 rng{2024};

  // ---- the ranks of a lane ----
  for (uint64_t v = 0; v < 4096; ++v)
  {
    const uint64_t r = rng.next();
    const uint32_t lane = static_cast<uint32_t>(v % 64);
    check(P::popcount64(r) == static_cast<uint32_t>(__builtin_popcountll(r)), "popcount64");
    check(P::rank_in_wave(r, lane) == static_cast<uint32_t>(__builtin_popcountll(r & ((1ull << lane) - 1))), "rank_in_wave");
    check(P::rank_in_wave_inclusive(r, lane) == P::rank_in_wave(r, lane) + static_cast<uint32_t>((r >> lane) & 1),
          "rank_in_wave_inclusive: the exclusive rank and the lane's own bit");
  }
  check(P::rank_in_wave(~0ull, 0) == 0 && P::rank_in_wave(~0ull, 63) == 63, "rank_in_wave: the end lanes");
  check(P::rank_in_wave_inclusive(~0ull, 0) == 1 && P::rank_in_wave_inclusive(~0ull, 63) == 64 &&
          P::rank_in_wave_inclusive(0ull, 63) == 0 && P::rank_in_wave_inclusive(1ull << 63, 62) == 0,
        "rank_in_wave_inclusive: the end lanes");

  // ---- the scan's chunks tile [0, n_tiles) exactly, without overflow ----
  {
    const uint32_t sizes[] = {0u, 1u, 255u, 256u, 257u, 65536u, (1u << 24) + 1u, 0xffffffffu};
    for (uint32_t n_tiles : sizes)
    {
      const uint64_t chunk = (static_cast<uint64_t>(n_tiles) + P::kScanThreads - 1) / P::kScanThreads;
      uint32_t next = 0;
      for (uint32_t t = 0; t < P::kScanThreads; ++t)
      {
        const P::Chunk c = P::scan_chunk(t, n_tiles);
        check(c.lo == next && c.hi >= c.lo && c.hi <= n_tiles, "scan_chunk: starts where the last one ended, inside the tiles");
        check(c.hi - c.lo <= chunk && (c.hi - c.lo == chunk || c.hi == n_tiles), "scan_chunk: ceil(n_tiles / 256) tiles, or what is left");
        next = c.hi;
      }
      check(next == n_tiles, "scan_chunk: the chunks end at n_tiles");
    }
  }

  // ---- the compaction over random maps ----
  {
    const signed char values[] = {0, 0, 0, -1, 100, 1, -128, 127};
    const uint32_t dims[][2] = {{1, 1}, {63, 5}, {64, 4}, {65, 9}, {255, 3}, {257, 7}, {300, 300}, {16, 16}, {1, 700}, {700, 1}};
    for (const auto & d : dims)
    {
      const uint32_t W = d[0], H = d[1];
      for (int density = 0; density < 4; ++density)
      {
        std::vector<signed char> map(static_cast<size_t>(W) * H);
        for (signed char & c : map)
        {
          const uint64_t r = rng.next();
          c = density == 0 ? static_cast<signed char>(0)
                           : (density == 1 ? static_cast<signed char>(100) : values[(r >> 8) % (density == 2 ? 8 : 4)]);
        }
        for (int reg = 0; reg < 4; ++reg)
        {
          uint32_t x0 = 0, y0 = 0, w = W, h = H;
          if (reg > 0)
          {
            w = 1 + static_cast<uint32_t>(rng.next() % W);
            h = 1 + static_cast<uint32_t>(rng.next() % H);
            x0 = reg == 1 ? 0 : (reg == 2 ? W - w : static_cast<uint32_t>(rng.next() % (W - w + 1)));
            y0 = reg == 1 ? 0 : (reg == 2 ? H - h : static_cast<uint32_t>(rng.next() % (H - h + 1)));
          }
          std::vector<uint32_t> want;
          for (uint32_t y = y0; y < y0 + h; ++y)
          {
            for (uint32_t x = x0; x < x0 + w; ++x)
            {
              if (map[static_cast<size_t>(y) * W + x] == 0) want.push_back(y * W + x);
            }
          }
          check(compact_as_launched(map, W, x0, y0, w, h) == want, "compaction: the table of a plain loop");
        }
      }
    }
  }

  if (failures != 0)
  {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
