// The window table of record addresses (csrc/ndt2d_address_table.h) of the large search's
// compacted-records forms, checked against the per-cell route it replaces:
//   interior path:  cell = row * size_x + col - idx_bias (modulo 2^32), idx = the map byte's bit 0 ? cell : -1,
//                   rank = rank_table[idx] (entry -1 and entry ncell: the sentinel's, n_occ),
//                   address = records + 48 * rank
//   near path:      cell = NDT::getIndex's gy * size_x + gx, or ncell outside the grid, then the same table
// over every cell of the padded window, the filler columns and "outside", for windows inside the grid, far
// from its origin, clipped at each corner, wider than the grid, on grids with size_x != size_y (both odd),
// with one occupied cell, none in range, every cell, and random occupancy.  Bit 0 of a map byte is the
// occupancy of the sub-cell's own grid cell (0 outside the grid), which is what the rank table encodes.
// A program of its own, no GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ndt2d_address_table.h"

namespace
{

int failures = 0;
long long byte_rank_windows = 0, windows = 0, window_cells = 0, padding_cells = 0, sentinel_entries = 0, near_cells = 0, near_beyond_window = 0;

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rng()   // xorshift64*
{
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545f4914f6cdd1dull;
}

void fail(const char * what, long long a, long long b, long long c, long long d)
{
  if (++failures <= 10) std::printf("FAILED %s: %lld %lld %lld %lld\n", what, a, b, c, d);
}

constexpr uint32_t kRecordBytes = 48;
constexpr uint32_t kLead = 8;   // uint16 entries in front of entry 0 of the rank table; the last is entry -1

struct Grid
{
  uint32_t size_x, size_y, n_occ;
  std::vector<uint8_t> occupied;   // per cell
  std::vector<uint16_t> rank;      // kLead entries, then ncell + 1
  const uint16_t * cell_rank() const { return rank.data() + kLead; }
};

// kind 0: random third, 1: one cell (the given one), 2: every cell, 3: first and last row and column
Grid make_grid(uint32_t size_x, uint32_t size_y, int kind, uint32_t one_cell)
{
  Grid g;
  g.size_x = size_x;
  g.size_y = size_y;
  const uint32_t ncell = size_x * size_y;
  g.occupied.assign(ncell, 0);
  for (uint32_t i = 0; i < ncell; ++i)
  {
    const uint32_t x = i % size_x, y = i / size_x;
    if (kind == 0) g.occupied[i] = rng() % 3 == 0;
    if (kind == 1) g.occupied[i] = i == one_cell;
    if (kind == 2) g.occupied[i] = 1;
    if (kind == 3) g.occupied[i] = x == 0 || y == 0 || x == size_x - 1 || y == size_y - 1;
  }
  g.n_occ = 0;
  for (uint32_t i = 0; i < ncell; ++i) g.n_occ += g.occupied[i];
  g.rank.assign(kLead + ncell + 1, 0xffffu);
  uint32_t k = 0;
  for (uint32_t i = 0; i < ncell; ++i) g.rank[kLead + i] = static_cast<uint16_t>(g.occupied[i] ? k++ : g.n_occ);
  g.rank[kLead + ncell] = static_cast<uint16_t>(g.n_occ);
  g.rank[kLead - 1] = static_cast<uint16_t>(g.n_occ);
  return g;
}

void check_window(const Grid & g, int32_t win_x0, int32_t win_y0, int32_t win_w, int32_t win_h, int32_t pad,
                  uint32_t records_address)
{
  ++windows;
  const uint32_t ncell = g.size_x * g.size_y;
  const ndt2d::AddressTableShape s = ndt2d::address_table_shape(win_w, win_h, pad);
  if (s.rows != static_cast<uint32_t>(win_h + 2 * pad) || s.cols != static_cast<uint32_t>(win_w + 2 * pad)) fail("shape", s.rows, s.cols, win_w, win_h);
  if ((1u << s.stride_log2) < s.cols || (s.stride_log2 > 0 && (1u << (s.stride_log2 - 1)) >= s.cols)) fail("stride", s.stride_log2, s.cols, 0, 0);
  const uint32_t n = ndt2d::address_table_entries(s);
  for (uint32_t width : {ndt2d::kAddressEntryBytes, ndt2d::kRankEntryBytes})
  {
    const uint32_t bytes = ndt2d::address_table_bytes(s, width);
    if (n != (s.rows << s.stride_log2) + 1u || bytes < width * n || bytes % 16u != 0u || bytes >= width * n + 16u) fail("bytes", n, bytes, width, 0);
  }
  // the table as a block stages it (the vector's bounds are the sanitizer's to watch)
  // (with one-byte entries the kernel keeps the rank and makes the same address from it: records + 48 * rank)
  std::vector<uint32_t> table(n);
  std::vector<uint8_t> ranks(n);
  const bool byte_ranks = g.n_occ + 1u <= ndt2d::kRankEntryMaxRecords;
  for (uint32_t i = 0; i < n; ++i)
  {
    const uint32_t rank = ndt2d::address_table_rank(g.cell_rank(), g.size_x, g.size_y, g.n_occ, win_x0, win_y0, pad, s, i);
    if (rank > g.n_occ) fail("rank beyond the sentinel", i, rank, g.n_occ, 0);
    table[i] = ndt2d::address_table_value(records_address, rank, kRecordBytes);
    ranks[i] = static_cast<uint8_t>(rank);
    if (byte_ranks && records_address + kRecordBytes * ranks[i] != table[i]) fail("rank in a byte", i, rank, ranks[i], 0);
  }
  if (byte_ranks) ++byte_rank_windows;
  const uint32_t sentinel = records_address + g.n_occ * kRecordBytes;
  if (table[ndt2d::address_table_outside(s)] != sentinel) fail("outside", table[n - 1], sentinel, 0, 0);
  // interior path: every cell of the padded window by the per-cell route
  const uint32_t idx_bias = static_cast<uint32_t>(pad - win_y0) * g.size_x + static_cast<uint32_t>(pad - win_x0);
  for (uint32_t row = 0; row < s.rows; ++row)
  {
    for (uint32_t col = 0; col < (1u << s.stride_log2); ++col)
    {
      const uint32_t entry = ndt2d::address_table_entry(s, col, row);
      if (entry >= n - 1u) fail("entry beyond the table", col, row, entry, n);
      if (col >= s.cols)
      {
        if (table[entry] != sentinel) fail("filler column", col, row, table[entry], sentinel);
        continue;
      }
      ++window_cells;
      const int32_t cx = static_cast<int32_t>(col) - pad + win_x0, cy = static_cast<int32_t>(row) - pad + win_y0;
      const bool in_grid = cx >= 0 && cy >= 0 && cx < static_cast<int32_t>(g.size_x) && cy < static_cast<int32_t>(g.size_y);
      if (!in_grid) ++padding_cells;
      const uint32_t cell = row * g.size_x + (col - idx_bias);
      if (in_grid && cell != static_cast<uint32_t>(cy) * g.size_x + static_cast<uint32_t>(cx)) fail("idx_bias", col, row, cell, 0);
      const bool bit0 = in_grid && g.occupied[cell] != 0;       // the map byte's occupancy bit
      const int32_t idx = bit0 ? static_cast<int32_t>(cell) : -1;
      const uint32_t want = records_address + kRecordBytes * g.cell_rank()[idx];
      if (table[entry] != want) fail("interior path", col, row, table[entry], want);
      if (want == sentinel) ++sentinel_entries;
    }
  }
  // near path: every grid cell and a ring of "outside" round the grid
  const uint32_t off_x = static_cast<uint32_t>(pad - win_x0), off_y = static_cast<uint32_t>(pad - win_y0);
  for (int32_t gy = -2; gy < static_cast<int32_t>(g.size_y) + 2; ++gy)
  {
    for (int32_t gx = -2; gx < static_cast<int32_t>(g.size_x) + 2; ++gx)
    {
      const bool inside = gx >= 0 && gy >= 0 && gx < static_cast<int32_t>(g.size_x) && gy < static_cast<int32_t>(g.size_y);
      // (outside, the kernel's truncated coordinates are whatever the conversion gave)
      const uint32_t ux = inside ? static_cast<uint32_t>(gx) : static_cast<uint32_t>(rng());
      const uint32_t uy = inside ? static_cast<uint32_t>(gy) : static_cast<uint32_t>(rng());
      const uint32_t entry = ndt2d::address_table_entry_of_cell(s, off_x, off_y, inside, ux, uy);
      if (entry >= n) fail("near entry beyond the table", gx, gy, entry, n);
      const uint32_t cell = inside ? uy * g.size_x + ux : ncell;
      const uint32_t want = records_address + kRecordBytes * g.cell_rank()[cell];
      ++near_cells;
      const bool in_window = inside && ux + off_x < s.cols && uy + off_y < s.rows;
      if (inside && !in_window)
      {
        // beyond the padded window: no point of a search lands here; the table says "outside"
        ++near_beyond_window;
        if (table[entry] != sentinel) fail("beyond the window", gx, gy, table[entry], sentinel);
      }
      else if (table[entry] != want)
      {
        fail("near path", gx, gy, table[entry], want);
      }
    }
  }
}

}  // namespace

int main()
{
  struct Size { uint32_t x, y; };
  const Size sizes[] = {{41, 41}, {37, 53}, {53, 37}, {9, 7}, {201, 201}, {1, 1}, {255, 3}};
  for (const Size & size : sizes)
  {
    for (int kind = 0; kind < 4; ++kind)
    {
      const Grid g = make_grid(size.x, size.y, kind, kind == 1 ? static_cast<uint32_t>(rng() % (size.x * size.y)) : 0u);
      if (g.n_occ >= 65535u) continue;
      const int32_t sx = static_cast<int32_t>(size.x), sy = static_cast<int32_t>(size.y);
      for (int32_t pad : {3, 4, 7, 13})
      {
        // the whole grid; windows at each corner, far from the origin, of one cell; random ones
        check_window(g, 0, 0, sx, sy, pad, 0x4000u);
        for (int corner = 0; corner < 4; ++corner)
        {
          const int32_t w = sx > 5 ? 5 : sx, h = sy > 3 ? 3 : sy;
          check_window(g, (corner & 1) ? sx - w : 0, (corner & 2) ? sy - h : 0, w, h, pad, 0x3100u + 16u * static_cast<uint32_t>(corner));
        }
        check_window(g, sx - 1, sy - 1, 1, 1, pad, 0xc400u);
        for (int k = 0; k < 20; ++k)
        {
          const int32_t x0 = static_cast<int32_t>(rng() % size.x), y0 = static_cast<int32_t>(rng() % size.y);
          const int32_t w = 1 + static_cast<int32_t>(rng() % static_cast<uint32_t>(sx - x0));
          const int32_t h = 1 + static_cast<int32_t>(rng() % static_cast<uint32_t>(sy - y0));
          if (w + 2 * pad > 256 || h + 2 * pad > 256) continue;   // (the one-byte coordinate)
          check_window(g, x0, y0, w, h, pad, 256u * static_cast<uint32_t>(h + 2 * pad) + 16u * static_cast<uint32_t>(rng() % 4096u));
        }
      }
    }
  }
  std::printf("%lld windows with ranks in a byte, ", byte_rank_windows);
  std::printf("%lld windows, %lld window cells (%lld outside the grid, %lld at the sentinel), %lld near cells (%lld beyond the window)\n",
              windows, window_cells, padding_cells, sentinel_entries, near_cells, near_beyond_window);
  if (failures != 0)
  {
    std::printf("FAILED: %d\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
