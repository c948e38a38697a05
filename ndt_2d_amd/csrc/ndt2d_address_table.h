// The large search's window table of record addresses (ndt2d_lane_fn.h: lane_beams, ndt2d_match_lane.hip:
// the staging of match_lane_body).  Plain integer C++, no HIP header: the search kernels and the host
// check (tests/cpp/address_table_check.cpp) compile the same lines.
//
// The compacted-records forms keep the records of the cells that can score in LDS, behind the map.
// An exact evaluation used to go from its look-up coordinate to its record by way of the grid:
// row * size_x + col - idx_bias, a select on the map byte's occupancy bit (the padded window reaches
// beyond the grid), the grid's cell -> rank table, rank * 48 + the records' address.  Everything in
// that but the lane's two coordinate bytes is fixed for the launch, so a block now stages a table
// shaped like the WINDOW instead of a copy of the grid's rank table: one entry per cell of the padded
// window, rows of a power-of-two stride, an entry = the LDS byte address of the cell's record (or the
// record's rank in a byte: see kRankEntryBytes).  A
// window cell outside the grid, a cell that cannot score and the filler columns behind the window's
// width hold the sentinel record's address, and so does one entry behind the last row: "outside", what
// the near-boundary path selects for a point the reference's index arithmetic puts off the grid.
//
// The table trusts GridDesc::cell_rank where the per-cell route also asked the map byte's bit 0.  The
// two agree: bit 0 of a sub-cell inside the grid is the cell's bit of the occupancy bitmap
// (sub_cell_byte), and every installer writes rank n_occ exactly for the cells whose bit is clear --
// the host installs count and rank by the bitmap's own test !(n < 5), compact_grid_kernel ranks the
// bitmap's set bits.
#ifndef NDT2D_ADDRESS_TABLE_H_
#define NDT2D_ADDRESS_TABLE_H_

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NDT2D_ADDRESS_HD __host__ __device__
#else
#define NDT2D_ADDRESS_HD
#endif

namespace ndt2d
{

struct AddressTableShape
{
  uint32_t rows;         // cells of the padded window along y: win_h + 2 * pad
  uint32_t cols;         // ... along x: win_w + 2 * pad
  uint32_t stride_log2;  // entries per row: the smallest power of two that holds cols
};

NDT2D_ADDRESS_HD inline AddressTableShape address_table_shape(int32_t win_w, int32_t win_h, int32_t pad)
{
  AddressTableShape s;
  s.rows = static_cast<uint32_t>(win_h + 2 * pad);
  s.cols = static_cast<uint32_t>(win_w + 2 * pad);
  s.stride_log2 = 0;
  while ((1u << s.stride_log2) < s.cols) ++s.stride_log2;
  return s;
}

// Entry of "outside": the one behind the last row.
NDT2D_ADDRESS_HD inline uint32_t address_table_outside(const AddressTableShape & s) { return s.rows << s.stride_log2; }

NDT2D_ADDRESS_HD inline uint32_t address_table_entries(const AddressTableShape & s) { return address_table_outside(s) + 1u; }

// An entry is the record's LDS byte address (32 bits), or, where two blocks' images do not fit a CU with
// that, the record's rank in one byte (a grid of fewer than 256 cells that can score): the address is
// then one multiply-add away, as it was behind the grid's rank table.
constexpr uint32_t kAddressEntryBytes = 4;
constexpr uint32_t kRankEntryBytes = 1;
constexpr uint32_t kRankEntryMaxRecords = 256;   // n_occ + 1 (the sentinel's) ranks in a byte

// LDS bytes of the table, rounded to the 16 bytes the records behind it are aligned to.
NDT2D_ADDRESS_HD inline uint32_t address_table_bytes(const AddressTableShape & s, uint32_t entry_bytes)
{
  return (address_table_entries(s) * entry_bytes + 15u) & ~15u;
}

// Entry of window cell (col, row), what the interior path forms from the lane's two coordinate bytes.
NDT2D_ADDRESS_HD inline uint32_t address_table_entry(const AddressTableShape & s, uint32_t col, uint32_t row)
{
  return (row << s.stride_log2) + col;
}

// Rank of the record an entry stands for.  The window's cell (0, 0) is grid cell (win_x0 - pad, win_y0 - pad).
NDT2D_ADDRESS_HD inline uint32_t address_table_rank(const uint16_t * cell_rank, uint32_t size_x, uint32_t size_y,
                                                    uint32_t n_occ, int32_t win_x0, int32_t win_y0, int32_t pad,
                                                    const AddressTableShape & s, uint32_t entry)
{
  const uint32_t row = entry >> s.stride_log2;
  const uint32_t col = entry & ((1u << s.stride_log2) - 1u);
  if (row >= s.rows || col >= s.cols) return n_occ;
  const int32_t cx = static_cast<int32_t>(col) - pad + win_x0;
  const int32_t cy = static_cast<int32_t>(row) - pad + win_y0;
  if (cx < 0 || cy < 0 || cx >= static_cast<int32_t>(size_x) || cy >= static_cast<int32_t>(size_y)) return n_occ;
  return cell_rank[static_cast<uint32_t>(cy) * size_x + static_cast<uint32_t>(cx)];
}

NDT2D_ADDRESS_HD inline uint32_t address_table_value(uint32_t records_address, uint32_t rank, uint32_t record_bytes)
{
  return records_address + rank * record_bytes;
}

// The near-boundary path: entry of the grid cell (gx, gy) the reference's index arithmetic gave, or of
// "outside" (inside == false; also a cell beyond the padded window, which no point of the search
// reaches: the window holds every point the scan, the pose and the lattice can produce).
// off_x = pad - win_x0, off_y = pad - win_y0, modulo 2^32.
NDT2D_ADDRESS_HD inline uint32_t address_table_entry_of_cell(const AddressTableShape & s, uint32_t off_x,
                                                             uint32_t off_y, bool inside, uint32_t gx, uint32_t gy)
{
  const uint32_t col = gx + off_x, row = gy + off_y;
  return (inside && col < s.cols && row < s.rows) ? address_table_entry(s, col, row) : address_table_outside(s);
}

}  // namespace ndt2d

#endif  // NDT2D_ADDRESS_TABLE_H_
