// Device layer, the NDT grid of a context: installed from host records (dense, or as the list of
// its touched cells), built on the device, read back, and the read-only view of it that the
// kernels living beside the context take (batch/ndt2d_batch_host.h installed_grid).
#include <algorithm>
#include <limits>

#include "device/ndt2d_context.h"

using namespace ndt2d_device;

using ndt2d::GridDesc;
using ndt2d::kCellDoubles;
using ndt2d::kCellStrideGlobal;

extern "C" {

int ndt2d_set_grid(ndt2d_handle h, const double * cells6, uint32_t size_x, uint32_t size_y,
                   double cell_size, double origin_x, double origin_y)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (cells6 == nullptr || size_x == 0 || size_y == 0 || !(cell_size > 0.0))
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_grid: bad argument");
  }
  const uint64_t ncell64 = static_cast<uint64_t>(size_x) * size_y;
  if (ncell64 >= (1ull << 31)) return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_grid: grid too large");
  const uint32_t ncell = static_cast<uint32_t>(ncell64);
  NDT2D_HIP(h, hipSetDevice(h->device));
  // The old grid is gone from here on (ensure() may free its buffers): a failure
  // below leaves the context without a grid, never with dangling pointers.
  h->has_grid = false;
  h->bytes_job.n = 0;
  h->stage_cap = 0;   // an open ndt2d_grid_stage_begin is void: this call takes the staging buffer

  // The cells6 records travel once, through pinned staging (the caller's buffer is
  // free on return); the device derives the layouts the scorers read -- packed records
  // h = -0.5 * information with the sentinel for cells that cannot score (n < 5,
  // reference src/ndt_model.cpp:107), their 64-byte-stride copy, the occupancy bitmap
  // and the per-cell map bytes -- in ndt2d_build.hip.  Asynchronous on the stream.
  int rc;
  const size_t n6 = static_cast<size_t>(ncell) * 6;
  // Small maps also get the records of the cells that can score in compacted form, with
  // a cell -> record table (the small-lattice search keeps both in LDS): built here, on
  // the pass over the cells that copies them into the staging buffer anyway.
  uint32_t n_occ = 0;
  const bool compactable = ncell < 65535u;
  if (compactable)
  {
    for (uint32_t i = 0; i < ncell; ++i) n_occ += !(cells6[6 * static_cast<size_t>(i) + 5] < 5.0) ? 1u : 0u;
  }
  const size_t n_compact = compactable ? static_cast<size_t>(n_occ + 1) * kCellDoubles : 0;
  // (uint16 in doubles, whole 16-byte pieces: the kernel copies it with 16-byte loads)
  const size_t n_rank = compactable ? (static_cast<size_t>(ncell) + 1 + 7) / 8 * 2 : 0;
  const size_t n_upload = n6 + n_compact + n_rank;
  if ((rc = ensure(h, h->compact, n_upload)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cells_lds_image, static_cast<size_t>(ncell + 1) * kCellDoubles)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cells_global, static_cast<size_t>(ncell + 1) * kCellStrideGlobal)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->occ_bits, ((static_cast<size_t>(ncell) + 1 + 31) / 32 + 2) / 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cell_bytes, (static_cast<size_t>(size_x) + 2) * (size_y + 2) / 8 + 1)) != NDT2D_OK) return rc;
  if ((rc = stage_acquire(h, h->stage_grid, n_upload)) != NDT2D_OK) return rc;
  std::memcpy(h->stage_grid.ptr, cells6, n6 * sizeof(double));
  if (compactable)
  {
    double * recs = h->stage_grid.ptr + n6;
    uint16_t * rank = reinterpret_cast<uint16_t *>(recs + n_compact);
    uint32_t k = 0;
    for (uint32_t i = 0; i < ncell; ++i)
    {
      const double * c = cells6 + 6 * static_cast<size_t>(i);
      if (!(c[5] < 5.0))
      {
        double * r = recs + static_cast<size_t>(k) * kCellDoubles;
        r[0] = c[0];
        r[1] = c[1];
        r[2] = -0.5 * c[2];
        r[3] = -0.5 * c[3];
        r[4] = -0.5 * c[4];
        r[5] = 1.0;
        rank[i] = static_cast<uint16_t>(k++);
      }
      else
      {
        rank[i] = static_cast<uint16_t>(n_occ);
      }
    }
    rank[ncell] = static_cast<uint16_t>(n_occ);
    static const double sentinel[kCellDoubles] = {1.0e300, 0.0, -1.0, 0.0, -1.0, 0.0};
    std::memcpy(recs + static_cast<size_t>(n_occ) * kCellDoubles, sentinel, sizeof(sentinel));
  }
  if ((rc = stage_copy(h, h->stage_grid, h->compact.ptr, n_upload)) != NDT2D_OK) return rc;

  GridDesc g{};
  g.size_x = size_x;
  g.size_y = size_y;
  g.ncell = ncell;
  g.cell_size = cell_size;
  g.pow2 = is_pow2(cell_size) ? 1 : 0;
  g.inv_cell_size = 1.0 / cell_size;
  g.origin_x = origin_x;
  g.origin_y = origin_y;
  h->cells6_ptr = h->compact.ptr;
  h->sparse_n = 0;
  h->sparse_index = nullptr;
  h->sparse_cells6 = nullptr;
  hipError_t e = ndt2d::launch_pack_grid(g, h->cells6_ptr, h->cells_lds_image.ptr, h->cells_global.ptr,
                                         reinterpret_cast<uint32_t *>(h->occ_bits.ptr),
                                         reinterpret_cast<uint8_t *>(h->cell_bytes.ptr), h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_pack_grid");
  if ((rc = stage_mark(h, h->stage_grid)) != NDT2D_OK) return rc;   // (behind the kernel, see stage_copy)
  g.cells_lds_image = h->cells_lds_image.ptr;
  g.cells_global = h->cells_global.ptr;
  g.occ_bits = reinterpret_cast<const uint32_t *>(h->occ_bits.ptr);
  g.cell_bytes = reinterpret_cast<const uint8_t *>(h->cell_bytes.ptr);
  if (compactable)
  {
    g.compact_records = h->compact.ptr + n6;
    g.cell_rank = reinterpret_cast<const uint16_t *>(h->compact.ptr + n6 + n_compact);
    g.n_occ = n_occ;
  }
  h->grid = g;
  h->coarse_log2 = -1;
  h->block_bytes_log2 = -1;
  h->has_grid = true;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_build_grid(ndt2d_handle h, double ndt_resolution, double range_max,
                     const double * poses_xyt, const double * points_xy, const size_t * offsets,
                     size_t n_scans)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (!(ndt_resolution > 0.0) || n_scans == 0 || poses_xyt == nullptr || offsets == nullptr ||
      n_scans > (1u << 30))
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_build_grid: bad argument");
  }
  const size_t n_points = offsets[n_scans];
  if (n_points >= (1ull << 31) || (n_points > 0 && points_xy == nullptr))
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_build_grid: bad points");
  }
  // Extent: ScanMatcherNDT::addScans (reference src/scan_matcher_ndt.cpp:52-66); max_x_ /
  // max_y_ start at numeric_limits<double>::min() as the reference has it.
  double min_x = std::numeric_limits<double>::max(), max_x = std::numeric_limits<double>::min();
  double min_y = std::numeric_limits<double>::max(), max_y = std::numeric_limits<double>::min();
  for (size_t k = 0; k < n_scans; ++k)
  {
    min_x = std::min(poses_xyt[3 * k] - range_max, min_x);
    max_x = std::max(poses_xyt[3 * k] + range_max, max_x);
    min_y = std::min(poses_xyt[3 * k + 1] - range_max, min_y);
    max_y = std::max(poses_xyt[3 * k + 1] + range_max, max_y);
  }
  // NDT::NDT (src/ndt_model.cpp:118-126): size_x_ = (size_t)(size_x / cell_size + 1)
  const double fsx = ((max_x - min_x) / ndt_resolution) + 1;
  const double fsy = ((max_y - min_y) / ndt_resolution) + 1;
  if (!(fsx >= 1.0) || !(fsy >= 1.0) || fsx * fsy >= 2147483648.0)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_build_grid: degenerate grid extent");
  }
  const uint32_t size_x = static_cast<uint32_t>(static_cast<size_t>(fsx));
  const uint32_t size_y = static_cast<uint32_t>(static_cast<size_t>(fsy));
  const uint32_t ncell = size_x * size_y;
  NDT2D_HIP(h, hipSetDevice(h->device));
  // as in ndt2d_set_grid: no grid until the new one is complete
  h->has_grid = false;
  h->bytes_job.n = 0;
  h->stage_cap = 0;

  // staging that must stay alive until the copies are done: kept in the context
  NDT2D_SYNC(h);
  h->stage_scans.resize(4 * n_scans);
  h->stage_offsets.resize(((n_scans + 1) + 1) & ~size_t(1));
  for (size_t k = 0; k < n_scans; ++k)
  {
    h->stage_scans[4 * k] = poses_xyt[3 * k];
    h->stage_scans[4 * k + 1] = poses_xyt[3 * k + 1];
    ndt2d_cos_sin(poses_xyt[3 * k + 2], &h->stage_scans[4 * k + 2], &h->stage_scans[4 * k + 3]);  // :135-136, host libm
    h->stage_offsets[k] = static_cast<uint32_t>(offsets[k]);
  }
  h->stage_offsets[n_scans] = static_cast<uint32_t>(n_points);

  const size_t temp_bytes = ndt2d::build_sort_temp_bytes(static_cast<uint32_t>(n_points), ncell);
  int rc;
  if ((rc = ensure(h, h->b_points, 2 * n_points + 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->b_scans, 4 * n_scans)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->b_offsets, h->stage_offsets.size() / 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->b_world, 2 * n_points + 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->b_keys, n_points + 2)) != NDT2D_OK) return rc;   // 2 x u32 arrays
  if ((rc = ensure(h, h->b_vals, n_points + 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->b_temp, temp_bytes / 8 + 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->b_seg, static_cast<size_t>(ncell) + 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cells6, static_cast<size_t>(ncell) * 6)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cells_lds_image, static_cast<size_t>(ncell + 1) * kCellDoubles)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cells_global, static_cast<size_t>(ncell + 1) * kCellStrideGlobal)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->occ_bits, ((static_cast<size_t>(ncell) + 1 + 31) / 32 + 2) / 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cell_bytes, (static_cast<size_t>(size_x) + 2) * (size_y + 2) / 8 + 1)) != NDT2D_OK) return rc;

  if (n_points > 0)
  {
    NDT2D_HIP(h, hipMemcpyAsync(h->b_points.ptr, points_xy, 2 * n_points * sizeof(double),
                                hipMemcpyHostToDevice, h->stream));
  }
  NDT2D_HIP(h, hipMemcpyAsync(h->b_scans.ptr, h->stage_scans.data(), 4 * n_scans * sizeof(double),
                              hipMemcpyHostToDevice, h->stream));
  NDT2D_HIP(h, hipMemcpyAsync(h->b_offsets.ptr, h->stage_offsets.data(),
                              (n_scans + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));

  GridDesc g{};
  g.size_x = size_x;
  g.size_y = size_y;
  g.ncell = ncell;
  g.cell_size = ndt_resolution;
  g.pow2 = is_pow2(ndt_resolution) ? 1 : 0;
  g.inv_cell_size = 1.0 / ndt_resolution;
  g.origin_x = min_x;
  g.origin_y = min_y;

  ndt2d::BuildArgs a{};
  a.eigen_form = h->eigen_form;
  a.grid = g;
  a.points_xy = h->b_points.ptr;
  a.n_points = static_cast<uint32_t>(n_points);
  a.scans = h->b_scans.ptr;
  a.offsets = reinterpret_cast<const uint32_t *>(h->b_offsets.ptr);
  a.n_scans = static_cast<uint32_t>(n_scans);
  a.world_xy = h->b_world.ptr;
  a.keys_in = reinterpret_cast<uint32_t *>(h->b_keys.ptr);
  a.keys_out = a.keys_in + n_points + 1;
  a.vals_in = reinterpret_cast<uint32_t *>(h->b_vals.ptr);
  a.vals_out = a.vals_in + n_points + 1;
  a.sort_temp = h->b_temp.ptr;
  a.sort_temp_bytes = temp_bytes;
  a.seg_begin = reinterpret_cast<uint32_t *>(h->b_seg.ptr);
  a.cells6 = h->cells6.ptr;
  a.cells_lds_image = h->cells_lds_image.ptr;
  a.cells_global = h->cells_global.ptr;
  a.occ_bits = reinterpret_cast<uint32_t *>(h->occ_bits.ptr);
  a.cell_bytes = reinterpret_cast<uint8_t *>(h->cell_bytes.ptr);
  if (int trc = next_timing_slot(h); trc != NDT2D_OK) return trc;
  NDT2D_HIP(h, hipEventRecord(h->ev0, h->stream));
  hipError_t e = ndt2d::launch_build_grid(a, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_build_grid");
  NDT2D_HIP(h, hipEventRecord(h->ev1, h->stream));
  h->timed = true;
  h->last_kernels = 7;
  h->last_variant = "build/sort-by-cell+in-order-recurrence";

  g.cells_lds_image = h->cells_lds_image.ptr;
  g.cells_global = h->cells_global.ptr;
  g.occ_bits = reinterpret_cast<const uint32_t *>(h->occ_bits.ptr);
  g.cell_bytes = reinterpret_cast<const uint8_t *>(h->cell_bytes.ptr);
  h->cells6_ptr = h->cells6.ptr;
  h->sparse_n = 0;
  h->sparse_index = nullptr;
  h->sparse_cells6 = nullptr;
  if (ncell < 65535u)
  {
    // Small grids also get the compacted records + cell -> record table the searches keep in LDS
    // (as a host-installed grid does, ndt2d_set_grid): a loop closure's map is built here, and its
    // search was 8-20 % slower without them.  The count of scoring cells comes back to the host (the
    // kernels' LDS images are sized by it): one small copy behind the build.
    const size_t n_rec = static_cast<size_t>(ncell + 1) * kCellDoubles;
    const size_t n_rank = (static_cast<size_t>(ncell) + 1 + 7) / 8 * 2;
    if ((rc = ensure(h, h->compact, n_rec + n_rank + 2)) != NDT2D_OK) return rc;
    double * records = h->compact.ptr;
    uint16_t * ranks = reinterpret_cast<uint16_t *>(h->compact.ptr + n_rec);
    uint32_t * d_n_occ = reinterpret_cast<uint32_t *>(h->compact.ptr + n_rec + n_rank);
    e = ndt2d::launch_compact_grid(ncell, h->cells_lds_image.ptr, reinterpret_cast<const uint32_t *>(h->occ_bits.ptr),
                                   records, ranks, d_n_occ, h->stream);
    if (e != hipSuccess) return fail_hip(h, e, "launch_compact_grid");
    uint32_t n_occ = 0;
    NDT2D_HIP(h, hipMemcpyAsync(&n_occ, d_n_occ, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    NDT2D_SYNC(h);
    if (n_occ > 0)
    {
      g.compact_records = records;
      g.cell_rank = ranks;
      g.n_occ = n_occ;
    }
  }
  h->grid = g;
  h->coarse_log2 = -1;
  h->block_bytes_log2 = -1;
  h->has_grid = true;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

// Largest [rank table | compacted records] image any search kernel would keep in LDS
// (ndt2d_match_small.hip: 72 KB together with its map and rows; ndt2d_match_lane.hip: half a
// CU's LDS minus its map): beyond it the compacted form is not prepared.
static constexpr size_t kCompactImageBudget = 80 * 1024;

// Layout of the staged image of a list install for a capacity of `cap` listed cells (doubles):
// [cells6: 6 cap][cell indices: cap u32][ranks of the listed cells: cap u16][compact records:
// (cap + 1) x 6][occupancy words of the grid]
struct StageLayout
{
  size_t n6, n_idx, n_rk, n_compact_max, off_occ, n_words, n_upload;
};
static StageLayout stage_layout(size_t cap, uint32_t ncell, bool with_compact)
{
  StageLayout l{};
  l.n6 = cap * 6;
  l.n_idx = (cap + 1) / 2;
  l.n_rk = (cap + 3) / 4;
  if ((l.n6 + l.n_idx + l.n_rk) & 1) ++l.n_rk;   // the compact records are read with 16-byte loads
  l.n_compact_max = with_compact ? (cap + 1) * kCellDoubles : 0;
  // (occupancy words of the cells that can score: they tell the install kernel which cells
  // the list will write, ndt2d_build.hip)
  l.n_words = (static_cast<size_t>(ncell) + 1 + 31) / 32;
  l.off_occ = l.n6 + l.n_idx + l.n_rk + l.n_compact_max;
  l.n_upload = l.off_occ + (l.n_words + 1) / 2 + 2;
  return l;
}

int ndt2d_grid_stage_begin(ndt2d_handle h, uint32_t size_x, uint32_t size_y, size_t capacity,
                           uint32_t ** cell_index_out, double ** cells6_out)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  h->stage_cap = 0;
  if (cell_index_out == nullptr || cells6_out == nullptr || size_x == 0 || size_y == 0 || capacity >= (1ull << 31))
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_grid_stage_begin: bad argument");
  }
  const uint64_t ncell64 = static_cast<uint64_t>(size_x) * size_y;
  if (ncell64 >= (1ull << 31)) return fail(h, NDT2D_ERR_INVALID, "ndt2d_grid_stage_begin: grid too large");
  const uint32_t ncell = static_cast<uint32_t>(ncell64);
  NDT2D_HIP(h, hipSetDevice(h->device));
  h->has_grid = false;   // (see ndt2d_set_grid)
  h->bytes_job.n = 0;
  const size_t cap = capacity > 0 ? capacity : 1;
  // the compacted records are prepared only when their image could fit a search kernel's LDS
  const size_t rank_table_bytes = (static_cast<size_t>(ncell) + 1 + 7) / 8 * 16;
  const bool may_compact = rank_table_bytes + 2 * kCellDoubles * sizeof(double) <= kCompactImageBudget;
  const StageLayout l = stage_layout(cap, ncell, may_compact);
  int rc;
  if ((rc = ensure(h, h->compact, l.n_upload)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cells_lds_image, static_cast<size_t>(ncell + 1) * kCellDoubles)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cells_global, static_cast<size_t>(ncell + 1) * kCellStrideGlobal)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->occ_bits, ((static_cast<size_t>(ncell) + 1 + 31) / 32 + 2) / 2)) != NDT2D_OK) return rc;
  if ((rc = ensure(h, h->cell_bytes, (static_cast<size_t>(size_x) + 2) * (size_y + 2) / 8 + 1)) != NDT2D_OK) return rc;
  if (may_compact && (rc = ensure(h, h->ranks, rank_table_bytes / sizeof(double) + 2)) != NDT2D_OK) return rc;
  if ((rc = stage_acquire(h, h->stage_grid, l.n_upload)) != NDT2D_OK) return rc;
  h->stage_cap = cap;
  h->stage_sx = size_x;
  h->stage_sy = size_y;
  h->stage_may_compact = may_compact;
  *cells6_out = h->stage_grid.ptr;
  *cell_index_out = reinterpret_cast<uint32_t *>(h->stage_grid.ptr + l.n6);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_grid_stage_commit(ndt2d_handle h, size_t n_listed, double cell_size, double origin_x, double origin_y)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (h->stage_cap == 0) return fail(h, NDT2D_ERR_STATE, "ndt2d_grid_stage_commit: no ndt2d_grid_stage_begin before it");
  const size_t cap = h->stage_cap;
  h->stage_cap = 0;
  if (n_listed > cap || !(cell_size > 0.0)) return fail(h, NDT2D_ERR_INVALID, "ndt2d_grid_stage_commit: bad argument");
  const uint32_t size_x = h->stage_sx, size_y = h->stage_sy;
  const uint32_t ncell = size_x * size_y;
  const uint32_t n = static_cast<uint32_t>(n_listed);
  const StageLayout l = stage_layout(cap, ncell, h->stage_may_compact);
  const size_t n6 = l.n6, n_idx = l.n_idx, n_rk = l.n_rk, off_occ = l.off_occ, n_words = l.n_words, n_upload = l.n_upload;
  double * st = h->stage_grid.ptr;
  const double * cells6 = st;
  uint32_t * st_idx = reinterpret_cast<uint32_t *>(st + n6);
  const uint32_t * cell_index = st_idx;
  for (uint32_t k = 0; k < n; ++k)
  {
    if (cell_index[k] >= ncell) return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_grid_sparse: cell index out of range");
  }
  uint32_t n_occ = 0;
  for (uint32_t k = 0; k < n; ++k) n_occ += !(cells6[6 * static_cast<size_t>(k) + 5] < 5.0) ? 1u : 0u;
  const size_t rank_table_bytes = (static_cast<size_t>(ncell) + 1 + 7) / 8 * 16;
  const bool compactable = h->stage_may_compact && n_occ > 0 && n_occ < 65535u &&
                           rank_table_bytes + (static_cast<size_t>(n_occ) + 1) * kCellDoubles * sizeof(double) <=
                             kCompactImageBudget;
  const size_t n_compact = compactable ? static_cast<size_t>(n_occ + 1) * kCellDoubles : 0;
  int rc;
  uint16_t * st_rk = reinterpret_cast<uint16_t *>(st + n6 + n_idx);
  double * st_rec = st + n6 + n_idx + n_rk;
  uint32_t * st_occ = reinterpret_cast<uint32_t *>(st + off_occ);
  std::memset(st_occ, 0, (n_words + 1) / 2 * sizeof(double));
  uint32_t k_occ = 0;
  // every cell at most once, whether it can score or not (two records for one cell: whichever
  // thread stored last would win, in the install kernel or in ndt2d_get_grid's scatter)
  h->stage_seen.assign(n_words, 0u);
  for (uint32_t k = 0; k < n; ++k)
  {
    const double * c = cells6 + 6 * static_cast<size_t>(k);
    {
      const uint32_t bit = 1u << (cell_index[k] & 31u);
      if (h->stage_seen[cell_index[k] >> 5] & bit)
      {
        return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_grid_sparse: a cell is listed twice");
      }
      h->stage_seen[cell_index[k] >> 5] |= bit;
    }
    if (!(c[5] < 5.0))
    {
      const uint32_t bit = 1u << (cell_index[k] & 31u);
      st_occ[cell_index[k] >> 5] |= bit;
      if (compactable)
      {
        double * r = st_rec + static_cast<size_t>(k_occ) * kCellDoubles;
        r[0] = c[0];
        r[1] = c[1];
        r[2] = -0.5 * c[2];
        r[3] = -0.5 * c[3];
        r[4] = -0.5 * c[4];
        r[5] = 1.0;
      }
      st_rk[k] = static_cast<uint16_t>(k_occ++);
    }
    else
    {
      st_rk[k] = static_cast<uint16_t>(n_occ);
    }
  }
  if (compactable)
  {
    static const double sentinel[kCellDoubles] = {1.0e300, 0.0, -1.0, 0.0, -1.0, 0.0};
    std::memcpy(st_rec + static_cast<size_t>(n_occ) * kCellDoubles, sentinel, sizeof(sentinel));
  }
  // the install kernel reads the staged image in place and leaves the device copy behind; a
  // staging buffer the device cannot address is copied first
  ndt2d::SparseImage image{};
  image.n = n;
  image.off_idx = n6;
  image.off_rk = n6 + n_idx;
  image.off_compact = n6 + n_idx + n_rk;
  image.n_compact = n_compact;
  image.off_occ = off_occ;
  if (h->stage_grid.dev != nullptr)
  {
    image.src = h->stage_grid.dev;
    image.dst = h->compact.ptr;
  }
  else
  {
    if ((rc = stage_copy(h, h->stage_grid, h->compact.ptr, n_upload)) != NDT2D_OK) return rc;
    image.src = h->compact.ptr;
    image.dst = nullptr;
  }

  GridDesc g{};
  g.size_x = size_x;
  g.size_y = size_y;
  g.ncell = ncell;
  g.cell_size = cell_size;
  g.pow2 = is_pow2(cell_size) ? 1 : 0;
  g.inv_cell_size = 1.0 / cell_size;
  g.origin_x = origin_x;
  g.origin_y = origin_y;
  const double * d_cells6 = h->compact.ptr;
  const uint32_t * d_idx = reinterpret_cast<const uint32_t *>(h->compact.ptr + n6);
  hipError_t e = ndt2d::launch_grid_install(
    g, image, h->cells_lds_image.ptr, h->cells_global.ptr, reinterpret_cast<uint32_t *>(h->occ_bits.ptr),
    reinterpret_cast<uint8_t *>(h->cell_bytes.ptr),
    compactable ? reinterpret_cast<uint16_t *>(h->ranks.ptr) : nullptr, n_occ, h->stream);
  if (e != hipSuccess) return fail_hip(h, e, "launch_grid_install");
  // The map bytes around the listed cells (they read the records the install has just written):
  // queued right behind it.  Until round 6 the job waited for the next few-pose launch to carry
  // it -- the mapper's scoreScan -- or ran ahead of the next search; since a short scan's single
  // pose is scored on the host (round 4) it always ended up in front of the search, on the
  // critical path of the mapper's cycle.  Here it runs while the host prepares that search.
  g.cells_lds_image = h->cells_lds_image.ptr;
  g.cells_global = h->cells_global.ptr;
  g.occ_bits = reinterpret_cast<const uint32_t *>(h->occ_bits.ptr);
  g.cell_bytes = reinterpret_cast<const uint8_t *>(h->cell_bytes.ptr);
  {
    ndt2d::SparseBytesJob job{};
    job.cell_index = d_idx;
    job.cells6 = d_cells6;
    job.n = n;
    job.bytes = reinterpret_cast<uint8_t *>(h->cell_bytes.ptr);
    e = ndt2d::launch_sparse_bytes(g, job, h->stream);
    if (e != hipSuccess) return fail_hip(h, e, "launch_sparse_bytes");
    h->bytes_job.n = 0;
  }
  // (behind the install kernel, which reads the buffer in place)
  if ((rc = stage_mark(h, h->stage_grid)) != NDT2D_OK) return rc;
  if (compactable)
  {
    g.compact_records = h->compact.ptr + n6 + n_idx + n_rk;
    g.cell_rank = reinterpret_cast<const uint16_t *>(h->ranks.ptr);
    g.n_occ = n_occ;
  }
  h->cells6_ptr = nullptr;          // made from the list when ndt2d_get_grid asks for them
  h->sparse_n = n;
  h->sparse_index = d_idx;
  h->sparse_cells6 = d_cells6;
  h->grid = g;
  h->coarse_log2 = -1;
  h->block_bytes_log2 = -1;
  h->has_grid = true;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_set_grid_sparse(ndt2d_handle h, const uint32_t * cell_index, const double * cells6,
                          size_t n_listed, uint32_t size_x, uint32_t size_y, double cell_size,
                          double origin_x, double origin_y)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if ((n_listed > 0 && (cell_index == nullptr || cells6 == nullptr)) || size_x == 0 || size_y == 0 ||
      !(cell_size > 0.0) || n_listed >= (1ull << 31))
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_grid_sparse: bad argument");
  }
  uint32_t * st_idx = nullptr;
  double * st_cells6 = nullptr;
  const int rc = ndt2d_grid_stage_begin(h, size_x, size_y, n_listed, &st_idx, &st_cells6);
  if (rc != NDT2D_OK) return rc;
  if (n_listed > 0)
  {
    std::memcpy(st_cells6, cells6, n_listed * 6 * sizeof(double));
    std::memcpy(st_idx, cell_index, n_listed * sizeof(uint32_t));
  }
  return ndt2d_grid_stage_commit(h, n_listed, cell_size, origin_x, origin_y);
  NDT2D_C_CATCH(h)
}

int ndt2d_set_eigenvalue_form(ndt2d_handle h, const char * form)
{
  NDT2D_C_TRY
  if (h == nullptr || form == nullptr) return NDT2D_ERR_INVALID;
  if (std::strcmp(form, "eigen") == 0) h->eigen_form = 0;
  else if (std::strcmp(form, "closed") == 0) h->eigen_form = 1;
  else return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_eigenvalue_form: unknown form (eigen, closed)");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_get_grid(ndt2d_handle h, double * cells6_out, size_t capacity_cells, uint32_t * size_x,
                   uint32_t * size_y, double * cell_size, double * origin_x, double * origin_y)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_get_grid: no grid");
  if (size_x) *size_x = h->grid.size_x;
  if (size_y) *size_y = h->grid.size_y;
  if (cell_size) *cell_size = h->grid.cell_size;
  if (origin_x) *origin_x = h->grid.origin_x;
  if (origin_y) *origin_y = h->grid.origin_y;
  if (cells6_out != nullptr)
  {
    if (capacity_cells < h->grid.ncell) return fail(h, NDT2D_ERR_INVALID, "ndt2d_get_grid: capacity");
    NDT2D_HIP(h, hipSetDevice(h->device));
    if (h->cells6_ptr == nullptr)
    {
      // a grid installed as a list: the dense records from the list, once
      int rc = ensure(h, h->cells6, static_cast<size_t>(h->grid.ncell) * 6);
      if (rc != NDT2D_OK) return rc;
      hipError_t e = ndt2d::launch_grid_sparse_to_dense(h->sparse_index, h->sparse_cells6, h->sparse_n,
                                                        h->grid.ncell, h->cells6.ptr, h->stream);
      if (e != hipSuccess) return fail_hip(h, e, "launch_grid_sparse_to_dense");
      h->cells6_ptr = h->cells6.ptr;
    }
    NDT2D_HIP(h, hipMemcpyAsync(cells6_out, h->cells6_ptr,
                                static_cast<size_t>(h->grid.ncell) * 6 * sizeof(double),
                                hipMemcpyDeviceToHost, h->stream));
    NDT2D_SYNC(h);
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_clear_grid(ndt2d_handle h)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  h->has_grid = false;
  h->bytes_job.n = 0;
  h->stage_cap = 0;   // (an open list is dropped with the grid it was for)
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_has_grid(ndt2d_handle h) { return (h != nullptr && h->has_grid) ? 1 : 0; }

int ndt2d_grid_view_get(ndt2d_handle h, ndt2d_grid_view * out)
{
  NDT2D_C_TRY
  if (h == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_grid_view_get: no grid");
  const GridDesc & g = h->grid;
  out->cells_global = g.cells_global;
  out->occ_bits = g.occ_bits;
  out->size_x = g.size_x;
  out->size_y = g.size_y;
  out->ncell = g.ncell;
  out->pow2 = g.pow2;
  out->cell_size = g.cell_size;
  out->inv_cell_size = g.inv_cell_size;
  out->origin_x = g.origin_x;
  out->origin_y = g.origin_y;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

}  // extern "C"
