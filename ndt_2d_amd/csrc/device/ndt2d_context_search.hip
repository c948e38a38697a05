// Device layer, the lattice search of a context: beams, search tables, launch and fetch.
#include <algorithm>
#include <limits>

#include "device/ndt2d_context.h"
#include "ndt2d_lane_fn.h"   // lane_strip_shape

using namespace ndt2d_device;

namespace
{

// Host-side figures of the translation lattice: its extent and the widest 8-step patch.
void lattice_extent(ndt2d_context * h, const double * dlin, size_t n_lin)
{
  h->dlin_absmax = 0.0;
  h->patch_span = 0.0;
  for (size_t i = 0; i < n_lin; ++i)
  {
    if (std::fabs(dlin[i]) > h->dlin_absmax) h->dlin_absmax = std::fabs(dlin[i]);
  }
  for (size_t i = 0; i < n_lin && h->patch_span >= 0.0; i += 8)
  {
    const size_t last = i + 7 < n_lin ? i + 7 : n_lin - 1;
    for (size_t k = i; k < last; ++k)
    {
      if (!(dlin[k + 1] >= dlin[k])) h->patch_span = -1.0;   // not ascending (or NaN): no claim
    }
    if (h->patch_span >= 0.0 && dlin[last] - dlin[i] > h->patch_span) h->patch_span = dlin[last] - dlin[i];
  }
  // the strip tiles of the lattice edge (ndt2d::lane_tiling): their long side's aligned groups,
  // and the short side -- the steps behind the last whole group of eight
  h->strip_span_long = h->strip_span_short = 0.0;
  uint32_t long_log2 = 0;
  if (!ndt2d::lane_strip_shape(static_cast<uint32_t>(n_lin), &long_log2)) return;
  for (size_t k = 0; k + 1 < n_lin; ++k)
  {
    if (!(dlin[k + 1] >= dlin[k])) return;   // not ascending (or NaN): no claim
  }
  const size_t group = static_cast<size_t>(1) << long_log2;
  for (size_t i = 0; i < n_lin; i += group)
  {
    const size_t last = i + group - 1 < n_lin ? i + group - 1 : n_lin - 1;
    if (dlin[last] - dlin[i] > h->strip_span_long) h->strip_span_long = dlin[last] - dlin[i];
  }
  h->strip_span_short = dlin[n_lin - 1] - dlin[n_lin / 8 * 8];
}

}  // namespace

// max |beam|; an infinite reach (NaN / inf beam) disables the windowed lane mapping
double ndt2d_device::beam_reach(const double * beams_xy, size_t n_beams)
{
  double rmax = 0.0;
  for (size_t i = 0; i < n_beams; ++i)
  {
    const double r = std::hypot(beams_xy[2 * i], beams_xy[2 * i + 1]);
    if (r > rmax) rmax = r;
    if (std::isnan(r)) rmax = std::numeric_limits<double>::infinity();
  }
  return rmax;
}

extern "C" {

int ndt2d_set_beams(ndt2d_handle h, const double * beams_xy, size_t n_beams)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (beams_xy == nullptr || n_beams == 0 || n_beams > (1u << 20))
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_beams: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->beams, 2 * n_beams + 2);
  if (rc != NDT2D_OK) return rc;
  rc = stage_acquire(h, h->stage_beams, 2 * n_beams);
  if (rc != NDT2D_OK) return rc;
  std::memcpy(h->stage_beams.ptr, beams_xy, 2 * n_beams * sizeof(double));
  rc = stage_submit(h, h->stage_beams, h->beams.ptr, 2 * n_beams);
  if (rc != NDT2D_OK) return rc;
  h->n_beams = n_beams;
  h->beams_ptr = h->beams.ptr;
  // a search prepared for other beams must be set up again (ndt2d_set_search) before
  // ndt2d_match_launch: its caller pairs the tables with THESE beams
  h->has_search = false;
  h->beam_rmax = beam_reach(beams_xy, n_beams);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_set_search(ndt2d_handle h, double pose_x, double pose_y, const double * dth,
                     const double * cos_th, const double * sin_th, size_t n_th,
                     const double * dlin, size_t n_lin)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (dth == nullptr || cos_th == nullptr || sin_th == nullptr || dlin == nullptr || n_th == 0 ||
      n_lin == 0 || n_th > (1u << 24) || n_lin > 46340)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_search: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  const size_t n_tab = 3 * n_th + n_lin;
  int rc = ensure(h, h->tables, n_tab);
  if (rc != NDT2D_OK) return rc;
  rc = stage_acquire(h, h->stage_tables, n_tab);
  if (rc != NDT2D_OK) return rc;
  double * t = h->stage_tables.ptr;
  std::memcpy(t, dth, n_th * sizeof(double));
  std::memcpy(t + n_th, cos_th, n_th * sizeof(double));
  std::memcpy(t + 2 * n_th, sin_th, n_th * sizeof(double));
  std::memcpy(t + 3 * n_th, dlin, n_lin * sizeof(double));
  h->tables_uploaded = false;   // ndt2d_match_launch uploads them if its kernel reads HBM
  h->n_th = n_th;
  h->n_lin = n_lin;
  lattice_extent(h, dlin, n_lin);
  h->pose_x = pose_x;
  h->pose_y = pose_y;
  h->tables_ptr = h->tables.ptr;
  h->has_search = true;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_set_search_beams(ndt2d_handle h, const double * beams_xy, size_t n_beams, double pose_x,
                           double pose_y, const double * dth, const double * cos_th,
                           const double * sin_th, size_t n_th, const double * dlin, size_t n_lin)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (beams_xy == nullptr)
  {
    // the beams the context holds stay: only the tables change (and need no copy yet)
    if (n_beams == 0 || n_beams != h->n_beams || h->beams_ptr == nullptr)
    {
      return fail(h, NDT2D_ERR_STATE, "ndt2d_set_search_beams: no such beams on the device");
    }
    return ndt2d_set_search(h, pose_x, pose_y, dth, cos_th, sin_th, n_th, dlin, n_lin);
  }
  if (n_beams == 0 || n_beams > (1u << 20) || dth == nullptr ||
      cos_th == nullptr || sin_th == nullptr || dlin == nullptr || n_th == 0 || n_lin == 0 ||
      n_th > (1u << 24) || n_lin > 46340)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_search_beams: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  // one staging buffer, one copy: [beams 2n][dth | cos | sin  3 n_th][dlin n_lin]
  const size_t n_tab = 3 * n_th + n_lin;
  const size_t n_all = 2 * n_beams + n_tab;
  int rc = ensure(h, h->call_dev, n_all);
  if (rc != NDT2D_OK) return rc;
  rc = stage_acquire(h, h->stage_call, n_all);
  if (rc != NDT2D_OK) return rc;
  double * t = h->stage_call.ptr;
  std::memcpy(t, beams_xy, 2 * n_beams * sizeof(double));
  t += 2 * n_beams;
  std::memcpy(t, dth, n_th * sizeof(double));
  std::memcpy(t + n_th, cos_th, n_th * sizeof(double));
  std::memcpy(t + 2 * n_th, sin_th, n_th * sizeof(double));
  std::memcpy(t + 3 * n_th, dlin, n_lin * sizeof(double));
  rc = stage_submit(h, h->stage_call, h->call_dev.ptr, n_all);
  if (rc != NDT2D_OK) return rc;
  h->n_beams = n_beams;
  h->beam_rmax = beam_reach(beams_xy, n_beams);
  h->beams_ptr = h->call_dev.ptr;
  h->tables_ptr = h->call_dev.ptr + 2 * n_beams;
  h->tables_uploaded = true;
  h->n_th = n_th;
  h->n_lin = n_lin;
  lattice_extent(h, dlin, n_lin);
  h->pose_x = pose_x;
  h->pose_y = pose_y;
  h->has_search = true;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_match_launch(ndt2d_handle h, size_t th_begin, size_t th_end, double * d_scores,
                       double * d_record)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (th_begin >= th_end) return fail(h, NDT2D_ERR_INVALID, "ndt2d_match_launch: bad theta range");
  return ndt2d_match_launch_strided(h, th_begin, 1, th_end - th_begin, d_scores, d_record);
  NDT2D_C_CATCH(h)
}

int ndt2d_match_launch_strided(ndt2d_handle h, size_t th_first, size_t th_stride, size_t th_count,
                               double * d_scores, double * d_record)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_match_launch: no grid");
  if (!h->has_search || h->n_beams == 0)
  {
    return fail(h, NDT2D_ERR_STATE, "ndt2d_match_launch: set_beams/set_search first");
  }
  if (th_count == 0 || th_stride == 0 || th_first >= h->n_th ||
      (th_count - 1) > (h->n_th - 1 - th_first) / th_stride)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_match_launch: bad theta range");
  }
  const size_t th_begin = th_first, th_end = th_first + th_count;
  NDT2D_TEST_MAYBE_FAIL(h, "ndt2d_match_launch");
  NDT2D_HIP(h, hipSetDevice(h->device));
  int rc = ensure(h, h->record, NDT2D_MATCH_RECORD_DOUBLES);
  if (rc != NDT2D_OK) return rc;
  if (h->bytes_job.n > 0)
  {
    // the map bytes of a list install that no scoreScan has carried yet
    hipError_t be = ndt2d::launch_sparse_bytes(h->grid, h->bytes_job, h->stream);
    if (be != hipSuccess) return fail_hip(h, be, "launch_sparse_bytes");
    h->bytes_job.n = 0;
  }

  ndt2d::MatchArgs a{};
  a.grid = h->grid;
  a.beams_xy = h->beams_ptr;
  a.n_beams = static_cast<uint32_t>(h->n_beams);
  a.dth = h->tables_ptr;
  a.cos_th = h->tables_ptr + h->n_th;
  a.sin_th = h->tables_ptr + 2 * h->n_th;
  a.dlin = h->tables_ptr + 3 * h->n_th;
  a.dlin_absmax = h->dlin_absmax;
  a.patch_span = h->patch_span;
  a.strip_span_long = h->strip_span_long;
  a.strip_span_short = h->strip_span_short;
  a.beam_rmax = h->beam_rmax;
  a.n_th = static_cast<uint32_t>(h->n_th);
  a.n_lin = static_cast<uint32_t>(h->n_lin);
  a.th_begin = static_cast<uint32_t>(th_begin);
  a.th_end = static_cast<uint32_t>(th_end);
  a.th_stride = static_cast<uint32_t>(th_stride);
  a.pose_x = h->pose_x;
  a.pose_y = h->pose_y;
  a.scores = d_scores;
  if (!(h->force_variant & (ndt2d::kVariantWave | ndt2d::kVariantLane)))
  {
    // a small lattice on a window wider than 256 cells: the small-lattice search wants the
    // grid's map bytes per block of cells (made once per grid and block size)
    const int k = ndt2d::match_small_block_log2(a, ndt2d::poses_lds_per_block());
    if (k > 0)
    {
      if (h->block_bytes_log2 != k)
      {
        rc = ensure(h, h->block_bytes, ndt2d::grid_block_bytes_size(h->grid, static_cast<uint32_t>(k)) / 8 + 2);
        if (rc != NDT2D_OK) return rc;
        hipError_t be = ndt2d::grid_block_bytes_launch(h->grid, static_cast<uint32_t>(k),
                                                       reinterpret_cast<uint8_t *>(h->block_bytes.ptr), h->stream);
        if (be != hipSuccess) return fail_hip(h, be, "grid_block_bytes_launch");
        h->block_bytes_log2 = k;
      }
      a.grid.block_bytes = reinterpret_cast<const uint8_t *>(h->block_bytes.ptr);
      a.grid.block_bytes_log2 = static_cast<uint32_t>(k);
    }
  }
  if (!h->tables_uploaded)
  {
    a.host_tables = h->stage_tables.ptr;
    if (ndt2d::match_needs_device_tables(a, !(h->force_variant & ndt2d::kVariantWave), h->force_variant))
    {
      rc = stage_submit(h, h->stage_tables, h->tables.ptr, 3 * h->n_th + h->n_lin);
      if (rc != NDT2D_OK) return rc;
      h->tables_uploaded = true;
      a.host_tables = nullptr;
    }
  }
  {
    // the head of the workspace holds counters the kernels expect to find at zero (they
    // leave them so): a fresh allocation is cleared once
    const size_t cap_before = h->ws_match.cap;
    rc = ensure(h, h->ws_match, ndt2d::match_workspace_doubles(a));
    if (rc != NDT2D_OK) return rc;
    // (a fresh allocation is cleared once: the counters at its head, and the `done` words of the
    // small-lattice search behind its record table)
    if (h->ws_match.cap != cap_before)
    {
      const size_t head_and_small = (ndt2d::match_workspace_head_doubles() +
                                     ndt2d::kSmallMaxItems * (NDT2D_MATCH_RECORD_DOUBLES + 1)) * sizeof(double);
      const size_t all = h->ws_match.cap * sizeof(double);
      NDT2D_HIP(h, hipMemsetAsync(h->ws_match.ptr, 0, head_and_small < all ? head_and_small : all, h->stream));
    }
  }

  // scratch for the rotated-beam table of the lane-per-candidate mapping
  double * outer = nullptr;
  if (!(h->force_variant & ndt2d::kVariantWave))
  {
    rc = ensure(h, h->outer, ndt2d::match_lane_outer_doubles(a));
    if (rc != NDT2D_OK) return rc;
    outer = h->outer.ptr;
  }

  rc = ensure_host_res(h);
  if (rc != NDT2D_OK) return rc;
  ndt2d::LaunchInfo info{"", 0};
  if (h->timing)
  {
    if (int trc = next_timing_slot(h); trc != NDT2D_OK) return trc;
  }
  h->match_seq = ++h->seq;
  h->match_pos = h->queued;   // (every mark so far is behind work queued before this search)
  // (the event pair brackets the search kernel itself)
  hipError_t e = ndt2d::launch_match(a, h->ws_match.ptr, outer, h->record.ptr, d_record,
                                     h->host_res_dev, h->match_seq, h->force_variant, h->stream,
                                     h->timing ? h->ev0 : nullptr, h->timing ? h->ev1 : nullptr, &info);
  if (e != hipSuccess) return fail_hip(h, e, "launch_match");
  h->timed = h->timing;
  h->last_kernels = info.n_kernels;
  h->last_variant = info.variant;
  h->match_pending = true;
  ++h->match_launches;
  h->last_candidates = static_cast<uint64_t>(th_end - th_begin) * h->n_lin * h->n_lin;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_match_fetch(ndt2d_handle h, ndt2d_match_result * out)
{
  NDT2D_C_TRY
  if (h == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  if (!h->match_pending) return fail(h, NDT2D_ERR_STATE, "ndt2d_match_fetch: nothing launched");
  NDT2D_HIP(h, hipSetDevice(h->device));
  // the final reduction wrote the record into host-coherent memory, then its flag
  // (whatever the wait says, the search is no longer pending: a call that failed leaves the
  // context ready for the next one)
  h->match_pending = false;
  ++h->match_fetches;
  int rc = wait_host_flag(h, ndt2d::kHostFlagSlot, h->match_seq, h->match_pos);
  if (rc != NDT2D_OK) return rc;
  double rec[NDT2D_MATCH_RECORD_DOUBLES];
  for (int k = 0; k < NDT2D_MATCH_RECORD_DOUBLES; ++k) rec[k] = h->host_res[k];
  out->best_score = rec[0];
  out->best_index = rec[1] < 0.0 ? NDT2D_NO_INDEX : static_cast<uint64_t>(rec[1]);
  // (index + 0.5: another candidate lies within the near-tie tolerance of the winner, ndt2d_device_fn.h merge_best)
  out->near_tie = (rec[1] >= 0.0 && rec[1] != std::floor(rec[1])) ? 1u : 0u;
  for (int k = 0; k < 10; ++k) out->acc[k] = rec[2 + k];
  out->n_candidates = h->last_candidates;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_match_near_best(ndt2d_handle h, size_t th_begin, size_t th_end, double rel, uint64_t * index_out,
                          size_t capacity, size_t * n_out, ndt2d_match_result * result_out)
{
  NDT2D_C_TRY
  if (h == nullptr || n_out == nullptr || (capacity > 0 && index_out == nullptr)) return NDT2D_ERR_INVALID;
  *n_out = 0;
  if (!(rel >= 0.0) || th_begin >= th_end || th_end > h->n_th || capacity > 65536)
  {
    return fail(h, NDT2D_ERR_INVALID, "ndt2d_match_near_best: bad argument");
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  const size_t n_scores = (th_end - th_begin) * h->n_lin * h->n_lin;
  int rc = ensure(h, h->tmp_scores, n_scores);
  if (rc != NDT2D_OK) return rc;
  rc = ensure(h, h->near_list, capacity + 2);
  if (rc != NDT2D_OK) return rc;
  rc = ndt2d_match_launch(h, th_begin, th_end, h->tmp_scores.ptr, nullptr);
  if (rc != NDT2D_OK) return rc;
  unsigned long long * list = reinterpret_cast<unsigned long long *>(h->near_list.ptr);
  std::vector<unsigned long long> host(capacity + 1);
  // one pass over all scores; should more candidates qualify than the list holds, further passes
  // over a shrinking index range until the list holds exactly the FIRST ones in visiting order
  // (bisection on the upper index; a plateau of equal scores is the only realistic way there)
  auto collect = [&](uint64_t hi) -> int {
    hipError_t e = ndt2d::launch_collect_near(h->tmp_scores.ptr, n_scores, hi, h->record.ptr, rel, 0.0, list,
                                              static_cast<uint32_t>(capacity), h->stream);
    if (e != hipSuccess) return fail_hip(h, e, "launch_collect_near");
    NDT2D_HIP(h, hipMemcpyAsync(host.data(), list, (capacity + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                h->stream));
    NDT2D_SYNC(h);
    return NDT2D_OK;
  };
  if ((rc = collect(n_scores)) != NDT2D_OK) return rc;
  const size_t total = static_cast<size_t>(host[0]);
  if (total > capacity && capacity > 0)
  {
    uint64_t lo = 0, hi = n_scores;   // count(lo) <= capacity < count(hi)
    while (hi - lo > 1)
    {
      const uint64_t mid = lo + (hi - lo) / 2;
      if ((rc = collect(mid)) != NDT2D_OK) return rc;
      if (host[0] <= capacity) lo = mid; else hi = mid;
    }
    if ((rc = collect(lo)) != NDT2D_OK) return rc;
  }
  ndt2d_match_result res;
  rc = ndt2d_match_fetch(h, &res);
  if (rc != NDT2D_OK) return rc;
  if (result_out != nullptr) *result_out = res;
  *n_out = total;
  const size_t kept = std::min<size_t>(static_cast<size_t>(host[0]), capacity);
  const uint64_t base = static_cast<uint64_t>(th_begin) * h->n_lin * h->n_lin;
  for (size_t k = 0; k < kept; ++k) index_out[k] = base + host[1 + k];
  std::sort(index_out, index_out + kept);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_match_status(ndt2d_handle h, uint64_t * n_launched, uint64_t * n_fetched)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (n_launched != nullptr) *n_launched = h->match_launches;
  if (n_fetched != nullptr) *n_fetched = h->match_fetches;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_match(ndt2d_handle h, size_t th_begin, size_t th_end, double * h_scores,
                ndt2d_match_result * out)
{
  NDT2D_C_TRY
  if (h == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  double * d_scores = nullptr;
  size_t n_scores = 0;
  if (h_scores != nullptr)
  {
    if (th_begin >= th_end || th_end > h->n_th)
    {
      return fail(h, NDT2D_ERR_INVALID, "ndt2d_match: bad theta range");
    }
    NDT2D_HIP(h, hipSetDevice(h->device));
    n_scores = (th_end - th_begin) * h->n_lin * h->n_lin;
    int rc = ensure(h, h->tmp_scores, n_scores);
    if (rc != NDT2D_OK) return rc;
    d_scores = h->tmp_scores.ptr;
  }
  int rc = ndt2d_match_launch(h, th_begin, th_end, d_scores, nullptr);
  if (rc != NDT2D_OK) return rc;
  if (h_scores != nullptr)
  {
    NDT2D_HIP(h, hipMemcpyAsync(h_scores, d_scores, n_scores * sizeof(double),
                                hipMemcpyDeviceToHost, h->stream));
    NDT2D_SYNC(h);
  }
  return ndt2d_match_fetch(h, out);
  NDT2D_C_CATCH(h)
}

}  // extern "C"
