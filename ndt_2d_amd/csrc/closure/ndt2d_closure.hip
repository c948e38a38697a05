// Batched loop-closure match: ONE scan against K candidate maps in one build launch, one search
// launch, one reduction launch and one read-back (gfx950 / MI355X).
//
// Reference: the loop-closure thread, src/ndt_mapper.cpp:619-671 -- per candidate scan `reset()`,
// `addScans(begin, end)` of one or two old scans, `matchScan(scan, ...)`.  Through the matcher
// layer that is K round trips of (fused build: three launches and a read-back) + (search launch,
// fetch), each search a loop-closure-size lattice that leaves most of the chip idle.  The K
// candidates are independent and their scans are resident (ndt2d_scanstore), so here:
//
//   closure_build_kernel   one workgroup of 1,024 threads per candidate map: the workgroup of the
//       fused small-map build (build_small_workgroup, ../build_small/ndt2d_build_small_fn.h --
//       keys, stable LDS radix sort, segment heads, addPoint in the reference's order,
//       Cell::compute: the same code, hence the same grid bit for bit) on the candidate's own
//       geometry, then -- behind a barrier -- what the search reads for the slot: a packed record
//       {mean, -0.5 information, n} per touched cell (the form record_exponent takes) and a
//       uint16 per grid cell, the index of the cell's record or 0xffff for a cell that cannot
//       score (untouched, or n < 5: src/ndt_model.cpp:107) and for entry ncell, "off the grid".
//       The workgroup clears the table itself.  No install kernels, nothing read back.
//   batch_search_kernel<C, POW2, ClosureSlots> (../batch/ndt2d_batch_search.h)  grid (theta
//       step, candidate map), a lane per (dx, dy): the block rotates the beams once for its theta
//       step (points_outer, src/scan_matcher_ndt.cpp:106-115, cos / sin from the host libm) into
//       LDS in pieces of kStageBeams, every lane adds points_inner = outer + (dx, dy) (:121-125)
//       through cell_index / record_exponent / exp_score of ndt2d_device_fn.h.  K x n_theta
//       blocks: 640 of seven waves for the plugin's defaults and K = 8, where one sequential
//       search is 80 x 7 tiles.
//   batch_reduce_kernel    one block per candidate map: the n_theta records of its blocks ->
//       {best_score, best_index (+0.5: near tie), acc[10]} with merge_best, fixed order.
//
// The bits of a raw score.  The small-lattice search (ndt2d_match_small.hip) -- the one every
// loop-closure-size lattice takes -- cuts a candidate's beams into look-up groups of four and
// deals the groups round-robin to C waves, C a function of the beam count alone; a score is
// ((p_0 + p_1) + p_2) + ... of the C in-order partial sums.  A lane here keeps the same C partial
// sums (template argument: registers) while it walks the beams once in order, and adds them the
// same way: the raw scores are the sequential path's bit for bit wherever that path runs the
// small-lattice search with its default plan.  (C = 1 is the plain running sum of the reference.)
// Terms are skipped by the rule of negligible_below(): bit-exact.
//
// Determinism.  Nothing depends on timing: a lane's sums are its own; a block reduces its lanes
// over the DPP network and its waves in wave order; the reducing block takes records r, r + 256,
// ... per thread, then the same two steps.  Stream order is the only ordering between the three
// launches and __syncthreads the only barrier inside them; no polls, no atomics.  Two calls
// give the same bits.
//
// LDS of the search block: kStageBeams x {ox, oy} = 16 KB, reused for one record per wave.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../build_small/ndt2d_build_small_fn.h"
#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_search.h"
#include "batch/ndt2d_batch_host.h"

namespace ndt2d
{

namespace
{

using namespace fused;

constexpr uint32_t kNoRecord = 0xffffu;

// One candidate map of a launch.  Offsets are into the closure's device arrays.
struct ClosureSlot
{
  GridDesc grid;          // geometry only
  uint32_t scan_first;    // first record of the candidate's scans in the scan table
  uint32_t n_scans;
  uint32_t n_points;
  uint32_t sort_passes;
  uint32_t world_off;     // points
  uint32_t list_off;      // touched-cell records
  uint32_t lookup_off;    // uint16 entries, a multiple of 8
  uint32_t pad;
};
static_assert(sizeof(ClosureSlot) % sizeof(double) == 0, "slots travel in a buffer of doubles");

struct ClosureBuildArgs
{
  const ClosureSlot * slots;
  const double * pool_xy;
  const SmallScan * scans;
  double * world_xy;
  double * cells6;        // [..][6] the fused build's raw list
  double * records;       // [..][6] packed {mean_x, mean_y, h00, h01, h11, n}
  uint32_t * index;       // [..] cell of every listed record
  uint16_t * lookup;
  uint32_t * n_touched;   // [slots]
  int eigen_form;
};

__global__ void __launch_bounds__(kThreads) closure_build_kernel(const ClosureBuildArgs a)
{
  extern __shared__ __align__(16) unsigned char lds[];
  const ClosureSlot & s = a.slots[blockIdx.x];
  const uint32_t t = threadIdx.x;

  SmallBuildArgs b;
  b.grid = s.grid;
  b.pool_xy = a.pool_xy;
  b.scans = a.scans + s.scan_first;
  b.n_scans = s.n_scans;
  b.n_points = s.n_points;
  b.sort_passes = s.sort_passes;
  b.world_xy = a.world_xy + 2 * static_cast<size_t>(s.world_off);
  b.list_cells6 = a.cells6 + 6 * static_cast<size_t>(s.list_off);
  b.list_index = a.index + s.list_off;
  b.n_touched_out = a.n_touched + blockIdx.x;
  b.eigen_form = a.eigen_form;
  const uint32_t n_touched = build_small_workgroup(b, lds);

  // the slot's cell -> record table, two entries a store (lookup_off is even; entry ncell is
  // "off the grid", the entry behind it padding)
  uint32_t * lookup2 = reinterpret_cast<uint32_t *>(a.lookup + s.lookup_off);
  const uint32_t n_pairs = (s.grid.ncell + 2u) / 2u;
  for (uint32_t i = t; i < n_pairs; i += kThreads) lookup2[i] = 0xffffffffu;
  __syncthreads();   // the list and the cleared table are the workgroup's to read from here
  uint16_t * lookup = a.lookup + s.lookup_off;
  double * records = a.records + 6 * static_cast<size_t>(s.list_off);
  for (uint32_t k = t; k < n_touched; k += kThreads)
  {
    const double2 * c6 = reinterpret_cast<const double2 *>(b.list_cells6 + static_cast<size_t>(k) * 6);
    const double2 m = c6[0], i0 = c6[1], i1 = c6[2];
    double2 * r = reinterpret_cast<double2 *>(records + static_cast<size_t>(k) * 6);
    // h = -0.5 * information (exact), as every install of the context packs it
    r[0] = m;
    r[1] = double2{-0.5 * i0.x, -0.5 * i0.y};
    r[2] = double2{-0.5 * i1.x, i1.y};
    if (!(i1.y < 5.0)) lookup[b.list_index[k]] = static_cast<uint16_t>(k);
  }
}

// A slot's map as the lane's walk reads it: the uint16 cell -> record table and the packed records.
struct SlotMap
{
  const uint16_t * lookup;
  const double * records;
  __device__ __forceinline__ bool find(uint32_t cell, uint32_t & rank) const
  {
    rank = lookup[cell];
    return rank != kNoRecord;
  }
  __device__ __forceinline__ const double2 * record(uint32_t rank) const
  {
    return reinterpret_cast<const double2 *>(records + static_cast<size_t>(rank) * 6);
  }
};

// SLOTS of the loop closure: slot y of the launch is candidate map y of the chunk; the scan, its
// pose and the theta steps' cos / sin are the call's.
struct ClosureSlots
{
  const ClosureSlot * slots;
  const uint16_t * lookup;
  const double * records;
  const double * beams_xy;   // [n_beams][2] robot frame
  const double * cos_th, * sin_th;
  uint32_t n_beams;
  double pose_x, pose_y;

  __device__ __forceinline__ BatchBlock<SlotMap> load(uint32_t y, uint32_t ith, uint32_t) const
  {
    const ClosureSlot & s = slots[y];
    return {s.grid, SlotMap{lookup + s.lookup_off, records + 6 * static_cast<size_t>(s.list_off)},
            beams_xy, n_beams, pose_x, pose_y, cos_th[ith], sin_th[ith], y};
  }
};

}  // namespace

}  // namespace ndt2d

// ---- the object and the C entry points ----

// (BatchHost's stage: [tables | beams | slots | scan table]; its events: before the build, behind
// it, behind the search)
struct ndt2d_closure : ndt2d::BatchHost
{
  ndt2d_scanstore * store = nullptr;
  size_t max_candidates = 0;
  // per chunk, grown on demand (bytes)
  void * d_world = nullptr, * d_cells6 = nullptr, * d_records = nullptr, * d_index = nullptr, * d_lookup = nullptr;
  size_t world_cap = 0, cells6_cap = 0, records_cap = 0, index_cap = 0, lookup_cap = 0;
  uint32_t * d_n_touched = nullptr;
  std::vector<ndt2d::ClosureSlot> slots;
};

namespace
{

using ndt2d::GridDesc;
using ndt2d::ClosureSlot;
using ndt2d::fused::SmallScan;
using ndt2d::batch_fail;
using ndt2d::grow_device;
using ndt2d::kRec;

void free_closure(ndt2d_closure * c)
{
  ndt2d::batch_release(c);
  if (c->d_world != nullptr) (void)hipFree(c->d_world);
  if (c->d_cells6 != nullptr) (void)hipFree(c->d_cells6);
  if (c->d_records != nullptr) (void)hipFree(c->d_records);
  if (c->d_index != nullptr) (void)hipFree(c->d_index);
  if (c->d_lookup != nullptr) (void)hipFree(c->d_lookup);
  if (c->d_n_touched != nullptr) (void)hipFree(c->d_n_touched);
  delete c;
}

struct SearchTables
{
  const double * beams_xy;
  size_t n_beams;
  double pose_x, pose_y;
  const double * dth, * cos_th, * sin_th;
  size_t n_th;
  const double * dlin;
  size_t n_lin;
};

// Candidates [k0, k1) of a call whose arguments have been checked: c->slots[k] holds their geometry
// and counts.  records_out / all_scores: the call's, whole.
int match_chunk(ndt2d_closure * c, size_t k0, size_t k1, const size_t * cand_offsets, const size_t * ids,
                const double * poses_xyt, const SearchTables & t, double * records_out, double * all_scores)
{
  ndt2d_scanstore * store = c->store;
  const size_t n_slots = k1 - k0;
  const size_t n_scans = cand_offsets[k1] - cand_offsets[k0];
  const size_t n_lattice = t.n_th * t.n_lin * t.n_lin;
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(c->h));

  // offsets of the slots into the chunk's arrays
  size_t n_world = 0, n_list = 0, n_lookup = 0;
  for (size_t k = k0; k < k1; ++k)
  {
    ClosureSlot & s = c->slots[k];
    s.scan_first = static_cast<uint32_t>(cand_offsets[k] - cand_offsets[k0]);
    s.world_off = static_cast<uint32_t>(n_world);
    s.list_off = static_cast<uint32_t>(n_list);
    s.lookup_off = static_cast<uint32_t>(n_lookup);
    n_world += s.n_points;
    n_list += std::max<size_t>(1, std::min<size_t>(s.n_points, s.grid.ncell));
    n_lookup += (static_cast<size_t>(s.grid.ncell) + 2 + 7) & ~size_t(7);
  }

  // [tables | beams | slots | scan table]
  const size_t n_tables = 3 * t.n_th + t.n_lin;
  const size_t off_beams = (n_tables + 1) & ~size_t(1), off_slots = off_beams + 2 * t.n_beams;   // (beams: 16-byte loads)
  const size_t off_scans = off_slots + n_slots * (sizeof(ClosureSlot) / sizeof(double));
  const size_t n_stage = off_scans + 5 * n_scans;
  NDT2D_BATCH_HIP(c, grow_device(&c->d_world, &c->world_cap, std::max<size_t>(1, n_world) * 2 * sizeof(double)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_cells6, &c->cells6_cap, n_list * 6 * sizeof(double)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_records, &c->records_cap, n_list * 6 * sizeof(double)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_index, &c->index_cap, n_list * sizeof(uint32_t)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_lookup, &c->lookup_cap, n_lookup * sizeof(uint16_t)));
  const size_t n_out = n_slots * (kRec + (all_scores != nullptr ? n_lattice : 0));
  NDT2D_BATCH_HIP(c, ndt2d::batch_grow(c, n_stage, n_slots, t.n_th, n_out));

  double * st = c->h_stage;
  std::memcpy(st, t.dth, t.n_th * sizeof(double));
  std::memcpy(st + t.n_th, t.cos_th, t.n_th * sizeof(double));
  std::memcpy(st + 2 * t.n_th, t.sin_th, t.n_th * sizeof(double));
  std::memcpy(st + 3 * t.n_th, t.dlin, t.n_lin * sizeof(double));
  std::memcpy(st + off_beams, t.beams_xy, 2 * t.n_beams * sizeof(double));
  std::memcpy(st + off_slots, c->slots.data() + k0, n_slots * sizeof(ClosureSlot));
  SmallScan * table = reinterpret_cast<SmallScan *>(st + off_scans);
  for (size_t k = k0; k < k1; ++k)
  {
    uint32_t first = 0;
    for (size_t j = cand_offsets[k]; j < cand_offsets[k + 1]; ++j)
    {
      SmallScan & sc = table[j - cand_offsets[k0]];
      sc.x = poses_xyt[3 * j];
      sc.y = poses_xyt[3 * j + 1];
      ndt2d_cos_sin(poses_xyt[3 * j + 2], &sc.c, &sc.s);   // (src/ndt_model.cpp:135-136, host libm)
      sc.pool_offset = store->offset[ids[j]];
      sc.first = first;
      first += store->count[ids[j]];
    }
  }

  NDT2D_BATCH_HIP(c, hipMemcpyAsync(c->d_stage, st, n_stage * sizeof(double), hipMemcpyHostToDevice, stream));
  c->timed = false;
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[0], stream));

  ndt2d::ClosureBuildArgs b{};
  b.slots = reinterpret_cast<const ClosureSlot *>(c->d_stage + off_slots);
  b.pool_xy = store->pool;
  b.scans = reinterpret_cast<const SmallScan *>(c->d_stage + off_scans);
  b.world_xy = static_cast<double *>(c->d_world);
  b.cells6 = static_cast<double *>(c->d_cells6);
  b.records = static_cast<double *>(c->d_records);
  b.index = static_cast<uint32_t *>(c->d_index);
  b.lookup = static_cast<uint16_t *>(c->d_lookup);
  b.n_touched = c->d_n_touched;
  b.eigen_form = store->eigen_form;
  // (no static LDS in front of the workgroup's arrays: prepare_absolute_lds_kernel, ndt2d_kernels.h)
  NDT2D_BATCH_HIP(c, ndt2d::prepare_absolute_lds_kernel(reinterpret_cast<const void *>(ndt2d::closure_build_kernel),
                                                          ndt2d::fused::kLdsBytes));
  hipLaunchKernelGGL(ndt2d::closure_build_kernel, dim3(static_cast<uint32_t>(n_slots)), dim3(ndt2d::fused::kThreads),
                     ndt2d::fused::kLdsBytes, stream, b);
  NDT2D_BATCH_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[1], stream));

  ndt2d::BatchSearchArgs<ndt2d::ClosureSlots> a{};
  a.slots.slots = b.slots;
  a.slots.lookup = b.lookup;
  a.slots.records = b.records;
  a.slots.beams_xy = c->d_stage + off_beams;
  a.slots.cos_th = c->d_stage + t.n_th;
  a.slots.sin_th = c->d_stage + 2 * t.n_th;
  a.slots.n_beams = static_cast<uint32_t>(t.n_beams);
  a.slots.pose_x = t.pose_x;
  a.slots.pose_y = t.pose_y;
  a.dth = c->d_stage;
  a.dlin = c->d_stage + 3 * t.n_th;
  a.n_th = static_cast<uint32_t>(t.n_th);
  a.n_lin = static_cast<uint32_t>(t.n_lin);
  a.scores = all_scores != nullptr ? c->d_out + n_slots * kRec : nullptr;
  a.partials = static_cast<double *>(c->d_partials);
  const dim3 grid(a.n_th, static_cast<uint32_t>(n_slots));
  ndt2d::launch_batch_search(ndt2d::sum_chunks(a.slots.n_beams), c->slots[k0].grid.pow2 != 0, grid,
                             dim3(ndt2d::batch_search_threads(t.n_lin * t.n_lin)), stream, a);
  NDT2D_BATCH_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[2], stream));
  return ndt2d::batch_reduce_and_fetch(c, stream, k0, n_slots, a.n_th, n_lattice, -1, records_out, all_scores);
}

}  // namespace

extern "C" {

int ndt2d_closure_create(ndt2d_handle h, ndt2d_scanstore * store, size_t max_candidates, ndt2d_closure ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || store == nullptr || store->h != h || max_candidates == 0 || max_candidates > 4096)
  {
    return NDT2D_ERR_INVALID;
  }
  ndt2d_closure * c = new ndt2d_closure();
  c->h = h;
  c->store = store;
  c->device = ndt2d_device_id(h);
  c->max_candidates = max_candidates;
  hipError_t e = hipSetDevice(c->device);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&c->d_n_touched), max_candidates * sizeof(uint32_t));
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    free_closure(c);
    return NDT2D_ERR_HIP;
  }
  *out = c;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_closure_destroy(ndt2d_closure * c)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::batch_drain(c);
  free_closure(c);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_closure_last_error(ndt2d_closure * c)
{
  return c != nullptr ? c->err.c_str() : "null closure";
}

int ndt2d_closure_set_timing(ndt2d_closure * c, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(c, enabled);
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_last_ms(ndt2d_closure * c, float * build_ms, float * search_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(c, "closure", build_ms, search_ms);
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_match(ndt2d_closure * c, size_t n_candidates, const size_t * cand_offsets, const size_t * ids,
                        const double * poses_xyt, double ndt_resolution, double range_max, const double * beams_xy,
                        size_t n_beams, double pose_x, double pose_y, const double * dth, const double * cos_th,
                        const double * sin_th, size_t n_th, const double * dlin, size_t n_lin, double * records_out,
                        double * all_scores)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (n_candidates == 0) return NDT2D_OK;
  if (cand_offsets == nullptr || ids == nullptr || poses_xyt == nullptr || records_out == nullptr ||
      beams_xy == nullptr || dth == nullptr || cos_th == nullptr || sin_th == nullptr || dlin == nullptr)
  {
    return batch_fail(c, NDT2D_ERR_INVALID, "ndt2d_closure_match: null argument");
  }
  if (!(ndt_resolution > 0.0) || !std::isfinite(ndt_resolution) || !std::isfinite(range_max))
  {
    return batch_fail(c, NDT2D_ERR_INVALID, "ndt2d_closure_match: bad resolution or range_max");
  }
  if (n_beams == 0 || n_beams >= (1u << 24) || n_th == 0 || n_th >= (1u << 20) || n_lin == 0 || n_lin > 4096 ||
      n_candidates >= (1u << 24) || !std::isfinite(pose_x) || !std::isfinite(pose_y))
  {
    return batch_fail(c, NDT2D_ERR_INVALID, "ndt2d_closure_match: bad search (beams, lattice or pose)");
  }
  const ndt2d_scanstore * store = c->store;
  // every candidate is checked before anything is launched
  c->slots.assign(n_candidates, ClosureSlot{});
  for (size_t k = 0; k < n_candidates; ++k)
  {
    const std::string who = "ndt2d_closure_match: candidate " + std::to_string(k);
    if (cand_offsets[k + 1] < cand_offsets[k] || cand_offsets[k + 1] - cand_offsets[0] >= (1u << 28))
    {
      return batch_fail(c, NDT2D_ERR_INVALID, who + ": offsets must not decrease");
    }
    const size_t j0 = cand_offsets[k], j1 = cand_offsets[k + 1];
    if (j1 == j0) return batch_fail(c, NDT2D_ERR_INVALID, who + " has no scans");
    size_t n_points = 0;
    for (size_t j = j0; j < j1; ++j)
    {
      if (ids[j] >= store->count.size())
      {
        return batch_fail(c, NDT2D_ERR_INVALID, who + ": unknown scan id " + std::to_string(ids[j]));
      }
      if (!std::isfinite(poses_xyt[3 * j]) || !std::isfinite(poses_xyt[3 * j + 1]) || !std::isfinite(poses_xyt[3 * j + 2]))
      {
        return batch_fail(c, NDT2D_ERR_INVALID, who + ": a scan pose is not finite");
      }
      n_points += store->count[ids[j]];
    }
    ClosureSlot & s = c->slots[k];
    if (!ndt2d::fused::addscans_geometry(ndt_resolution, range_max, poses_xyt + 3 * j0, j1 - j0, &s.grid))
    {
      return batch_fail(c, NDT2D_ERR_INVALID, who + ": degenerate grid extent");
    }
    if (!ndt2d::fused::small_map_fits(s.grid, n_points) || s.grid.ncell == 0)
    {
      return batch_fail(c, NDT2D_ERR_INVALID, who + ": the map exceeds the fused build's limits (" + std::to_string(n_points) +
                                           " points of at most " + std::to_string(ndt2d::fused::kFusedMaxPoints) + ", " +
                                           std::to_string(s.grid.ncell) + " cells of fewer than 65535)");
    }
    s.n_scans = static_cast<uint32_t>(j1 - j0);
    s.n_points = static_cast<uint32_t>(n_points);
    s.sort_passes = ndt2d::fused::sort_passes_for(s.grid.ncell);
  }
  NDT2D_BATCH_HIP(c, hipSetDevice(c->device));
  const SearchTables t{beams_xy, n_beams, pose_x, pose_y, dth, cos_th, sin_th, n_th, dlin, n_lin};
  // more candidates than slots: in chunks
  for (size_t k0 = 0; k0 < n_candidates; k0 += c->max_candidates)
  {
    const size_t k1 = std::min(n_candidates, k0 + c->max_candidates);
    const int rc = match_chunk(c, k0, k1, cand_offsets, ids, poses_xyt, t, records_out, all_scores);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

}  // extern "C"
