// Batched loop-closure match: ONE scan against K candidate maps in one build launch, one search
// launch, one reduction launch and one read-back (gfx950 / MI355X) -- and the Newton NDT
// registration of K (scan, pose) jobs on such maps in one build launch and one refinement launch,
// and their match verification in one build launch and one verify launch.
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
//   verify_kernel<POW2, CELLS, SlotSource> (../verify/ndt2d_verify_kernel.h)
//       ndt2d_closure_verify: the match verification of K (scan, pose) jobs, each on its
//       candidate's own map, behind the same build launch in ONE launch with a workgroup of 256
//       threads per job; the plan is ndt2d_closure_jobs.h's with the jobs' beams as weights.  A
//       job's record and per-beam results have the bits ndt2d_verify_run gives on the grid
//       ndt2d_scanstore_build installs for the candidate.
//
//   refine_kernel<POW2, CELLS, SlotSource> (../refine/ndt2d_refine_kernel.h)
//       ndt2d_closure_refine: the Newton NDT registration of K jobs, each on its
//       candidate's own map -- behind the same build launch, ONE launch with a workgroup of 256
//       threads per job, which reads its slot's table and records through SlotSource and nothing of
//       the grid installed in the context.  Which candidates a launch builds and which jobs run on
//       them is ndt2d_closure_jobs.h's plan; a job's record has the bits ndt2d_refine_run gives on
//       the grid ndt2d_scanstore_build installs for the candidate (the build is the fused build's
//       workgroup, the kernel has one text).
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
//
// The host side.  What keeps device indices in range exists once: place_chunk_slots (the slots'
// offsets into the launch's arrays, from slot_extent of ndt2d_closure_jobs.h, and the arrays'
// growth) and fill_scan_table serve the three entry points -- the match's chunk [k0, k1) is the
// plan whose candidates are k0 .. k1 - 1 -- and job_chunk is the one path of a chunk of jobs: the
// sent scans, the stage [beams | slots | scan table | jobs | cos / sin], the upload, the build, the
// launch, the read-back; the refinement and the verification give it their job record, their launch
// and the scatter of what came back.  check_job_call is what both refuse, in one order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../build_small/ndt2d_build_small_fn.h"
#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_search.h"
#include "batch/ndt2d_batch_host.h"
#include "batch/ndt2d_refine_jobs.h"
#include "closure/ndt2d_closure_jobs.h"
#include "refine/ndt2d_refine_kernel.h"
#include "verify/ndt2d_verify_kernel.h"

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

// SOURCE of the Newton registration (../refine/ndt2d_refine_kernel.h): a job's map is the slot its
// record names -- the slot's own geometry, table and records.  Nothing of the context's installed
// grid is read: the slots' GridDesc hold geometry only.  Entry ncell of a slot's table is 0xffff
// (closure_build_kernel), so an off-grid point or neighbour finds no record.
struct SlotSource
{
  const ClosureSlot * slots;
  const uint16_t * lookup;
  const double * records;
  __device__ __forceinline__ const GridDesc & grid(uint32_t slot) const { return slots[slot].grid; }
  __device__ __forceinline__ SlotMap map(uint32_t slot) const
  {
    const ClosureSlot & s = slots[slot];
    return SlotMap{lookup + s.lookup_off, records + 6 * static_cast<size_t>(s.list_off)};
  }
};

using SlotRefineArgs = RefineArgs<SlotSource>;

// CELLS: the neighbourhood of a point, 1 or 9.  pow2: of every slot (they share the call's resolution).
template <uint32_t CELLS>
void launch_slot_refine(bool pow2, dim3 blocks, dim3 threads, hipStream_t stream, const SlotRefineArgs & a)
{
  if (pow2) hipLaunchKernelGGL((refine_kernel<true, CELLS, SlotSource>), blocks, threads, 0, stream, a);
  else hipLaunchKernelGGL((refine_kernel<false, CELLS, SlotSource>), blocks, threads, 0, stream, a);
}

using SlotVerifyArgs = VerifyArgs<SlotSource>;

// The match verification (../verify/ndt2d_verify_kernel.h) on the slots: find() is "can score" for the
// neighbourhood and for the ray alike (a table entry exists only for cells of n >= 5), the clip, the
// line and the origin cell run on the slot's own geometry.
template <uint32_t CELLS>
void launch_slot_verify(bool pow2, dim3 blocks, dim3 threads, hipStream_t stream, const SlotVerifyArgs & a)
{
  if (pow2) hipLaunchKernelGGL((verify_kernel<true, CELLS, SlotSource>), blocks, threads, 0, stream, a);
  else hipLaunchKernelGGL((verify_kernel<false, CELLS, SlotSource>), blocks, threads, 0, stream, a);
}

}  // namespace

}  // namespace ndt2d

// ---- the object and the C entry points ----

// (BatchHost's stage: [tables | beams | slots | scan table]; its events: before the build, behind
// it, behind the search -- or the refinement, or the verification)
struct ndt2d_closure : ndt2d::BatchHost
{
  ndt2d_scanstore * store = nullptr;
  size_t max_candidates = 0;
  // per chunk, grown on demand (bytes)
  void * d_world = nullptr, * d_cells6 = nullptr, * d_records = nullptr, * d_index = nullptr, * d_lookup = nullptr;
  size_t world_cap = 0, cells6_cap = 0, records_cap = 0, index_cap = 0, lookup_cap = 0;
  uint32_t * d_n_touched = nullptr;
  std::vector<ndt2d::ClosureSlot> slots;         // candidate of the call -> its geometry and counts
  std::vector<ndt2d::ClosureSlot> chunk_slots;   // slot of the launch, placed
  std::vector<uint32_t> match_candidates;        // ndt2d_closure_match: slot of the launch -> candidate
  // ndt2d_closure_refine
  uint32_t cells = 1;                 // the neighbourhood of a point: 1 (its own cell) or 9 (the 3 x 3 round it)
  std::vector<uint64_t> scan_first;   // scan -> its first beam within the chunk's beams (or: not sent)
  std::vector<uint32_t> sent;         // the chunk's scans in upload order
  // ndt2d_closure_verify
  ndt2d::VerifySettings verify;       // ndt2d_verify's, with its defaults
  std::vector<size_t> job_first;     // job of the call -> its first beam within the caller's per-beam arrays
  std::vector<size_t> job_beams;      // job of the call -> the beams of its scan (its weight in the plan)
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

// What every entry point refuses about a candidate (the message names it); c->slots[k]: candidate
// k's geometry and counts.
int check_candidates(ndt2d_closure * c, const char * entry, size_t n_candidates, const size_t * cand_offsets,
                     const size_t * ids, const double * poses_xyt, double ndt_resolution, double range_max)
{
  const ndt2d_scanstore * store = c->store;
  c->slots.assign(n_candidates, ClosureSlot{});
  for (size_t k = 0; k < n_candidates; ++k)
  {
    const std::string who = std::string(entry) + ": candidate " + std::to_string(k);
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
  return NDT2D_OK;
}

// The build launch of a chunk whose stage has been uploaded: a workgroup per slot.  *b: what was
// launched (the search and the refinement read its records and table).
int launch_build(ndt2d_closure * c, hipStream_t stream, size_t n_slots, const ClosureSlot * d_slots,
                 const SmallScan * d_scans, ndt2d::ClosureBuildArgs * b)
{
  const ndt2d_scanstore * store = c->store;
  b->slots = d_slots;
  b->pool_xy = store->pool;
  b->scans = d_scans;
  b->world_xy = static_cast<double *>(c->d_world);
  b->cells6 = static_cast<double *>(c->d_cells6);
  b->records = static_cast<double *>(c->d_records);
  b->index = static_cast<uint32_t *>(c->d_index);
  b->lookup = static_cast<uint16_t *>(c->d_lookup);
  b->n_touched = c->d_n_touched;
  b->eigen_form = store->eigen_form;
  // (no static LDS in front of the workgroup's arrays: prepare_absolute_lds_kernel, ndt2d_kernels.h)
  NDT2D_BATCH_HIP(c, ndt2d::prepare_absolute_lds_kernel(reinterpret_cast<const void *>(ndt2d::closure_build_kernel),
                                                          ndt2d::fused::kLdsBytes));
  hipLaunchKernelGGL(ndt2d::closure_build_kernel, dim3(static_cast<uint32_t>(n_slots)), dim3(ndt2d::fused::kThreads),
                     ndt2d::fused::kLdsBytes, stream, *b);
  NDT2D_BATCH_HIP(c, hipGetLastError());
  return NDT2D_OK;
}

// The candidates of a call: candidate k is scans ids[cand_offsets[k] .. cand_offsets[k + 1]) at poses_xyt.
struct CandidateMaps
{
  const size_t * cand_offsets;
  const size_t * ids;
  const double * poses_xyt;
};

// The slots of one launch -- candidates[y] of the call on slot y: a chunk of a job plan
// (ndt2d_closure_jobs.h), or the match's k0 .. k1 - 1 -- into c->chunk_slots: c->slots[k] (candidate
// k's geometry and counts, check_candidates) with its offsets into the launch's arrays, the running
// sums of slot_extent, and the arrays grown to hold them.  *n_map_scans: the scans of the slots' maps.
int place_chunk_slots(ndt2d_closure * c, const std::vector<uint32_t> & candidates, size_t * n_map_scans)
{
  const size_t n_slots = candidates.size();
  c->chunk_slots.resize(n_slots);
  size_t n_world = 0, n_list = 0, n_lookup = 0, n_scans = 0;
  for (size_t y = 0; y < n_slots; ++y)
  {
    ClosureSlot & s = c->chunk_slots[y];
    s = c->slots[candidates[y]];
    const ndt2d::SlotExtent e = ndt2d::slot_extent(s.n_points, s.grid.ncell);
    s.scan_first = static_cast<uint32_t>(n_scans);
    s.world_off = static_cast<uint32_t>(n_world);
    s.list_off = static_cast<uint32_t>(n_list);
    s.lookup_off = static_cast<uint32_t>(n_lookup);
    n_scans += s.n_scans;
    n_world += s.n_points;
    n_list += e.list;
    n_lookup += e.lookup;
  }
  *n_map_scans = n_scans;
  NDT2D_BATCH_HIP(c, grow_device(&c->d_world, &c->world_cap, std::max<size_t>(1, n_world) * 2 * sizeof(double)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_cells6, &c->cells6_cap, n_list * 6 * sizeof(double)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_records, &c->records_cap, n_list * 6 * sizeof(double)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_index, &c->index_cap, n_list * sizeof(uint32_t)));
  NDT2D_BATCH_HIP(c, grow_device(&c->d_lookup, &c->lookup_cap, n_lookup * sizeof(uint16_t)));
  return NDT2D_OK;
}

// The scan table of the slots' maps (c->chunk_slots: place_chunk_slots), as the build reads it.
void fill_scan_table(const ndt2d_closure * c, const std::vector<uint32_t> & candidates, const CandidateMaps & m, SmallScan * table)
{
  const ndt2d_scanstore * store = c->store;
  for (size_t y = 0; y < candidates.size(); ++y)
  {
    const size_t k = candidates[y];
    uint32_t first = 0;
    for (size_t j = m.cand_offsets[k]; j < m.cand_offsets[k + 1]; ++j)
    {
      SmallScan & sc = table[c->chunk_slots[y].scan_first + (j - m.cand_offsets[k])];
      sc.x = m.poses_xyt[3 * j];
      sc.y = m.poses_xyt[3 * j + 1];
      ndt2d_cos_sin(m.poses_xyt[3 * j + 2], &sc.c, &sc.s);   // (src/ndt_model.cpp:135-136, host libm)
      sc.pool_offset = store->offset[m.ids[j]];
      sc.first = first;
      first += store->count[m.ids[j]];
    }
  }
}

// Candidates [k0, k1) of a call whose arguments have been checked: c->slots[k] holds their geometry
// and counts.  records_out / all_scores: the call's, whole.
int match_chunk(ndt2d_closure * c, size_t k0, size_t k1, const CandidateMaps & m, const SearchTables & t, double * records_out,
                double * all_scores)
{
  const size_t n_slots = k1 - k0;
  const size_t n_lattice = t.n_th * t.n_lin * t.n_lin;
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(c->h));

  // the chunk as a plan: slot y is candidate k0 + y
  c->match_candidates.resize(n_slots);
  for (size_t y = 0; y < n_slots; ++y) c->match_candidates[y] = static_cast<uint32_t>(k0 + y);
  size_t n_scans = 0;
  const int prc = place_chunk_slots(c, c->match_candidates, &n_scans);
  if (prc != NDT2D_OK) return prc;

  // [tables | beams | slots | scan table]
  const size_t n_tables = 3 * t.n_th + t.n_lin;
  const size_t off_beams = (n_tables + 1) & ~size_t(1), off_slots = off_beams + 2 * t.n_beams;   // (beams: 16-byte loads)
  const size_t off_scans = off_slots + n_slots * (sizeof(ClosureSlot) / sizeof(double));
  const size_t n_stage = off_scans + 5 * n_scans;
  const size_t n_out = n_slots * (kRec + (all_scores != nullptr ? n_lattice : 0));
  NDT2D_BATCH_HIP(c, ndt2d::batch_grow(c, n_stage, n_slots, t.n_th, n_out));

  double * st = c->h_stage;
  std::memcpy(st, t.dth, t.n_th * sizeof(double));
  std::memcpy(st + t.n_th, t.cos_th, t.n_th * sizeof(double));
  std::memcpy(st + 2 * t.n_th, t.sin_th, t.n_th * sizeof(double));
  std::memcpy(st + 3 * t.n_th, t.dlin, t.n_lin * sizeof(double));
  std::memcpy(st + off_beams, t.beams_xy, 2 * t.n_beams * sizeof(double));
  std::memcpy(st + off_slots, c->chunk_slots.data(), n_slots * sizeof(ClosureSlot));
  fill_scan_table(c, c->match_candidates, m, reinterpret_cast<SmallScan *>(st + off_scans));

  NDT2D_BATCH_HIP(c, hipMemcpyAsync(c->d_stage, st, n_stage * sizeof(double), hipMemcpyHostToDevice, stream));
  c->timed = false;
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[0], stream));

  ndt2d::ClosureBuildArgs b{};
  const int brc = launch_build(c, stream, n_slots, reinterpret_cast<const ClosureSlot *>(c->d_stage + off_slots),
                               reinterpret_cast<const SmallScan *>(c->d_stage + off_scans), &b);
  if (brc != NDT2D_OK) return brc;
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
  ndt2d::launch_batch_search(ndt2d::sum_chunks(a.slots.n_beams), c->chunk_slots[0].grid.pow2 != 0, grid,
                             dim3(ndt2d::batch_search_threads(t.n_lin * t.n_lin)), stream, a);
  NDT2D_BATCH_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[2], stream));
  return ndt2d::batch_reduce_and_fetch(c, stream, k0, n_slots, a.n_th, n_lattice, -1, records_out, all_scores);
}

// What a chunk's launch reads, on the device: the built slots, the jobs' records, the cos / sin
// pairs of their headings and the chunk's beams.
struct ChunkOnDevice
{
  ndt2d::SlotSource source;
  const double * jobs, * trig, * beams_xy;
  dim3 blocks;   // a block per job
  bool pow2;     // of every slot
  hipStream_t stream;
};

// One chunk of a job plan -- the refinement's or the verification's -- of a call whose arguments
// have been checked (c->slots[k]: candidate k's geometry and counts): one upload, [beams | slots |
// scan table | jobs | cos / sin pairs], the build of the chunk's candidates, the launch on its jobs
// -- a block each, on the slot its record names -- and one read-back of n_back doubles into
// c->h_out, waited for.  t: the call's jobs and scans (jobs_xyt, scan_of, beams_xy, beam_offsets,
// n_scans).  write_job(b, k, first, to): the record (job_doubles doubles) of block b, job k of the
// call, whose scan's first beam within the chunk's beams is `first`.  launch(d): the kernel on
// d.stream.  The events: before the build, behind it, behind the launch.
template <class CALL, class WRITE_JOB, class LAUNCH>
int job_chunk(ndt2d_closure * c, const ndt2d::ClosureJobChunk & plan, const CandidateMaps & m, const CALL & t, size_t job_doubles,
              size_t n_back, WRITE_JOB write_job, LAUNCH launch)
{
  const size_t n_slots = plan.candidates.size(), n_jobs = plan.jobs.size();
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(c->h));

  size_t n_map_scans = 0;
  const int prc = place_chunk_slots(c, plan.candidates, &n_map_scans);
  if (prc != NDT2D_OK) return prc;

  // the scans this chunk's jobs name, each once, in the order the jobs first name them
  const size_t n_beams = ndt2d::refine_jobs::plan_sent_scans(
    n_jobs, [&](size_t b) { return static_cast<size_t>(plan.jobs[b]); }, [&](size_t k) { return t.scan_of(k); }, t.beam_offsets,
    t.n_scans, c->scan_first, c->sent);

  const size_t off_slots = 2 * n_beams;   // (beams in front: 16-byte loads)
  const size_t off_scans = off_slots + n_slots * (sizeof(ClosureSlot) / sizeof(double));
  const size_t off_jobs = off_scans + 5 * n_map_scans;
  const size_t off_trig = off_jobs + n_jobs * job_doubles;
  const size_t n_stage = off_trig + 2 * n_jobs;
  NDT2D_BATCH_HIP(c, ndt2d::grow_pair(&c->h_stage, &c->d_stage, &c->stage_cap, n_stage));
  NDT2D_BATCH_HIP(c, ndt2d::grow_pair(&c->h_out, &c->d_out, &c->out_cap, n_back));

  double * st = c->h_stage;
  ndt2d::refine_jobs::copy_sent_scans(c->sent, c->scan_first, t.beams_xy, t.beam_offsets, st);
  std::memcpy(st + off_slots, c->chunk_slots.data(), n_slots * sizeof(ClosureSlot));
  fill_scan_table(c, plan.candidates, m, reinterpret_cast<SmallScan *>(st + off_scans));
  for (size_t b = 0; b < n_jobs; ++b)
  {
    const size_t k = plan.jobs[b];
    write_job(b, k, c->scan_first[t.scan_of(k)], st + off_jobs + b * job_doubles);
    // cos / sin of the job's heading from the host libm, as everywhere in this library
    ndt2d_cos_sin(t.jobs_xyt[3 * k + 2], st + off_trig + 2 * b, st + off_trig + 2 * b + 1);
  }
  NDT2D_BATCH_HIP(c, hipMemcpyAsync(c->d_stage, st, n_stage * sizeof(double), hipMemcpyHostToDevice, stream));
  c->timed = false;
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[0], stream));

  ndt2d::ClosureBuildArgs b{};
  const int brc = launch_build(c, stream, n_slots, reinterpret_cast<const ClosureSlot *>(c->d_stage + off_slots),
                               reinterpret_cast<const SmallScan *>(c->d_stage + off_scans), &b);
  if (brc != NDT2D_OK) return brc;
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[1], stream));

  launch(ChunkOnDevice{{b.slots, b.lookup, b.records}, c->d_stage + off_jobs, c->d_stage + off_trig, c->d_stage,
                       dim3(static_cast<uint32_t>(n_jobs)), c->chunk_slots[0].grid.pow2 != 0, stream});
  NDT2D_BATCH_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_BATCH_HIP(c, hipEventRecord(c->ev[2], stream));
  NDT2D_BATCH_HIP(c, hipMemcpyAsync(c->h_out, c->d_out, n_back * sizeof(double), hipMemcpyDeviceToHost, stream));
  NDT2D_BATCH_HIP(c, hipStreamSynchronize(stream));
  c->timed = c->timing;
  return NDT2D_OK;
}

struct RefineCall : ndt2d::refine_jobs::JobList
{
  ndt2d::refine::Rules rules;
};

// One chunk of ndt2d_closure_refine's plan.  records_out: the call's, whole.
int refine_chunk(ndt2d_closure * c, const ndt2d::ClosureJobChunk & plan, const CandidateMaps & m, const RefineCall & t,
                 double * records_out)
{
  using ndt2d::RefineJob;
  using ndt2d::kRefineRec;
  const size_t n_jobs = plan.jobs.size();
  const int rc = job_chunk(
    c, plan, m, t, ndt2d::kRefineJobDoubles, n_jobs * kRefineRec,
    [&](size_t b, size_t k, uint64_t first, double * to) {
      const double * p = t.jobs_xyt + 3 * k;
      *reinterpret_cast<RefineJob *>(to) = RefineJob{p[0], p[1], p[2], static_cast<uint32_t>(t.beams_of(k)), plan.job_slot[b], first};
    },
    [&](const ChunkOnDevice & d) {
      ndt2d::SlotRefineArgs a{};
      a.source = d.source;
      a.jobs = reinterpret_cast<const RefineJob *>(d.jobs);
      a.trig = d.trig;
      a.beams_xy = d.beams_xy;
      a.rules = t.rules;
      a.records = c->d_out;
      if (c->cells == 9) ndt2d::launch_slot_refine<9>(d.pow2, d.blocks, dim3(ndt2d::kRefineThreads), d.stream, a);
      else ndt2d::launch_slot_refine<1>(d.pow2, d.blocks, dim3(ndt2d::kRefineThreads), d.stream, a);
    });
  if (rc != NDT2D_OK) return rc;
  for (size_t bj = 0; bj < n_jobs; ++bj)
  {
    std::memcpy(records_out + static_cast<size_t>(plan.jobs[bj]) * kRefineRec, c->h_out + bj * kRefineRec, kRefineRec * sizeof(double));
  }
  return NDT2D_OK;
}

// One chunk of ndt2d_closure_verify's plan.  v: the jobs, the scans and the outputs, as
// ndt2d_verify_run takes them.  The chunk's per-beam results lie job after job in the plan's order;
// c->job_first[k]: where job k's go in the caller's arrays.
int verify_chunk(ndt2d_closure * c, const ndt2d::ClosureJobChunk & plan, const CandidateMaps & m, const ndt2d::VerifyCall & v)
{
  using ndt2d::VerifyJob;
  constexpr size_t kVerRec = ndt2d::kVerifyRec;
  const size_t n_jobs = plan.jobs.size();
  size_t n_out = 0;
  for (size_t b = 0; b < n_jobs; ++b) n_out += v.beams_of(plan.jobs[b]);
  const ndt2d::VerifyOutLayout out = ndt2d::verify_out_layout(n_jobs, n_out, v);
  size_t out_first = 0;
  const int rc = job_chunk(
    c, plan, m, v, ndt2d::kVerifyJobDoubles, out.total,
    [&](size_t b, size_t k, uint64_t first, double * to) {
      const double * p = v.jobs_xyt + 3 * k;
      *reinterpret_cast<VerifyJob *>(to) = VerifyJob{p[0], p[1], static_cast<uint32_t>(v.beams_of(k)), plan.job_slot[b], first, out_first};
      out_first += v.beams_of(k);
    },
    [&](const ChunkOnDevice & d) {
      ndt2d::SlotVerifyArgs a{};
      a.source = d.source;
      a.jobs = reinterpret_cast<const VerifyJob *>(d.jobs);
      a.trig = d.trig;
      a.beams_xy = d.beams_xy;
      a.rules = c->verify.rules();
      a.records = reinterpret_cast<uint32_t *>(c->d_out);
      a.beam_m2 = v.beam_m2_out != nullptr ? c->d_out + out.m2 : nullptr;
      a.beam_cells = v.beam_cells_out != nullptr ? reinterpret_cast<uint32_t *>(c->d_out + out.cells) : nullptr;
      a.beam_class = v.beam_class_out != nullptr ? reinterpret_cast<uint8_t *>(c->d_out + out.classes) : nullptr;
      if (c->verify.cells == 9) ndt2d::launch_slot_verify<9>(d.pow2, d.blocks, dim3(ndt2d::kVerifyThreads), d.stream, a);
      else ndt2d::launch_slot_verify<1>(d.pow2, d.blocks, dim3(ndt2d::kVerifyThreads), d.stream, a);
    });
  if (rc != NDT2D_OK) return rc;
  const uint32_t * records = reinterpret_cast<const uint32_t *>(c->h_out);
  const uint8_t * classes = reinterpret_cast<const uint8_t *>(c->h_out + out.classes);
  size_t at = 0;
  for (size_t bj = 0; bj < n_jobs; ++bj)
  {
    const size_t k = plan.jobs[bj], n = v.beams_of(k), to = c->job_first[k];
    std::memcpy(v.records_out + k * kVerRec, records + bj * kVerRec, kVerRec * sizeof(uint32_t));
    if (v.beam_m2_out != nullptr) std::memcpy(v.beam_m2_out + to, c->h_out + out.m2 + at, n * sizeof(double));
    if (v.beam_cells_out != nullptr) std::memcpy(v.beam_cells_out + 2 * to, c->h_out + out.cells + at, n * 2 * sizeof(uint32_t));
    if (v.beam_class_out != nullptr) std::memcpy(v.beam_class_out + to, classes + at, n);
    at += n;
  }
  return NDT2D_OK;
}

// What ndt2d_closure_refine and ndt2d_closure_verify (`entry`) refuse, every check before anything
// is launched: null arguments, the grid's parameters, the rules, every scan and every job -- what
// ndt2d_refine_run refuses, one text: batch/ndt2d_refine_jobs.h (rules NULL: the verification,
// which has none) -- every candidate, as ndt2d_closure_match does, and the jobs' candidates.
int check_job_call(ndt2d_closure * c, const char * entry, size_t n_candidates, const CandidateMaps & m, double ndt_resolution,
                   double range_max, const double * jobs_xyt, const uint32_t * job_scan, const uint32_t * job_candidate,
                   size_t n_jobs, const double * beams_xy, const size_t * beam_offsets, size_t n_scans, const void * records_out,
                   const ndt2d::refine::Rules * rules)
{
  const std::string who = std::string(entry) + ": ";
  if (m.cand_offsets == nullptr || m.ids == nullptr || m.poses_xyt == nullptr || jobs_xyt == nullptr || records_out == nullptr ||
      beams_xy == nullptr || beam_offsets == nullptr)
  {
    return batch_fail(c, NDT2D_ERR_INVALID, who + "null argument");
  }
  if (!(ndt_resolution > 0.0) || !std::isfinite(ndt_resolution) || !std::isfinite(range_max))
  {
    return batch_fail(c, NDT2D_ERR_INVALID, who + "bad resolution or range_max");
  }
  if (n_candidates >= (1u << 24)) return batch_fail(c, NDT2D_ERR_INVALID, who + "bad argument (n_candidates)");
  if (job_candidate == nullptr && n_candidates != n_jobs)
  {
    return batch_fail(c, NDT2D_ERR_INVALID,
                      who + "bad argument (no job_candidate: job k uses candidate k, n_candidates must equal n_jobs)");
  }
  const std::string refusal =
    rules != nullptr
      ? ndt2d::refine_jobs::refusal(entry, jobs_xyt, job_scan, n_jobs, beam_offsets, n_scans, rules->max_evals, rules->tol_lin, rules->tol_ang)
      : ndt2d::refine_jobs::refusal(entry, jobs_xyt, job_scan, n_jobs, beam_offsets, n_scans);
  if (!refusal.empty()) return batch_fail(c, NDT2D_ERR_INVALID, refusal);
  const int crc = check_candidates(c, entry, n_candidates, m.cand_offsets, m.ids, m.poses_xyt, ndt_resolution, range_max);
  if (crc != NDT2D_OK) return crc;
  for (size_t k = 0; k < n_jobs && job_candidate != nullptr; ++k)
  {
    if (job_candidate[k] >= n_candidates)
    {
      return batch_fail(c, NDT2D_ERR_INVALID, who + "job " + std::to_string(k) + ": candidate " + std::to_string(job_candidate[k]) +
                                             " of " + std::to_string(n_candidates));
    }
  }
  return NDT2D_OK;
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
  // every candidate is checked before anything is launched
  const int crc = check_candidates(c, "ndt2d_closure_match", n_candidates, cand_offsets, ids, poses_xyt, ndt_resolution, range_max);
  if (crc != NDT2D_OK) return crc;
  NDT2D_BATCH_HIP(c, hipSetDevice(c->device));
  const SearchTables t{beams_xy, n_beams, pose_x, pose_y, dth, cos_th, sin_th, n_th, dlin, n_lin};
  // more candidates than slots: in chunks
  for (size_t k0 = 0; k0 < n_candidates; k0 += c->max_candidates)
  {
    const size_t k1 = std::min(n_candidates, k0 + c->max_candidates);
    const int rc = match_chunk(c, k0, k1, {cand_offsets, ids, poses_xyt}, t, records_out, all_scores);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_set_neighbourhood(ndt2d_closure * c, uint32_t cells)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (cells != 1 && cells != 9)
  {
    return batch_fail(c, NDT2D_ERR_INVALID, "ndt2d_closure_set_neighbourhood: " + std::to_string(cells) + " cells (1 or 9)");
  }
  c->cells = cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_neighbourhood(ndt2d_closure * c, uint32_t * out)
{
  NDT2D_C_TRY
  if (c == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = c->cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_refine(ndt2d_closure * c, size_t n_candidates, const size_t * cand_offsets, const size_t * ids,
                         const double * poses_xyt, double ndt_resolution, double range_max, const double * jobs_xyt,
                         const uint32_t * job_scan, const uint32_t * job_candidate, size_t n_jobs, const double * beams_xy,
                         const size_t * beam_offsets, size_t n_scans, uint32_t max_evals, double tol_lin, double tol_ang,
                         double * records_out)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  const CandidateMaps m{cand_offsets, ids, poses_xyt};
  const ndt2d::refine::Rules rules{max_evals, tol_lin, tol_ang};
  const int crc = check_job_call(c, "ndt2d_closure_refine", n_candidates, m, ndt_resolution, range_max, jobs_xyt, job_scan,
                                 job_candidate, n_jobs, beams_xy, beam_offsets, n_scans, records_out, &rules);
  if (crc != NDT2D_OK) return crc;
  NDT2D_BATCH_HIP(c, hipSetDevice(c->device));
  const RefineCall t{{jobs_xyt, job_scan, n_jobs, beams_xy, beam_offsets, n_scans}, rules};
  for (const ndt2d::ClosureJobChunk & chunk :
       ndt2d::plan_closure_jobs(job_candidate, n_jobs, n_candidates, c->max_candidates, ndt2d::kRefineMaxJobs))
  {
    const int rc = refine_chunk(c, chunk, m, t, records_out);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_set_verify_neighbourhood(ndt2d_closure * c, uint32_t cells)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  return ndt2d::batch_refuse(c, c->verify.set_cells("ndt2d_closure_set_verify_neighbourhood", cells));
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_verify_neighbourhood(ndt2d_closure * c, uint32_t * out)
{
  NDT2D_C_TRY
  if (c == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = c->verify.cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_set_verify_gates(ndt2d_closure * c, double gate_inlier, double gate_pierce)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  return ndt2d::batch_refuse(c, c->verify.set_gates("ndt2d_closure_set_verify_gates", gate_inlier, gate_pierce));
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_verify_gates(ndt2d_closure * c, double * gate_inlier_out, double * gate_pierce_out)
{
  NDT2D_C_TRY
  if (c == nullptr || gate_inlier_out == nullptr || gate_pierce_out == nullptr) return NDT2D_ERR_INVALID;
  *gate_inlier_out = c->verify.gate_inlier;
  *gate_pierce_out = c->verify.gate_pierce;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_set_verify_rays(ndt2d_closure * c, int enabled)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  return ndt2d::batch_refuse(c, c->verify.set_rays("ndt2d_closure_set_verify_rays", enabled));
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_verify_rays(ndt2d_closure * c, int * out)
{
  NDT2D_C_TRY
  if (c == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = c->verify.rays ? 1 : 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_verify(ndt2d_closure * c, size_t n_candidates, const size_t * cand_offsets, const size_t * ids,
                         const double * poses_xyt, double ndt_resolution, double range_max, const double * jobs_xyt,
                         const uint32_t * job_scan, const uint32_t * job_candidate, size_t n_jobs, const double * beams_xy,
                         const size_t * beam_offsets, size_t n_scans, uint32_t * records_out, uint8_t * beam_class_out,
                         double * beam_m2_out, uint32_t * beam_cells_out)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  const CandidateMaps m{cand_offsets, ids, poses_xyt};
  const int crc = check_job_call(c, "ndt2d_closure_verify", n_candidates, m, ndt_resolution, range_max, jobs_xyt, job_scan,
                                 job_candidate, n_jobs, beams_xy, beam_offsets, n_scans, records_out, nullptr);
  if (crc != NDT2D_OK) return crc;
  for (size_t k = 0; k < n_candidates && c->verify.rays; ++k)
  {
    const GridDesc & g = c->slots[k].grid;
    if (g.size_x > ndt2d::verify::kMaxGridSide || g.size_y > ndt2d::verify::kMaxGridSide)
    {
      return batch_fail(c, NDT2D_ERR_INVALID,
                        "ndt2d_closure_verify: candidate " + std::to_string(k) + ": a grid side above 2^24 cells (rays enabled)");
    }
  }
  NDT2D_BATCH_HIP(c, hipSetDevice(c->device));
  const ndt2d::VerifyCall v{{jobs_xyt, job_scan, n_jobs, beams_xy, beam_offsets, n_scans},
                            records_out, beam_class_out, beam_m2_out, beam_cells_out};
  // job k's beams start at the sum of the earlier jobs' scan lengths
  c->job_first.resize(n_jobs + 1);
  c->job_beams.resize(n_jobs);
  c->job_first[0] = 0;
  for (size_t k = 0; k < n_jobs; ++k)
  {
    c->job_beams[k] = v.beams_of(k);
    c->job_first[k + 1] = c->job_first[k] + c->job_beams[k];
  }
  for (const ndt2d::ClosureJobChunk & chunk :
       ndt2d::plan_closure_jobs(job_candidate, n_jobs, n_candidates, c->max_candidates, ndt2d::kVerifyMaxJobs, c->job_beams.data(),
                                ndt2d::kVerifyChunkBeams))
  {
    const int rc = verify_chunk(c, chunk, m, v);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

}  // extern "C"
