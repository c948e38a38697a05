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
//   closure_search_kernel  grid (theta step, candidate map), a lane per (dx, dy): the block
//       rotates the beams once for its theta step (points_outer, src/scan_matcher_ndt.cpp:
//       106-115, cos / sin from the host libm) into LDS in pieces of kStageBeams, every lane adds
//       points_inner = outer + (dx, dy) (:121-125) through cell_index / record_exponent /
//       exp_score of ndt2d_device_fn.h.  K x n_theta blocks: 640 of seven waves for the plugin's
//       defaults and K = 8, where one sequential search is 80 x 7 tiles.
//   closure_reduce_kernel  one block per candidate map: the n_theta records of its blocks ->
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
#include <cstring>
#include <string>
#include <vector>

#include "../build_small/ndt2d_build_small_fn.h"
#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "ndt2d_walk_fn.h"

namespace ndt2d
{

namespace
{

using namespace fused;

constexpr uint32_t kNoRecord = 0xffffu;
// (the lane's beam walk, the block records and the chunk plan: ndt2d_walk_fn.h, shared with ../starts/)

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

struct ClosureSearchArgs
{
  const ClosureSlot * slots;
  const uint16_t * lookup;
  const double * records;
  const double * beams_xy;   // [n_beams][2] robot frame
  const double * dth, * cos_th, * sin_th, * dlin;
  uint32_t n_beams, n_th, n_lin;
  double pose_x, pose_y;
  double * scores;           // optional: [slot][n_th * n_lin * n_lin]
  double * partials;         // [slot][n_th][kRecord]
};

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

template <int C, bool POW2>
__global__ void __launch_bounds__(kSearchMaxThreads) closure_search_kernel(const ClosureSearchArgs a)
{
  __shared__ double2 rows[kStageBeams];
  const uint32_t ith = blockIdx.x, slot = blockIdx.y;
  const uint32_t tid = threadIdx.x, n_threads = blockDim.x;
  const ClosureSlot & s = a.slots[slot];
  const GridDesc g = s.grid;
  const SlotMap map{a.lookup + s.lookup_off, a.records + 6 * static_cast<size_t>(s.list_off)};
  const double ct = a.cos_th[ith], st = a.sin_th[ith], dt = a.dth[ith];
  const uint32_t n_lin = a.n_lin, n_cand = n_lin * n_lin;

  double best_s = 0.0;       // `double best_score = 0;` (:83)
  double best_i = kNoIndex;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;

  for (uint32_t c0 = 0; c0 < n_cand; c0 += n_threads)
  {
    const uint32_t c = c0 + tid;
    const bool valid = c < n_cand;
    const uint32_t cc = valid ? c : n_cand - 1u;
    const uint32_t ix = cc / n_lin, iy = cc - ix * n_lin;
    const double dx = a.dlin[ix], dy = a.dlin[iy];
    const double sum = lane_walk<C, POW2>(g, map, rows, a.beams_xy, a.n_beams, ct, st, a.pose_x, a.pose_y, dx, dy, valid);
    if (valid)
    {
      const double score = -sum;  // (:127)
      lane_take(score, static_cast<uint64_t>(ith) * n_cand + c, dx, dy, dt, best_s, best_i, acc);
      if (a.scores != nullptr) a.scores[(static_cast<uint64_t>(slot) * a.n_th + ith) * n_cand + c] = score;
    }
  }
  // the block's record (the rows are free behind block_record's first barrier)
  block_record<false>(best_s, best_i, acc, reinterpret_cast<double *>(rows),
                      a.partials + (static_cast<size_t>(slot) * a.n_th + ith) * kRecord);
}

// partials[slot][n_th][kRecord] -> out[slot][kRecord]
__global__ void __launch_bounds__(kReduceThreads) closure_reduce_kernel(const double * partials, uint32_t n_th,
                                                                         double * out)
{
  __shared__ double scratch[(kReduceThreads / 64) * kRecord];
  const uint32_t slot = blockIdx.x;
  reduce_slot_records(partials + static_cast<size_t>(slot) * n_th * kRecord, n_th, scratch,
                      out + static_cast<size_t>(slot) * kRecord);
}

template <bool POW2>
void launch_search_c(uint32_t chunks, dim3 grid, dim3 block, hipStream_t stream, const ClosureSearchArgs & a)
{
  switch (chunks)
  {
    case 1: hipLaunchKernelGGL((closure_search_kernel<1, POW2>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((closure_search_kernel<2, POW2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((closure_search_kernel<3, POW2>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((closure_search_kernel<4, POW2>), grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL((closure_search_kernel<5, POW2>), grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL((closure_search_kernel<6, POW2>), grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL((closure_search_kernel<7, POW2>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((closure_search_kernel<8, POW2>), grid, block, 0, stream, a); break;
  }
}

}  // namespace

}  // namespace ndt2d

// ---- the object and the C entry points ----

struct ndt2d_closure
{
  ndt2d_handle h = nullptr;
  ndt2d_scanstore * store = nullptr;
  int device = 0;
  size_t max_candidates = 0;
  std::string err;
  // one upload per chunk: [tables | beams | slots | scan table] (doubles), pinned and on the device
  double * h_stage = nullptr, * d_stage = nullptr;
  size_t stage_cap = 0;
  // per chunk, grown on demand (bytes)
  void * d_world = nullptr, * d_cells6 = nullptr, * d_records = nullptr, * d_index = nullptr, * d_lookup = nullptr;
  size_t world_cap = 0, cells6_cap = 0, records_cap = 0, index_cap = 0, lookup_cap = 0;
  uint32_t * d_n_touched = nullptr;
  void * d_partials = nullptr;
  size_t partials_cap = 0;
  // what comes back: [slot][12] records | [slot][lattice] scores (doubles), on the device and pinned
  double * d_out = nullptr, * h_out = nullptr;
  size_t out_cap = 0;
  std::vector<ndt2d::ClosureSlot> slots;
  bool timing = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // before the build, behind it, behind the search
  bool timed = false;
};

namespace
{

using ndt2d::GridDesc;
using ndt2d::ClosureSlot;
using ndt2d::fused::SmallScan;
constexpr size_t kRec = NDT2D_MATCH_RECORD_DOUBLES;

void guard_note(ndt2d_closure * c, const char * what) noexcept
{
  if (c == nullptr) return;
  try
  {
    c->err = what;
  }
  catch (...)
  {
  }
}
void guard_note(std::nullptr_t, const char *) noexcept {}

int cfail(ndt2d_closure * c, int code, const std::string & msg)
{
  if (c != nullptr) c->err = msg;
  return code;
}

int cfail_hip(ndt2d_closure * c, hipError_t e, const char * what)
{
  (void)hipGetLastError();  // clear sticky state
  return cfail(c, NDT2D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define NDT2D_CLOSURE_HIP(c, call)                          \
  do                                                        \
  {                                                         \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return cfail_hip(c, e__, #call); \
  } while (0)

// Device memory of at least `bytes` at *p (contents are not kept).
hipError_t grow_device(void ** p, size_t * cap, size_t bytes)
{
  if (bytes <= *cap) return hipSuccess;
  if (*p != nullptr) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = bytes + bytes / 4;
  const hipError_t e = hipMalloc(p, want);
  if (e == hipSuccess) *cap = want;
  return e;
}

hipError_t grow_pinned(double ** p, size_t doubles)
{
  if (*p != nullptr) (void)hipHostFree(*p);
  *p = nullptr;
  return hipHostMalloc(reinterpret_cast<void **>(p), doubles * sizeof(double), hipHostMallocDefault);
}

void free_closure(ndt2d_closure * c)
{
  (void)hipSetDevice(c->device);
  if (c->h_stage != nullptr) (void)hipHostFree(c->h_stage);
  if (c->d_stage != nullptr) (void)hipFree(c->d_stage);
  if (c->d_world != nullptr) (void)hipFree(c->d_world);
  if (c->d_cells6 != nullptr) (void)hipFree(c->d_cells6);
  if (c->d_records != nullptr) (void)hipFree(c->d_records);
  if (c->d_index != nullptr) (void)hipFree(c->d_index);
  if (c->d_lookup != nullptr) (void)hipFree(c->d_lookup);
  if (c->d_n_touched != nullptr) (void)hipFree(c->d_n_touched);
  if (c->d_partials != nullptr) (void)hipFree(c->d_partials);
  if (c->d_out != nullptr) (void)hipFree(c->d_out);
  if (c->h_out != nullptr) (void)hipHostFree(c->h_out);
  for (hipEvent_t ev : c->ev)
  {
    if (ev != nullptr) (void)hipEventDestroy(ev);
  }
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
  if (n_stage > c->stage_cap)
  {
    const size_t cap = n_stage + n_stage / 4 + 512;
    c->stage_cap = 0;
    NDT2D_CLOSURE_HIP(c, grow_pinned(&c->h_stage, cap));
    size_t dev_cap = 0;
    void * d = c->d_stage;
    c->d_stage = nullptr;
    if (d != nullptr) (void)hipFree(d);
    d = nullptr;
    NDT2D_CLOSURE_HIP(c, grow_device(&d, &dev_cap, cap * sizeof(double)));
    c->d_stage = static_cast<double *>(d);
    c->stage_cap = cap;
  }
  NDT2D_CLOSURE_HIP(c, grow_device(&c->d_world, &c->world_cap, std::max<size_t>(1, n_world) * 2 * sizeof(double)));
  NDT2D_CLOSURE_HIP(c, grow_device(&c->d_cells6, &c->cells6_cap, n_list * 6 * sizeof(double)));
  NDT2D_CLOSURE_HIP(c, grow_device(&c->d_records, &c->records_cap, n_list * 6 * sizeof(double)));
  NDT2D_CLOSURE_HIP(c, grow_device(&c->d_index, &c->index_cap, n_list * sizeof(uint32_t)));
  NDT2D_CLOSURE_HIP(c, grow_device(&c->d_lookup, &c->lookup_cap, n_lookup * sizeof(uint16_t)));
  NDT2D_CLOSURE_HIP(c, grow_device(&c->d_partials, &c->partials_cap, n_slots * t.n_th * kRec * sizeof(double)));
  const size_t n_out = n_slots * (kRec + (all_scores != nullptr ? n_lattice : 0));
  if (n_out > c->out_cap)
  {
    const size_t cap = n_out + n_out / 4;
    c->out_cap = 0;
    NDT2D_CLOSURE_HIP(c, grow_pinned(&c->h_out, cap));
    size_t dev_cap = 0;
    void * d = c->d_out;
    c->d_out = nullptr;
    if (d != nullptr) (void)hipFree(d);
    d = nullptr;
    NDT2D_CLOSURE_HIP(c, grow_device(&d, &dev_cap, cap * sizeof(double)));
    c->d_out = static_cast<double *>(d);
    c->out_cap = cap;
  }

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

  NDT2D_CLOSURE_HIP(c, hipMemcpyAsync(c->d_stage, st, n_stage * sizeof(double), hipMemcpyHostToDevice, stream));
  c->timed = false;
  if (c->timing) NDT2D_CLOSURE_HIP(c, hipEventRecord(c->ev[0], stream));

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
  NDT2D_CLOSURE_HIP(c, ndt2d::prepare_absolute_lds_kernel(reinterpret_cast<const void *>(ndt2d::closure_build_kernel),
                                                          ndt2d::fused::kLdsBytes));
  hipLaunchKernelGGL(ndt2d::closure_build_kernel, dim3(static_cast<uint32_t>(n_slots)), dim3(ndt2d::fused::kThreads),
                     ndt2d::fused::kLdsBytes, stream, b);
  NDT2D_CLOSURE_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_CLOSURE_HIP(c, hipEventRecord(c->ev[1], stream));

  ndt2d::ClosureSearchArgs a{};
  a.slots = b.slots;
  a.lookup = b.lookup;
  a.records = b.records;
  a.beams_xy = c->d_stage + off_beams;
  a.dth = c->d_stage;
  a.cos_th = c->d_stage + t.n_th;
  a.sin_th = c->d_stage + 2 * t.n_th;
  a.dlin = c->d_stage + 3 * t.n_th;
  a.n_beams = static_cast<uint32_t>(t.n_beams);
  a.n_th = static_cast<uint32_t>(t.n_th);
  a.n_lin = static_cast<uint32_t>(t.n_lin);
  a.pose_x = t.pose_x;
  a.pose_y = t.pose_y;
  a.scores = all_scores != nullptr ? c->d_out + n_slots * kRec : nullptr;
  a.partials = static_cast<double *>(c->d_partials);
  const size_t n_cand = t.n_lin * t.n_lin;
  const uint32_t threads = static_cast<uint32_t>(std::min<size_t>(ndt2d::kSearchMaxThreads, (n_cand + 63) & ~size_t(63)));
  const dim3 grid(static_cast<uint32_t>(t.n_th), static_cast<uint32_t>(n_slots));
  const uint32_t chunks = ndt2d::sum_chunks(a.n_beams);
  if (c->slots[k0].grid.pow2) ndt2d::launch_search_c<true>(chunks, grid, dim3(threads), stream, a);
  else ndt2d::launch_search_c<false>(chunks, grid, dim3(threads), stream, a);
  NDT2D_CLOSURE_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_CLOSURE_HIP(c, hipEventRecord(c->ev[2], stream));

  hipLaunchKernelGGL(ndt2d::closure_reduce_kernel, dim3(static_cast<uint32_t>(n_slots)), dim3(ndt2d::kReduceThreads), 0,
                     stream, a.partials, a.n_th, c->d_out);
  NDT2D_CLOSURE_HIP(c, hipGetLastError());
  // the one read-back of the chunk
  NDT2D_CLOSURE_HIP(c, hipMemcpyAsync(c->h_out, c->d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, stream));
  NDT2D_CLOSURE_HIP(c, hipStreamSynchronize(stream));
  c->timed = c->timing;
  std::memcpy(records_out + k0 * kRec, c->h_out, n_slots * kRec * sizeof(double));
  if (all_scores != nullptr)
  {
    std::memcpy(all_scores + k0 * n_lattice, c->h_out + n_slots * kRec, n_slots * n_lattice * sizeof(double));
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
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(c->h)));
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
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (enabled != 0 && c->ev[0] == nullptr)
  {
    NDT2D_CLOSURE_HIP(c, hipSetDevice(c->device));
    for (hipEvent_t & ev : c->ev) NDT2D_CLOSURE_HIP(c, hipEventCreate(&ev));
  }
  c->timing = enabled != 0;
  c->timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_closure_last_ms(ndt2d_closure * c, float * build_ms, float * search_ms)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (!c->timed) return cfail(c, NDT2D_ERR_STATE, "ndt2d_closure_last_ms: no timed match (ndt2d_closure_set_timing)");
  float b = 0.0f, s = 0.0f;
  NDT2D_CLOSURE_HIP(c, hipEventElapsedTime(&b, c->ev[0], c->ev[1]));
  NDT2D_CLOSURE_HIP(c, hipEventElapsedTime(&s, c->ev[1], c->ev[2]));
  if (build_ms != nullptr) *build_ms = b;
  if (search_ms != nullptr) *search_ms = s;
  return NDT2D_OK;
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
    return cfail(c, NDT2D_ERR_INVALID, "ndt2d_closure_match: null argument");
  }
  if (!(ndt_resolution > 0.0) || !std::isfinite(ndt_resolution) || !std::isfinite(range_max))
  {
    return cfail(c, NDT2D_ERR_INVALID, "ndt2d_closure_match: bad resolution or range_max");
  }
  if (n_beams == 0 || n_beams >= (1u << 24) || n_th == 0 || n_th >= (1u << 20) || n_lin == 0 || n_lin > 4096 ||
      n_candidates >= (1u << 24) || !std::isfinite(pose_x) || !std::isfinite(pose_y))
  {
    return cfail(c, NDT2D_ERR_INVALID, "ndt2d_closure_match: bad search (beams, lattice or pose)");
  }
  const ndt2d_scanstore * store = c->store;
  // every candidate is checked before anything is launched
  c->slots.assign(n_candidates, ClosureSlot{});
  for (size_t k = 0; k < n_candidates; ++k)
  {
    const std::string who = "ndt2d_closure_match: candidate " + std::to_string(k);
    if (cand_offsets[k + 1] < cand_offsets[k] || cand_offsets[k + 1] - cand_offsets[0] >= (1u << 28))
    {
      return cfail(c, NDT2D_ERR_INVALID, who + ": offsets must not decrease");
    }
    const size_t j0 = cand_offsets[k], j1 = cand_offsets[k + 1];
    if (j1 == j0) return cfail(c, NDT2D_ERR_INVALID, who + " has no scans");
    size_t n_points = 0;
    for (size_t j = j0; j < j1; ++j)
    {
      if (ids[j] >= store->count.size())
      {
        return cfail(c, NDT2D_ERR_INVALID, who + ": unknown scan id " + std::to_string(ids[j]));
      }
      if (!std::isfinite(poses_xyt[3 * j]) || !std::isfinite(poses_xyt[3 * j + 1]) || !std::isfinite(poses_xyt[3 * j + 2]))
      {
        return cfail(c, NDT2D_ERR_INVALID, who + ": a scan pose is not finite");
      }
      n_points += store->count[ids[j]];
    }
    ClosureSlot & s = c->slots[k];
    if (!ndt2d::fused::addscans_geometry(ndt_resolution, range_max, poses_xyt + 3 * j0, j1 - j0, &s.grid))
    {
      return cfail(c, NDT2D_ERR_INVALID, who + ": degenerate grid extent");
    }
    if (!ndt2d::fused::small_map_fits(s.grid, n_points) || s.grid.ncell == 0)
    {
      return cfail(c, NDT2D_ERR_INVALID, who + ": the map exceeds the fused build's limits (" + std::to_string(n_points) +
                                           " points of at most " + std::to_string(ndt2d::fused::kFusedMaxPoints) + ", " +
                                           std::to_string(s.grid.ncell) + " cells of fewer than 65535)");
    }
    s.n_scans = static_cast<uint32_t>(j1 - j0);
    s.n_points = static_cast<uint32_t>(n_points);
    s.sort_passes = ndt2d::fused::sort_passes_for(s.grid.ncell);
  }
  NDT2D_CLOSURE_HIP(c, hipSetDevice(c->device));
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
