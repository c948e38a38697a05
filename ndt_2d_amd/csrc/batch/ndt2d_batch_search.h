// The kernels of the batched searches, once (closure/ndt2d_closure.hip: one scan against K
// candidate maps; scans/ndt2d_scans.hip: K (scan, pose) jobs on the installed grid, and through it
// starts/ndt2d_starts.hip: one scan from K start poses):
//
//   batch_search_kernel<C, POW2, SLOTS>  grid (theta step, slot of the launch), a lane per
//       (dx, dy), as wide as the translation lattice (wider lattices loop): lane_walk<C, POW2> of
//       ndt2d_walk_fn.h per candidate, lane_take, the optional score store, the block's record.
//   batch_reduce_kernel   one block per slot: the n_theta records of its blocks ->
//       {best_score, best_index (+0.5: near tie), acc[10]} with merge_best, fixed order.
//
// What a block searches is a policy (SLOTS), carried by value in the kernel argument:
// load(blockIdx.y, ith, n_th) gives the block its BatchBlock -- the grid's geometry, the map policy of
// the walk, the beams and their count, the pose, cos / sin of the theta step and the slot its
// record and scores are written under.  Everything in it is uniform over the block.
// Included by the .hip translation units only.
#ifndef NDT2D_BATCH_SEARCH_H_
#define NDT2D_BATCH_SEARCH_H_

#include "ndt2d_installed_map.h"
#include "ndt2d_stage_layout.h"
#include "ndt2d_walk_fn.h"

namespace ndt2d
{

namespace
{

// What a block searches (MAP: the walk's map policy, ndt2d_walk_fn.h).
template <class MAP>
struct BatchBlock
{
  GridDesc grid;
  MAP map;
  const double * beams;   // [n_beams][2] robot frame
  uint32_t n_beams;
  double x, y, ct, st;    // the pose; cos / sin of (heading + dth[ith])
  uint32_t slot;          // its records and scores are written under
};

template <class SLOTS>
struct BatchSearchArgs
{
  SLOTS slots;
  const double * dth, * dlin;
  uint32_t n_th, n_lin;
  double * scores;           // optional: [slot][n_th * n_lin * n_lin]
  double * partials;         // [slot][n_th][kRecord]
};

template <int C, bool POW2, class SLOTS>
__global__ void __launch_bounds__(kSearchMaxThreads) batch_search_kernel(const BatchSearchArgs<SLOTS> a)
{
  __shared__ double2 rows[kStageBeams];
  const uint32_t ith = blockIdx.x;
  const uint32_t tid = threadIdx.x, n_threads = blockDim.x;
  const auto b = a.slots.load(blockIdx.y, ith, a.n_th);
  const double dt = a.dth[ith];
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
    const double sum = lane_walk<C, POW2>(b.grid, b.map, rows, b.beams, b.n_beams, b.ct, b.st, b.x, b.y, dx, dy, valid);
    if (valid)
    {
      const double score = -sum;  // (:127)
      lane_take(score, static_cast<uint64_t>(ith) * n_cand + c, dx, dy, dt, best_s, best_i, acc);
      if (a.scores != nullptr) a.scores[(static_cast<uint64_t>(b.slot) * a.n_th + ith) * n_cand + c] = score;
    }
  }
  // the block's record (the rows are free behind block_record's first barrier)
  block_record<false>(best_s, best_i, acc, reinterpret_cast<double *>(rows),
                      a.partials + (static_cast<size_t>(b.slot) * a.n_th + ith) * kRecord);
}

// partials[slot][n_th][kRecord] -> out[slot][kRecord]
__global__ void __launch_bounds__(kReduceThreads) batch_reduce_kernel(const double * partials, uint32_t n_th,
                                                                       double * out)
{
  __shared__ double scratch[(kReduceThreads / 64) * kRecord];
  const uint32_t slot = blockIdx.x;
  reduce_slot_records(partials + static_cast<size_t>(slot) * n_th * kRecord, n_th, scratch,
                      out + static_cast<size_t>(slot) * kRecord);
}

template <int C, class SLOTS>
void launch_batch_search_c(bool pow2, dim3 grid, dim3 block, hipStream_t stream, const BatchSearchArgs<SLOTS> & a)
{
  if (pow2) hipLaunchKernelGGL((batch_search_kernel<C, true, SLOTS>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((batch_search_kernel<C, false, SLOTS>), grid, block, 0, stream, a);
}

// chunks: the C of every slot of the launch (sum_chunks of its beam count).
template <class SLOTS>
void launch_batch_search(uint32_t chunks, bool pow2, dim3 grid, dim3 block, hipStream_t stream,
                         const BatchSearchArgs<SLOTS> & a)
{
  switch (chunks)
  {
    case 1: launch_batch_search_c<1>(pow2, grid, block, stream, a); break;
    case 2: launch_batch_search_c<2>(pow2, grid, block, stream, a); break;
    case 3: launch_batch_search_c<3>(pow2, grid, block, stream, a); break;
    case 4: launch_batch_search_c<4>(pow2, grid, block, stream, a); break;
    case 5: launch_batch_search_c<5>(pow2, grid, block, stream, a); break;
    case 6: launch_batch_search_c<6>(pow2, grid, block, stream, a); break;
    case 7: launch_batch_search_c<7>(pow2, grid, block, stream, a); break;
    default: launch_batch_search_c<8>(pow2, grid, block, stream, a); break;
  }
}

// The search block's width for a translation lattice of n_cand candidates.
inline uint32_t batch_search_threads(size_t n_cand)
{
  const size_t waves = (n_cand + 63) & ~size_t(63);
  return static_cast<uint32_t>(waves < kSearchMaxThreads ? waves : kSearchMaxThreads);
}

// One job of a chunk on the installed grid (InstalledMap: ndt2d_installed_map.h).
struct JobRec
{
  double x, y;
  uint32_t trig_row;     // its heading's row of the cos / sin table
  uint32_t n_beams;      // of its scan
  uint64_t beam_first;   // its scan's first beam within the chunk's beams
};
static_assert(sizeof(JobRec) == kJobDoubles * sizeof(double), "jobs travel in a buffer of doubles");

// SLOTS of the installed grid: slot y of the launch is job order[first + y] of the chunk, with its
// own beams, pose and heading row.
struct JobSlots
{
  GridDesc grid;             // geometry, cells_global, occ_bits
  const JobRec * jobs;       // [job of the chunk]
  const uint32_t * order;    // launch position -> job (ndt2d_job_groups.h)
  const double * trig;       // [rows][2][n_th]: cos | sin of (heading + dth[i])
  const double * beams_xy;   // the chunk's scans, [beam][2] robot frame
  uint32_t first;            // launch position of the group's first job

  __device__ __forceinline__ BatchBlock<InstalledMap> load(uint32_t y, uint32_t ith, uint32_t n_th) const
  {
    const uint32_t job = order[first + y];   // (uniform over the block)
    const JobRec s = jobs[job];
    const double * row = trig + static_cast<size_t>(s.trig_row) * 2 * n_th;
    return {grid, InstalledMap{grid.occ_bits, grid.cells_global}, beams_xy + 2 * s.beam_first, s.n_beams,
            s.x, s.y, row[ith], row[n_th + ith], job};
  }
};

// One start pose of a chunk: a job whose scan is the call's.
struct StartRec
{
  double x, y;
  uint32_t trig_row;   // its heading's row of the cos / sin table
  uint32_t pad;
};
static_assert(sizeof(StartRec) == kStartDoubles * sizeof(double), "starts travel in a buffer of doubles");

// SLOTS of one scan from K start poses on the installed grid: slot y of the launch is start y of
// the chunk; the beams are the call's.  (JobSlots with one scan costs a block an order entry, a
// longer record and a beam count that arrives with the record: measured)
struct StartSlots
{
  GridDesc grid;             // geometry, cells_global, occ_bits
  const StartRec * starts;   // [start of the chunk]
  const double * trig;       // [rows][2][n_th]: cos | sin of (heading + dth[i])
  const double * beams_xy;   // [n_beams][2] robot frame
  uint32_t n_beams;

  __device__ __forceinline__ BatchBlock<InstalledMap> load(uint32_t y, uint32_t ith, uint32_t n_th) const
  {
    const StartRec s = starts[y];
    const double * row = trig + static_cast<size_t>(s.trig_row) * 2 * n_th;
    return {grid, InstalledMap{grid.occ_bits, grid.cells_global}, beams_xy, n_beams, s.x, s.y, row[ith], row[n_th + ith], y};
  }
};

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_BATCH_SEARCH_H_
