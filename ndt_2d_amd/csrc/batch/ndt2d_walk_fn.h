// The lane of the batched searches (closure/ndt2d_closure.hip: one scan against K candidate maps;
// starts/ndt2d_starts.hip: one scan from K start poses on the installed grid; scans/ndt2d_scans.hip:
// K (scan, pose) jobs on the installed grid): a block per (theta step, slot), a lane per (dx, dy).
// What the one search kernel (ndt2d_batch_search.h) is made of lives here, so that a raw score
// has the same bits whichever of the three asks for it:
//
//   lane_walk      the block rotates the beams once for its theta step (points_outer,
//                  src/scan_matcher_ndt.cpp:106-115) into LDS in pieces of kStageBeams; every lane
//                  adds points_inner = outer + (dx, dy) (:121-125) through cell_index /
//                  record_exponent / exp_score of ndt2d_device_fn.h, keeping C in-order partial
//                  sums over groups of four beams dealt round-robin, and returns
//                  ((p_0 + p_1) + p_2) + ... -- the small-lattice search's sum (ndt2d_sum_chunks.h).
//   block_record   the block's (or the reducing block's) lanes -> one record
//                  {best_score, best_index (+0.5: near tie), acc[10]}: lanes over the DPP network,
//                  waves in wave order.
//
// The map a lane scores against is a policy (MAP): find(cell, &rank) says whether the cell can
// score and which record is its own, record(rank) points at {mean, -0.5 information} as three
// 16-byte pieces.  Included by the .hip translation units only.
#ifndef NDT2D_WALK_FN_H_
#define NDT2D_WALK_FN_H_

#include "ndt2d_device_fn.h"
#include "ndt2d_sum_chunks.h"

namespace ndt2d
{

constexpr uint32_t kStageBeams = 1024;        // beams rotated into LDS at a time
constexpr uint32_t kSearchMaxThreads = 1024;
constexpr uint32_t kReduceThreads = 256;
static_assert(kStageBeams * sizeof(double2) >= (kSearchMaxThreads / 64) * kRecord * sizeof(double), "a record per wave");

// One beam of one lattice candidate: the term the reference adds (:127, NDT::likelihood).
template <bool POW2, class MAP>
__device__ __forceinline__ void add_beam(const GridDesc & g, const MAP & map, double2 o, double dx, double dy,
                                         bool valid, double skip_below, double & sum, bool & added)
{
  const double px = o.x + dx;   // points_inner (:123-124)
  const double py = o.y + dy;
  const uint32_t cell = cell_index<POW2>(g, px, py);   // ncell: off the grid
  uint32_t rank;
  const bool found = map.find(cell, rank);
  const bool has = valid & found;
  if (wave_any(has))
  {
    const double2 * r = map.record(has ? rank : 0u);
    const double2 m = r[0], h0 = r[1], h1 = r[2];
    // (a lane without a record: exponent -inf, the reference's +0.0)
    const double e = has ? record_exponent(m.x, m.y, h0.x, h0.y, h1.x, px, py) : -HUGE_VAL;
    // !(e < bound) also keeps NaN exponents (degenerate cells) on the exact path
    if (wave_any(!(e < skip_below)))
    {
      sum += exp_score(e);
      added = true;
    }
  }
}

// The raw likelihood sum of the lane's candidate (dx, dy) for the block's theta step (ct, st) and
// pose.  rows: kStageBeams entries of LDS.  Called by every thread of the block (barriers inside);
// `valid` = the lane holds a candidate.
template <int C, bool POW2, class MAP>
__device__ __forceinline__ double lane_walk(const GridDesc & g, const MAP & map, double2 * rows,
                                            const double * beams_xy, uint32_t n_beams, double ct, double st,
                                            double pose_x, double pose_y, double dx, double dy, bool valid)
{
  const uint32_t tid = threadIdx.x, n_threads = blockDim.x;
  const uint32_t n_groups = (n_beams + kGroupBeams - 1) / kGroupBeams;
  // groups of a piece: whole rounds of the C partial sums
  constexpr uint32_t kPieceGroups = (kStageBeams / kGroupBeams / C) * C;
  double p[C], skip_below[C];
#pragma unroll
  for (int j = 0; j < C; ++j)
  {
    p[j] = 0.0;
    skip_below[j] = negligible_below(0.0);
  }
  for (uint32_t g0 = 0; g0 < n_groups; g0 += kPieceGroups)
  {
    const uint32_t b0 = g0 * kGroupBeams;
    const uint32_t b1 = min(n_beams, b0 + kPieceGroups * kGroupBeams);
    __syncthreads();   // the piece before has been read
    for (uint32_t b = b0 + tid; b < b1; b += n_threads)
    {
      const double2 q = reinterpret_cast<const double2 *>(beams_xy)[b];
      // points_outer (:111-114)
      rows[b - b0] = double2{q.x * ct - q.y * st + pose_x, q.x * st + q.y * ct + pose_y};
    }
    __syncthreads();
    const uint32_t g1 = (b1 - b0 + kGroupBeams - 1) / kGroupBeams;   // groups of this piece
    for (uint32_t gr = 0; gr < g1; gr += C)
    {
#pragma unroll
      for (int j = 0; j < C; ++j)
      {
        const uint32_t first = (gr + j) * kGroupBeams;   // within the piece
        if (first < b1 - b0)
        {
          bool added = false;
#pragma unroll
          for (uint32_t u = 0; u < kGroupBeams; ++u)
          {
            if (first + u < b1 - b0)
            {
              add_beam<POW2>(g, map, rows[first + u], dx, dy, valid, skip_below[j], p[j], added);
            }
          }
          if (added) skip_below[j] = negligible_below(p[j]);
        }
      }
    }
  }
  // ((p_0 + p_1) + p_2) + ... as the small-lattice search adds its waves' partial sums
  double sum = p[0];
#pragma unroll
  for (int j = 1; j < C; ++j) sum += p[j];
  return sum;
}

// A lane's candidate into its running record: the reference's strict-< best (:128-134) and
// k += x x^T score, u += x score, s += score (:137-140).
__device__ __forceinline__ void lane_take(double score, uint64_t flat, double dx, double dy, double dt,
                                          double & best_s, double & best_i, double (&acc)[10])
{
  double cs = 0.0, ci = kNoIndex;
  if (score < 0.0)
  {
    cs = score;
    ci = static_cast<double>(flat);
  }
  merge_best(cs, ci, best_s, best_i);
  acc[0] += (dx * dx) * score;
  acc[1] += (dx * dy) * score;
  acc[2] += (dx * dt) * score;
  acc[3] += (dy * dy) * score;
  acc[4] += (dy * dt) * score;
  acc[5] += (dt * dt) * score;
  acc[6] += dx * score;
  acc[7] += dy * score;
  acc[8] += dt * score;
  acc[9] += score;
}

// The block's record from its lanes' records: lanes over the DPP network, waves in wave order.
// scratch: LDS for one record per wave, free to be written behind the barrier this begins with.
// FINAL: "no candidate scored below 0 -> no index" is applied (the reducing block).
template <bool FINAL>
__device__ __forceinline__ void block_record(double best_s, double best_i, double (&acc)[10], double * scratch,
                                             double * out)
{
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & (kWave - 1), wave = tid >> 6, n_waves = blockDim.x >> 6;
  wave_best_to_last_lane(best_s, best_i);
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = wave_sum_to_last_lane(acc[k]);
  __syncthreads();
  if (lane == kWave - 1)
  {
    scratch[wave * kRecord + 0] = best_s;
    scratch[wave * kRecord + 1] = best_i;
#pragma unroll
    for (int k = 0; k < 10; ++k) scratch[wave * kRecord + 2 + k] = acc[k];
  }
  __syncthreads();
  if (tid < static_cast<uint32_t>(kRecord))
  {
    double val;
    if (tid < 2)
    {
      double s0 = scratch[0], i0 = scratch[1];
      for (uint32_t w = 1; w < n_waves; ++w) merge_best(scratch[w * kRecord], scratch[w * kRecord + 1], s0, i0);
      if (FINAL) val = tid == 0 ? s0 : (s0 < 0.0 ? i0 : -1.0);   // no candidate scored below 0: no index
      else val = tid == 0 ? s0 : i0;
    }
    else
    {
      val = scratch[tid];
      for (uint32_t w = 1; w < n_waves; ++w) val += scratch[w * kRecord + tid];
    }
    out[tid] = val;
  }
}

// The reducing block (kReduceThreads threads): the n_th records of one slot's search blocks ->
// the slot's record, thread t taking records t, t + kReduceThreads, ... in order.
__device__ __forceinline__ void reduce_slot_records(const double * slot_partials, uint32_t n_th, double * scratch,
                                                    double * out)
{
  double bs = 0.0, bi = kNoIndex;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  for (uint32_t r = threadIdx.x; r < n_th; r += kReduceThreads)
  {
    const double * p = slot_partials + static_cast<size_t>(r) * kRecord;
    merge_best(p[0], p[1], bs, bi);
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] += p[2 + k];
  }
  block_record<true>(bs, bi, acc, scratch, out);
}

}  // namespace ndt2d

#endif  // NDT2D_WALK_FN_H_
