// The kernel of the Newton NDT registration, once (refine/ndt2d_refine.hip: K (scan, pose) jobs on
// the installed grid; closure/ndt2d_closure.hip: jobs on the loop closure's candidate maps): its
// job record, its arguments and the whole iteration of a job in one block (gfx950 / MI355X).  The
// objective, its ten sums and the iteration are the contract of include/ndt2d_hip.h ("Newton NDT
// registration"); the step between two evaluations is refine/ndt2d_refine_step.h.
//
//   refine_kernel<POW2>   grid (job of the chunk), 256 threads.  An evaluation at pose (x, y,
//       theta): thread t takes beams t, t + 256, ... of the job's scan in order, each through
//       cell_index / InstalledMap::find / record_exponent / exp_score of the shared device
//       functions, into ten partial sums {e, e a_0..2, e (-a_j a_k + M_jk)}; lanes reduce with
//       wave_sum_to_last_lane, the four waves in wave order.  Thread 0 turns the sums into
//       (f, g, H), runs the step (refine::begin / take) and leaves the trial pose with its cos /
//       sin and a control word in LDS; the block loops until the job stops, thread 0 writes the
//       job's record.
//   refine_kernel<POW2, 9>   the objective over the 3 x 3 cells round a point
//       (ndt2d_refine_set_neighbourhood): a job's items are (beam, neighbour) pairs, i = 9 beam
//       + j, neighbour j = (dy, dx) = (j / 3 - 1, j % 3 - 1) from the beam's own cell; thread t takes
//       items t, t + 256, ... in order, so a 100-beam scan occupies all 256 threads.  A neighbour
//       counts when it lies on the grid -- clipped on (gx, gy), not on the flat index: at gx = 0
//       the flat index minus one is the last cell of the row below -- and can score.  A trip in
//       which no lane of the wave holds a counting neighbour is skipped by a wave-wide vote (it
//       adds nothing).  CELLS = 1 is the loop above, instantiated apart: its code is the one-cell
//       kernel's as it was.
//
// The map is a template argument of the kernel.  A SOURCE gives, for the slot a job's record
// names, the GridDesc of that job's map (grid(slot): the geometry cell_index and the 3 x 3 clip
// use) and its map object of the walk's kind (map(slot): find(cell, rank) / record(rank),
// batch/ndt2d_walk_fn.h; entry ncell of it exists and never scores); both are uniform over the
// block.  InstalledSource (batch/ndt2d_installed_map.h) is the grid installed in the context: one
// grid for all jobs, refine/ndt2d_refine.hip.  The loop closure refines each job on its candidate's
// own map with the same kernel: closure/ndt2d_closure.hip includes this header too -- the kernel has
// one text, this one -- and instantiates it with its slots.
//
// The beams are read from the chunk's upload at every evaluation: a scan is at most a few KB per
// job and stays in L2 between the evaluations of its block, so nothing is staged in LDS and a
// scan of any length (beyond kStageBeams too) takes the same path.
//
// Off the grid.  cell_index gives ncell for every point outside the grid (NaN and infinite ones
// included), bit ncell of the bitmap is 0 and record ncell exists, so no lane indexes beyond
// either.  A job's beams are read at [beam_first, beam_first + n_beams) of the chunk's upload only;
// both come from the host's table, checked against the offsets before anything is launched.
//
// Determinism.  A thread's sums are its own, lanes reduce over the DPP network, waves in wave
// order; thread 0 alone decides.  No block waits for another, __syncthreads is the only barrier,
// stream order the only ordering between the upload, the launch and the read-back; no polls, no
// atomics.  A job's bits depend on its scan, its pose and the grid alone: not on the other jobs
// or the chunking.  cos / sin of the START heading come from the host libm inside the call, those
// of the later headings from the device's sincos.
//
// LDS: 4 x 10 wave sums, the pose of the evaluation with its cos / sin (5 doubles) and the control
// word: 364 bytes.  185 vector registers, no scratch (CELLS = 9: DESIGN.md 3.13).
// Included by the .hip translation units only.
#ifndef NDT2D_REFINE_KERNEL_H_
#define NDT2D_REFINE_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>

#include "ndt2d_hip.h"
#include "batch/ndt2d_installed_map.h"
#include "refine/ndt2d_refine_step.h"

namespace ndt2d
{

namespace
{

constexpr uint32_t kRefineThreads = 256;
constexpr uint32_t kRefineWaves = kRefineThreads / kWave;
constexpr uint32_t kRefineMaxJobs = 4096;   // blocks of a launch
constexpr int kSums = 10;             // e | e a_0..2 | H xx, xy, xt, yy, yt, tt
constexpr size_t kRefineRec = NDT2D_REFINE_RECORD_DOUBLES;

static_assert(refine::kConverged == NDT2D_REFINE_CONVERGED && refine::kMaxEvals == NDT2D_REFINE_MAX_EVALS &&
              refine::kStalled == NDT2D_REFINE_STALLED && refine::kNoOverlap == NDT2D_REFINE_NO_OVERLAP &&
              refine::kNotFinite == NDT2D_REFINE_NOT_FINITE, "the step's status values are the header's");

// One job of a chunk.
struct RefineJob
{
  double x, y, theta;
  uint32_t n_beams;      // of its scan
  uint32_t slot;         // of its map within the chunk (the installed grid: 0)
  uint64_t beam_first;   // its scan's first beam within the chunk's beams
};
constexpr size_t kRefineJobDoubles = 5;
static_assert(sizeof(RefineJob) == kRefineJobDoubles * sizeof(double), "jobs travel in a buffer of doubles");

template <class SOURCE>
struct RefineArgs
{
  SOURCE source;              // job -> its map
  const RefineJob * jobs;     // [job of the chunk]
  const double * trig;        // [job of the chunk][2]: cos, sin of its start heading (host libm)
  const double * beams_xy;    // the chunk's scans, [beam][2] robot frame
  refine::Rules rules;
  double * records;           // [job of the chunk][NDT2D_REFINE_RECORD_DOUBLES]
};

// The terms of the point q = R b + t against the record of `cell` into the thread's ten sums.
// Called by every lane of the wave together (exp_score tests the wave); valid = the lane holds an
// item whose cell may count (cell <= ncell; ncell: the sentinel, which never scores).
template <class MAP>
__device__ __forceinline__ void add_cell_terms(const MAP & map, uint32_t cell, double2 b, bool valid, double qx,
                                               double qy, double c, double s, double (&sum)[kSums])
{
  uint32_t rank;
  const bool found = map.find(cell, rank);
  const bool has = valid & found;
  const double2 * r = map.record(has ? rank : 0u);
  const double2 m = r[0], h0 = r[1], h1 = r[2];
  // (a lane without a record: exponent -inf, e = +0.0, and nothing is added)
  const double e = exp_score(has ? record_exponent(m.x, m.y, h0.x, h0.y, h1.x, qx, qy) : -HUGE_VAL);
  if (!has) return;
  // the information matrix: the records hold h = -0.5 I (exact scaling)
  const double i00 = -2.0 * h0.x, i01 = -2.0 * h0.y, i11 = -2.0 * h1.x;
  const double d0 = qx - m.x, d1 = qy - m.y;
  const double u0 = i00 * d0 + i01 * d1;
  const double u1 = i01 * d0 + i11 * d1;
  const double r0 = -s * b.x - c * b.y, r1 = c * b.x - s * b.y;   // dq / dtheta
  const double w0 = -c * b.x + s * b.y, w1 = -s * b.x - c * b.y;  // d2q / dtheta2
  const double a2 = u0 * r0 + u1 * r1;
  const double ir0 = i00 * r0 + i01 * r1;
  const double ir1 = i01 * r0 + i11 * r1;
  const double m22 = (r0 * ir0 + r1 * ir1) + (u0 * w0 + u1 * w1);
  sum[0] += e;
  sum[1] += e * u0;
  sum[2] += e * u1;
  sum[3] += e * a2;
  sum[4] += e * (-(u0 * u0) + i00);
  sum[5] += e * (-(u0 * u1) + i01);
  sum[6] += e * (-(u0 * a2) + ir0);
  sum[7] += e * (-(u1 * u1) + i11);
  sum[8] += e * (-(u1 * a2) + ir1);
  sum[9] += e * (-(a2 * a2) + m22);
}

// One beam's terms at the pose (x, y | c, s), against the cell it falls in.
template <bool POW2, class MAP>
__device__ __forceinline__ void add_terms(const GridDesc & g, const MAP & map, double2 b, bool valid, double x,
                                          double y, double c, double s, double (&sum)[kSums])
{
  const double qx = c * b.x - s * b.y + x;
  const double qy = s * b.x + c * b.y + y;
  const uint32_t cell = cell_index<POW2>(g, qx, qy);   // ncell: off the grid
  add_cell_terms(map, cell, b, valid, qx, qy, c, s, sum);
}

// The cell of a (beam, neighbour) item: neighbour j of the point's own cell, (dy, dx) = (j / 3 - 1,
// j % 3 - 1).  Off the grid (the point itself, NaN and infinite ones included, or the neighbour):
// the sentinel cell ncell, which never scores.
template <bool POW2>
__device__ __forceinline__ uint32_t neighbour_cell(const GridDesc & g, double qx, double qy, uint32_t j)
{
  const uint32_t own = cell_index<POW2>(g, qx, qy);   // ncell: off the grid
  const uint32_t gy = own / g.size_x, gx = own - gy * g.size_x;
  // (unsigned: gx + dx = -1 wraps to 2^32 - 1 and fails the same compare as gx + dx = size_x)
  const uint32_t nx = gx + (j % 3u) - 1u, ny = gy + (j / 3u) - 1u;
  const bool on = (own < g.ncell) & (nx < g.size_x) & (ny < g.size_y);
  return on ? ny * g.size_x + nx : g.ncell;
}

// SOURCE: where a job's map comes from (above).
template <bool POW2, uint32_t CELLS, class SOURCE>
__global__ void __launch_bounds__(kRefineThreads) refine_kernel(const RefineArgs<SOURCE> a)
{
  __shared__ double wave_sums[kRefineWaves][kSums];
  __shared__ double at[5];     // the pose of the evaluation: x, y, theta, cos, sin
  __shared__ uint32_t more;    // the control word: another evaluation is wanted
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const uint32_t job = blockIdx.x;
  const RefineJob jr = a.jobs[job];   // (uniform over the block)
  const GridDesc & grid = a.source.grid(jr.slot);
  const auto map = a.source.map(jr.slot);
  const double2 * beams = reinterpret_cast<const double2 *>(a.beams_xy) + jr.beam_first;
  const double start[3] = {jr.x, jr.y, jr.theta};
  refine::State st;   // (thread 0's)
  if (tid == 0)
  {
    at[0] = jr.x;
    at[1] = jr.y;
    at[2] = jr.theta;
    at[3] = a.trig[2 * job];
    at[4] = a.trig[2 * job + 1];
  }
  __syncthreads();
  for (bool first = true;; first = false)
  {
    const double x = at[0], y = at[1], c = at[3], s = at[4];
    double sum[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = 0.0;
    // (every thread makes the same number of trips: the waves stay whole)
    if constexpr (CELLS == 1)
    {
      for (uint32_t b0 = 0; b0 < jr.n_beams; b0 += kRefineThreads)
      {
        const uint32_t b = b0 + tid;
        const bool valid = b < jr.n_beams;
        add_terms<POW2>(grid, map, beams[valid ? b : jr.n_beams - 1u], valid, x, y, c, s, sum);
      }
    }
    else
    {
      // (n_beams <= 2^20: the item count fits 32 bits with room for the last trip's stride)
      const uint32_t n_items = CELLS * jr.n_beams;
      for (uint32_t i0 = 0; i0 < n_items; i0 += kRefineThreads)
      {
        const uint32_t i = i0 + tid;
        const bool valid = i < n_items;
        const uint32_t beam = valid ? i / CELLS : jr.n_beams - 1u;
        const double2 b = beams[beam];
        const double qx = c * b.x - s * b.y + x;
        const double qy = s * b.x + c * b.y + y;
        const uint32_t cell = valid ? neighbour_cell<POW2>(grid, qx, qy, i - beam * CELLS) : grid.ncell;
        uint32_t rank;
        // no lane of the wave holds a counting neighbour: the trip adds nothing
        if (!wave_any(map.find(cell, rank))) continue;
        add_cell_terms(map, cell, b, valid, qx, qy, c, s, sum);
      }
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = wave_sum_to_last_lane(sum[k]);
    if (lane == kWave - 1)
    {
#pragma unroll
      for (int k = 0; k < kSums; ++k) wave_sums[wave][k] = sum[k];
    }
    __syncthreads();
    if (tid == 0)
    {
      double t[kSums];
#pragma unroll
      for (int k = 0; k < kSums; ++k)
      {
        t[k] = wave_sums[0][k];
#pragma unroll
        for (uint32_t w = 1; w < kRefineWaves; ++w) t[k] += wave_sums[w][k];
      }
      const refine::Eval e{-t[0], {t[1], t[2], t[3]}, {t[4], t[5], t[6], t[7], t[8], t[9]}};
      const bool go = first ? refine::begin(st, start, e, a.rules) : refine::take(st, e, a.rules);
      if (go)
      {
        double sn, cs;
        sincos(st.trial[2], &sn, &cs);
        at[0] = st.trial[0];
        at[1] = st.trial[1];
        at[2] = st.trial[2];
        at[3] = cs;
        at[4] = sn;
      }
      more = go ? 1u : 0u;
    }
    __syncthreads();
    if (more == 0u) break;   // (uniform; the word is next written behind the next barrier)
  }
  if (tid == 0)
  {
    double * rec = a.records + static_cast<size_t>(job) * kRefineRec;
    rec[0] = st.pose[0];
    rec[1] = st.pose[1];
    rec[2] = st.pose[2];
    rec[3] = st.f_start;
    rec[4] = st.at.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) rec[5 + k] = st.at.g[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) rec[8 + k] = st.at.H[k];
    rec[14] = static_cast<double>(st.evals);
    rec[15] = static_cast<double>(st.steps);
    rec[16] = static_cast<double>(st.status);
    rec[17] = st.lambda;
  }
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_REFINE_KERNEL_H_
