// The kernel of the match verification, once (verify/ndt2d_verify.hip: K (scan, pose) jobs on the
// installed grid; closure/ndt2d_closure.hip: jobs on the loop closure's candidate maps), with what
// every call of it shares on the host: its job record and arguments, the settings of an object
// with their validation, the call's arrays and the layout of what comes back (gfx950 / MI355X).
// The classes, the ray and the records are the contract of include/ndt2d_hip.h ("Match
// verification"); the line walk and the closest approach are verify/ndt2d_verify_ray.h.
//
//   verify_kernel<POW2, CELLS>   grid (job of the chunk), 256 threads.  Thread t takes beams t,
//       t + 256, ... of the job's scan: the point through cell_index, its neighbourhood (CELLS = 1:
//       its own cell; 9: the 3 x 3 round it, clipped on (gx, gy)) through InstalledMap::find /
//       record_exponent of the shared device functions for the smallest m2, then -- rays enabled,
//       the beam on the grid, the job's origin cell on the grid -- the cells of the integer line
//       from the origin cell towards the beam's own.  Of a cell on the line the occupancy bit is
//       read first (one word): an empty cell, four in five in a room, costs the line's integer
//       step and that load; only a cell that can score has its record loaded and the closest
//       approach computed.  The walk ends at the first piercing cell, or where the line enters the
//       end's own 3 x 3 (the Chebyshev distance to the end never grows along the line), and never
//       makes more than dx - dy + 1 trips: the bound is computed before the loop.
//       The counts: every trip, each wave takes the lane masks of its classes (ballot) and adds
//       their popcounts to six wave-uniform counters; lane 0 of each wave leaves them in LDS,
//       thread 0 adds the four waves' and writes the job's record.
//
// The map is a template argument of the kernel, as of refine_kernel: a SOURCE gives, for the slot
// a job's record names, the GridDesc of that job's map and its map object (find(cell, rank) /
// record(rank)); both are uniform over the block.  InstalledSource (batch/ndt2d_installed_map.h) is
// the grid installed in the context: one grid for all jobs, verify/ndt2d_verify.hip.
// closure/ndt2d_closure.hip includes this header too and instantiates the kernel on its candidate
// slots (SlotSource): one text for both.
//
// The beams are read from the chunk's upload, once each.  LDS holds the waves' counters only.
//
// Off the grid.  cell_index gives ncell for every point outside the grid (NaN and infinite ones
// included), bit ncell of the bitmap is 0 and record ncell exists, so no lane indexes beyond
// either.  A line runs between two cells of the grid and stays inside their bounding box: every
// cell it visits is on the grid.  A job's beams are read at [beam_first, beam_first + n_beams) of
// the chunk's upload and its per-beam results written at [out_first, out_first + n_beams) of the
// chunk's arrays only; both come from the host's table.
//
// Determinism.  A beam's byte, m2 and cells are its lane's own; the counts are integers.  No block
// waits for another, __syncthreads is the only barrier, stream order the only ordering between the
// upload, the launch and the read-back; no polls, no atomics.
//
// LDS: 4 x 6 counters, 96 bytes.  Registers and scratch: DESIGN.md 3.15.
// Included by the .hip translation units only.
#ifndef NDT2D_VERIFY_KERNEL_H_
#define NDT2D_VERIFY_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "ndt2d_hip.h"
#include "batch/ndt2d_installed_map.h"
#include "batch/ndt2d_refine_jobs.h"
#include "verify/ndt2d_verify_ray.h"

namespace ndt2d
{

namespace
{

constexpr uint32_t kVerifyThreads = 256;
constexpr uint32_t kVerifyWaves = kVerifyThreads / kWave;
constexpr uint32_t kVerifyMaxJobs = 4096;          // blocks of a launch
constexpr size_t kVerifyChunkBeams = size_t(1) << 24;   // per-beam results of one chunk (a job more is taken whole)
constexpr size_t kVerifyRec = NDT2D_VERIFY_RECORD_U32;
constexpr int kCounters = 6;   // off, unseen, outlier, inlier, pierced, walked

// One job of a chunk.
struct VerifyJob
{
  double x, y;
  uint32_t n_beams;      // of its scan
  uint32_t slot;         // of its map within the chunk (the installed grid: 0)
  uint64_t beam_first;   // its scan's first beam within the chunk's beams
  uint64_t out_first;    // its first beam within the chunk's per-beam results
};
constexpr size_t kVerifyJobDoubles = 5;
static_assert(sizeof(VerifyJob) == kVerifyJobDoubles * sizeof(double), "jobs travel in a buffer of doubles");

struct VerifyRules
{
  double gate_inlier, gate_pierce;
  uint32_t rays;   // 0: no ray is walked
};

template <class SOURCE>
struct VerifyArgs
{
  SOURCE source;              // job -> its map
  const VerifyJob * jobs;     // [job of the chunk]
  const double * trig;        // [job of the chunk][2]: cos, sin of its heading (host libm)
  const double * beams_xy;    // the chunk's scans, [beam][2] robot frame
  VerifyRules rules;
  uint32_t * records;         // [job of the chunk][NDT2D_VERIFY_RECORD_U32]
  // per beam of the chunk's jobs, each optional
  uint8_t * beam_class;
  double * beam_m2;
  uint32_t * beam_cells;      // [.][2]
};

// m2 = d^T I d of the point against the record: -2 x Cell::score's exponent (I = -2 h exactly).
__device__ __forceinline__ double record_m2(const double2 * r, double qx, double qy)
{
  const double2 m = r[0], h0 = r[1], h1 = r[2];
  return -2.0 * record_exponent(m.x, m.y, h0.x, h0.y, h1.x, qx, qy);
}

// SOURCE: where a job's map comes from (above).
template <bool POW2, uint32_t CELLS, class SOURCE>
__global__ void __launch_bounds__(kVerifyThreads) verify_kernel(const VerifyArgs<SOURCE> a)
{
  __shared__ uint32_t wave_counts[kVerifyWaves][kCounters];
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const uint32_t job = blockIdx.x;
  const VerifyJob jr = a.jobs[job];   // (uniform over the block)
  const GridDesc & grid = a.source.grid(jr.slot);
  const auto map = a.source.map(jr.slot);
  const double2 * beams = reinterpret_cast<const double2 *>(a.beams_xy) + jr.beam_first;
  const double c = a.trig[2 * job], s = a.trig[2 * job + 1];
  const double gate_inlier = a.rules.gate_inlier, gate_pierce = a.rules.gate_pierce;
  // the job's origin cell (uniform): off the grid, no ray of the job is walked
  const uint32_t origin = cell_index<POW2>(grid, jr.x, jr.y);
  const bool walk_job = (a.rules.rays != 0u) & (origin < grid.ncell);
  const int32_t oy = static_cast<int32_t>(origin / grid.size_x);
  const int32_t ox = static_cast<int32_t>(origin - static_cast<uint32_t>(oy) * grid.size_x);

  uint32_t count[kCounters];   // (wave-uniform: sums of popcounts)
#pragma unroll
  for (int k = 0; k < kCounters; ++k) count[k] = 0u;

  // (every thread makes the same number of trips: the waves stay whole for the ballots)
  for (uint32_t b0 = 0; b0 < jr.n_beams; b0 += kVerifyThreads)
  {
    const uint32_t b = b0 + tid;
    const bool valid = b < jr.n_beams;
    const double2 p = beams[valid ? b : jr.n_beams - 1u];
    const double qx = c * p.x - s * p.y + jr.x;
    const double qy = s * p.x + c * p.y + jr.y;
    const uint32_t own = cell_index<POW2>(grid, qx, qy);   // ncell: off the grid
    const bool off = own >= grid.ncell;
    const uint32_t gy = own / grid.size_x, gx = own - gy * grid.size_x;

    // the smallest m2 over the counting cells of the neighbourhood, ties to the lowest j
    double m2 = HUGE_VAL;
    uint32_t won = NDT2D_VERIFY_NO_CELL;
    if constexpr (CELLS == 1)
    {
      uint32_t rank;
      if (map.find(own, rank))   // (bit ncell is 0)
      {
        m2 = record_m2(map.record(rank), qx, qy);
        won = own;
      }
    }
    else
    {
      for (uint32_t j = 0; j < CELLS; ++j)
      {
        // (unsigned: gx + dx = -1 wraps to 2^32 - 1 and fails the same compare as gx + dx = size_x)
        const uint32_t nx = gx + (j % 3u) - 1u, ny = gy + (j / 3u) - 1u;
        const bool on = !off & (nx < grid.size_x) & (ny < grid.size_y);
        const uint32_t cell = on ? ny * grid.size_x + nx : grid.ncell;
        uint32_t rank;
        if (!map.find(cell, rank)) continue;
        const double v = record_m2(map.record(rank), qx, qy);
        // below the held one, or NaN while the held one is not (a NaN stays)
        if (won == NDT2D_VERIFY_NO_CELL || ((m2 == m2) & !(v >= m2)))
        {
          m2 = v;
          won = cell;
        }
      }
    }
    const bool seen = won != NDT2D_VERIFY_NO_CELL;
    const uint32_t cls = off ? NDT2D_BEAM_OFF : !seen ? NDT2D_BEAM_UNSEEN : (m2 <= gate_inlier) ? NDT2D_BEAM_INLIER : NDT2D_BEAM_OUTLIER;

    // the ray: origin cell -> the beam's own cell
    const bool walked = walk_job & valid & !off;
    uint32_t pierced_cell = NDT2D_VERIFY_NO_CELL;
    if (walked)
    {
      const double ux = qx - jr.x, uy = qy - jr.y;
      verify::Line l = verify::line_begin(ox, oy, static_cast<int32_t>(gx), static_cast<int32_t>(gy));
      const uint32_t max_cells = l.max_cells;   // dx - dy + 1, computed up front: the loop's bound
      for (uint32_t trip = 0; trip < max_cells; ++trip)
      {
        if (verify::line_to_end(l) <= 1) break;   // the end's own 3 x 3: nothing from here on is tested
        if (verify::line_cell_testable(l, ox, oy))
        {
          const uint32_t cell = static_cast<uint32_t>(l.y) * grid.size_x + static_cast<uint32_t>(l.x);
          uint32_t rank;
          if (map.find(cell, rank))   // the occupancy bit first: an empty cell ends here
          {
            const double2 * r = map.record(rank);
            const double2 m = r[0], h0 = r[1], h1 = r[2];
            const double rIr = verify::approach(ux, uy, m.x - jr.x, m.y - jr.y, -2.0 * h0.x, -2.0 * h0.y, -2.0 * h1.x);
            if (verify::pierces(rIr, gate_pierce))
            {
              pierced_cell = cell;
              break;
            }
          }
        }
        if (!verify::line_next(l)) break;
      }
    }
    const bool pierced = pierced_cell != NDT2D_VERIFY_NO_CELL;

    if (valid)
    {
      const uint64_t at = jr.out_first + b;
      if (a.beam_class != nullptr) a.beam_class[at] = static_cast<uint8_t>(cls | (pierced ? NDT2D_BEAM_PIERCED : 0u));
      if (a.beam_m2 != nullptr) a.beam_m2[at] = seen ? m2 : HUGE_VAL;
      if (a.beam_cells != nullptr)
      {
        reinterpret_cast<uint2 *>(a.beam_cells)[at] = uint2{won, pierced_cell};
      }
    }
    count[0] += __popcll(__builtin_amdgcn_ballot_w64(valid & (cls == NDT2D_BEAM_OFF)));
    count[1] += __popcll(__builtin_amdgcn_ballot_w64(valid & (cls == NDT2D_BEAM_UNSEEN)));
    count[2] += __popcll(__builtin_amdgcn_ballot_w64(valid & (cls == NDT2D_BEAM_OUTLIER)));
    count[3] += __popcll(__builtin_amdgcn_ballot_w64(valid & (cls == NDT2D_BEAM_INLIER)));
    count[4] += __popcll(__builtin_amdgcn_ballot_w64(pierced));
    count[5] += __popcll(__builtin_amdgcn_ballot_w64(walked));
  }
  if (lane == 0)
  {
#pragma unroll
    for (int k = 0; k < kCounters; ++k) wave_counts[wave][k] = count[k];
  }
  __syncthreads();
  if (tid == 0)
  {
    uint32_t * rec = a.records + static_cast<size_t>(job) * kVerifyRec;
    rec[0] = jr.n_beams;
#pragma unroll
    for (int k = 0; k < kCounters; ++k)
    {
      uint32_t t = wave_counts[0][k];
#pragma unroll
      for (uint32_t w = 1; w < kVerifyWaves; ++w) t += wave_counts[w][k];
      rec[1 + k] = t;
    }
    rec[7] = 0u;
  }
}

// ---- what every call of the kernel shares on the host ----

// The settings of an object that verifies (ndt2d_verify, ndt2d_closure: one each).  A setter takes
// the value, or returns what it refuses about it in the words of the entry point `entry`.
struct VerifySettings
{
  uint32_t cells = 1;   // the neighbourhood of a point: 1 (its own cell) or 9 (the 3 x 3 round it)
  double gate_inlier = 9.0, gate_pierce = 1.0;
  bool rays = true;
  VerifyRules rules() const { return VerifyRules{gate_inlier, gate_pierce, rays ? 1u : 0u}; }
  std::string set_cells(const char * entry, uint32_t n)
  {
    if (n != 1 && n != 9) return std::string(entry) + ": " + std::to_string(n) + " cells (1 or 9)";
    cells = n;
    return std::string();
  }
  std::string set_gates(const char * entry, double inlier, double pierce)
  {
    if (!(inlier >= 0.0) || !(pierce >= 0.0) || !std::isfinite(inlier) || !std::isfinite(pierce))
    {
      return std::string(entry) + ": a gate is negative or not finite";
    }
    gate_inlier = inlier;
    gate_pierce = pierce;
    return std::string();
  }
  std::string set_rays(const char * entry, int enabled)
  {
    if (enabled != 0 && enabled != 1) return std::string(entry) + ": " + std::to_string(enabled) + " (0 or 1)";
    rays = enabled != 0;
    return std::string();
  }
};

// A verification's jobs and scans (batch/ndt2d_refine_jobs.h) and where its results go.
struct VerifyCall : refine_jobs::JobList
{
  uint32_t * records_out;
  uint8_t * beam_class_out;
  double * beam_m2_out;
  uint32_t * beam_cells_out;
};

// Where what comes back lies in the out pair (doubles): [records | m2 | cells | classes], the
// per-beam pieces only where the caller wants them.
struct VerifyOutLayout
{
  size_t m2, cells, classes, total;
};

VerifyOutLayout verify_out_layout(size_t n_slots, size_t n_out, const VerifyCall & t)
{
  VerifyOutLayout l;
  l.m2 = n_slots * kVerifyRec / 2;
  l.cells = l.m2 + (t.beam_m2_out != nullptr ? n_out : 0);
  l.classes = l.cells + (t.beam_cells_out != nullptr ? n_out : 0);
  l.total = l.classes + (t.beam_class_out != nullptr ? (n_out + 7) / 8 : 0);
  return l;
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_VERIFY_KERNEL_H_
