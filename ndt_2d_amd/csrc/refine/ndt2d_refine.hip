// Newton NDT registration of K (scan, pose) jobs against the grid INSTALLED in the context: from
// each job's pose a damped Newton iteration on the scan's NDT score f(x, y, theta), in one upload,
// ONE kernel launch for the whole iteration of all jobs and one read-back per chunk (gfx950 /
// MI355X).  The objective, its ten sums and the iteration are the contract of include/ndt2d_hip.h
// ("Newton NDT registration"); the step between two evaluations is refine/ndt2d_refine_step.h.
//
// Every search of the library ends on the lattice (src/scan_matcher_ndt.cpp:103-143): the pose is
// quantised to the lattice's pitch.  This follows the gradient and Hessian of the same score from
// a pose -- a lattice winner, an odometry guess -- to the optimum under it.
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
// block.  InstalledSource, here, is the grid installed in the context: one grid for all jobs.  The
// loop closure refines each job on its candidate's own map with the same kernel:
// closure/ndt2d_closure.hip defines NDT2D_REFINE_KERNEL_ONLY and includes this file for its
// device half -- the kernel has one text, this one -- and instantiates it with its slots.
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
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_search.h"
#include "batch/ndt2d_batch_host.h"
#include "batch/ndt2d_refine_jobs.h"
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

// SOURCE of the grid installed in the context: one grid for all jobs, a cell is its own record.
struct InstalledSource
{
  GridDesc g;   // geometry, cells_global, occ_bits
  __device__ __forceinline__ const GridDesc & grid(uint32_t) const { return g; }
  __device__ __forceinline__ InstalledMap map(uint32_t) const { return InstalledMap{g.occ_bits, g.cells_global}; }
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

// ---- the installed grid: the object and the C entry points ----
#ifndef NDT2D_REFINE_KERNEL_ONLY

struct ndt2d_refine : ndt2d::BatchHost
{
  size_t max_jobs = 0;                // slots of a chunk
  uint32_t cells = 1;                 // the neighbourhood of a point: 1 (its own cell) or 9 (the 3 x 3 round it)
  std::vector<uint64_t> scan_first;   // scan -> its first beam within the chunk's beams (or: not sent)
  std::vector<uint32_t> sent;         // the chunk's scans in upload order
};

namespace ndt2d
{

namespace
{

using InstalledArgs = RefineArgs<InstalledSource>;

// The installed grid's instantiation <POW2, CELLS> of the kernel.  (An alias the launches could do
// without: tests/test_refine_neighbours_host.py pins the template head `<bool POW2, uint32_t CELLS>`
// to this file's text, which the kernel's own head no longer is since it gained SOURCE.  It goes
// when that pin is brought up to date.)
template <bool POW2, uint32_t CELLS>
constexpr auto installed_kernel = refine_kernel<POW2, CELLS, InstalledSource>;

// CELLS: the neighbourhood of a point, 1 or 9.
template <uint32_t CELLS>
void launch_refine(bool pow2, dim3 blocks, dim3 threads, hipStream_t stream, const InstalledArgs & a)
{
  if (pow2) hipLaunchKernelGGL((installed_kernel<true, CELLS>), blocks, threads, 0, stream, a);
  else hipLaunchKernelGGL((installed_kernel<false, CELLS>), blocks, threads, 0, stream, a);
}

struct RefineCall
{
  const double * jobs_xyt;
  const uint32_t * job_scan;   // NULL: job k uses scan k
  size_t n_jobs;
  const double * beams_xy;
  const size_t * beam_offsets;
  size_t n_scans;
  refine::Rules rules;
  size_t scan_of(size_t k) const { return job_scan != nullptr ? job_scan[k] : k; }
};

// Jobs [k0, k1) of a call whose arguments have been checked.  records_out: the call's, whole.
int refine_chunk(ndt2d_refine * s, const GridDesc & grid, size_t k0, size_t k1, const RefineCall & t, double * records_out)
{
  const size_t n_slots = k1 - k0;
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));

  // the scans this chunk's jobs name, each once, in the order the jobs first name them
  const size_t n_beams = refine_jobs::plan_sent_scans(
    n_slots, [&](size_t b) { return k0 + b; }, [&](size_t k) { return t.scan_of(k); }, t.beam_offsets, t.n_scans, s->scan_first,
    s->sent);

  // the one upload of the chunk: [beams | jobs | cos / sin pairs] (no lattice, no order table)
  const StageLayout at = stage_layout(0, 0, n_beams, n_slots, kRefineJobDoubles, 0, 2 * n_slots);
  NDT2D_BATCH_HIP(s, grow_pair(&s->h_stage, &s->d_stage, &s->stage_cap, at.total));
  NDT2D_BATCH_HIP(s, grow_pair(&s->h_out, &s->d_out, &s->out_cap, n_slots * kRefineRec));
  double * st = s->h_stage;
  for (uint32_t sc : s->sent)
  {
    std::memcpy(st + at.beams + 2 * s->scan_first[sc], t.beams_xy + 2 * t.beam_offsets[sc],
                2 * (t.beam_offsets[sc + 1] - t.beam_offsets[sc]) * sizeof(double));
  }
  for (size_t k = k0; k < k1; ++k)
  {
    const size_t sc = t.scan_of(k);
    const double * p = t.jobs_xyt + 3 * k;
    reinterpret_cast<RefineJob *>(st + at.jobs)[k - k0] =
      RefineJob{p[0], p[1], p[2], static_cast<uint32_t>(t.beam_offsets[sc + 1] - t.beam_offsets[sc]), 0u, s->scan_first[sc]};
    // cos / sin of the start heading from the host libm, as everywhere in this library
    ndt2d_cos_sin(p[2], st + at.trig + 2 * (k - k0), st + at.trig + 2 * (k - k0) + 1);
  }
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_stage, st, at.total * sizeof(double), hipMemcpyHostToDevice, stream));
  s->timed = false;
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[0], stream));

  InstalledArgs a{};
  a.source.g = grid;
  a.jobs = reinterpret_cast<const RefineJob *>(s->d_stage + at.jobs);
  a.trig = s->d_stage + at.trig;
  a.beams_xy = s->d_stage + at.beams;
  a.rules = t.rules;
  a.records = s->d_out;
  const dim3 blocks(static_cast<uint32_t>(n_slots)), threads(kRefineThreads);
  if (s->cells == 9) launch_refine<9>(grid.pow2 != 0, blocks, threads, stream, a);
  else launch_refine<1>(grid.pow2 != 0, blocks, threads, stream, a);
  NDT2D_BATCH_HIP(s, hipGetLastError());
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[1], stream));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, n_slots * kRefineRec * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[2], stream));
  NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
  s->timed = s->timing;
  std::memcpy(records_out + k0 * kRefineRec, s->h_out, n_slots * kRefineRec * sizeof(double));
  return NDT2D_OK;
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_refine_create(ndt2d_handle h, size_t max_jobs, ndt2d_refine ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || max_jobs == 0 || max_jobs > ndt2d::kRefineMaxJobs) return NDT2D_ERR_INVALID;
  ndt2d_refine * r = new ndt2d_refine();
  r->h = h;
  r->device = ndt2d_device_id(h);
  r->max_jobs = max_jobs;
  *out = r;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_refine_destroy(ndt2d_refine * r)
{
  NDT2D_C_TRY
  if (r == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::batch_drain(r);
  ndt2d::batch_release(r);
  delete r;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_refine_last_error(ndt2d_refine * r)
{
  return r != nullptr ? r->err.c_str() : "null refine";
}

int ndt2d_refine_set_timing(ndt2d_refine * r, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(r, enabled);
  NDT2D_C_CATCH(r)
}

int ndt2d_refine_last_ms(ndt2d_refine * r, float * kernel_ms, float * fetch_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(r, "refine", kernel_ms, fetch_ms);
  NDT2D_C_CATCH(r)
}

int ndt2d_refine_set_neighbourhood(ndt2d_refine * r, uint32_t cells)
{
  NDT2D_C_TRY
  if (r == nullptr) return NDT2D_ERR_INVALID;
  if (cells != 1 && cells != 9)
  {
    return batch_fail(r, NDT2D_ERR_INVALID, "ndt2d_refine_set_neighbourhood: " + std::to_string(cells) + " cells (1 or 9)");
  }
  r->cells = cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

int ndt2d_refine_neighbourhood(ndt2d_refine * r, uint32_t * out)
{
  NDT2D_C_TRY
  if (r == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = r->cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

int ndt2d_refine_covariance(const double * H6, double * cov9_out)
{
  NDT2D_C_TRY
  if (H6 == nullptr || cov9_out == nullptr) return NDT2D_ERR_INVALID;
  const double H[6] = {H6[0], H6[1], H6[2], H6[3], H6[4], H6[5]};
  double cov[9];
  if (!ndt2d::refine::covariance(H, cov)) return NDT2D_ERR_STATE;   // not positive definite, or not finite
  std::memcpy(cov9_out, cov, sizeof(cov));
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_refine_run(ndt2d_refine * r, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                     const double * beams_xy, const size_t * beam_offsets, size_t n_scans, uint32_t max_evals,
                     double tol_lin, double tol_ang, double * records_out)
{
  NDT2D_C_TRY
  if (r == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  if (jobs_xyt == nullptr || records_out == nullptr || beams_xy == nullptr || beam_offsets == nullptr)
  {
    return batch_fail(r, NDT2D_ERR_INVALID, "ndt2d_refine_run: null argument");
  }
  // the rules, every scan and every job are checked before anything is launched
  const std::string refusal = ndt2d::refine_jobs::refusal("ndt2d_refine_run", jobs_xyt, job_scan, n_jobs, beam_offsets, n_scans,
                                                         max_evals, tol_lin, tol_ang);
  if (!refusal.empty()) return batch_fail(r, NDT2D_ERR_INVALID, refusal);
  int rc = NDT2D_OK;
  const ndt2d::GridDesc grid = ndt2d::installed_grid(r->h, &rc);
  if (rc != NDT2D_OK)
  {
    return batch_fail(r, rc, std::string("ndt2d_refine_run") + (rc == NDT2D_ERR_NO_GRID ? ": no grid"
                                                                : rc == NDT2D_ERR_STATE ? ": the installed grid has no records"
                                                                                        : ": no grid view"));
  }
  NDT2D_BATCH_HIP(r, hipSetDevice(r->device));
  const ndt2d::RefineCall t{jobs_xyt, job_scan, n_jobs, beams_xy, beam_offsets, n_scans, {max_evals, tol_lin, tol_ang}};
  // more jobs than slots: in chunks
  for (size_t k0 = 0; k0 < n_jobs; k0 += r->max_jobs)
  {
    rc = ndt2d::refine_chunk(r, grid, k0, std::min(n_jobs, k0 + r->max_jobs), t, records_out);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

}  // extern "C"

#endif  // NDT2D_REFINE_KERNEL_ONLY: the object and the entry points of the installed grid
