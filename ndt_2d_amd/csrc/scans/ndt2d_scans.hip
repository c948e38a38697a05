// Batched scan tracking: K jobs, each a (scan, pose) pair, against the grid INSTALLED in the
// context -- a full matchScan lattice around each job's pose with the job's OWN beams, in one
// upload, the search launches, one reduction launch and one read-back per chunk (gfx950 / MI355X).
//
// Reference: localisation by scan matching (src/ndt_mapper.cpp:547-566): matchScan(scan,
// correction, covariance) on the global matcher, the correction added to the scan's pose
// (:557-561).  A fleet of robots on one shared map, a recorded bag replayed against a loaded map,
// or every scan of a graph re-matched after solver_->optimize (:680) is that branch for many
// scans: sequentially one upload, one search launch and one host round trip per scan, each search
// a lattice that fills a fraction of the chip.  closure/ batches one scan against K maps, starts/
// one scan from K poses; here the slots differ in their beams:
//
//   scans_search_kernel   grid (theta step, job of the launch's group), a lane per (dx, dy), as
//       wide as the translation lattice (wider lattices loop).  The block looks its job up in the
//       group's index table, takes the job's beam pointer and count, its (x, y) and its heading's
//       cos / sin row (host libm), and walks ../closure/ndt2d_walk_fn.h lane_walk<C, POW2> on the
//       installed grid, as starts/ does.  C, the number of partial sums, follows from the beam
//       count of the job's scan (../closure/ndt2d_sum_chunks.h) and is a template parameter of
//       the walk, so the jobs of a chunk are grouped by C (ndt2d_job_groups.h) and a chunk is one
//       launch per C present: one when the scans are subsampled to one count, eight at most.
//       Records and scores are written by job, in the caller's order, whatever the grouping.
//   scans_reduce_kernel   one block per job: the n_theta records of its blocks ->
//       {best_score, best_index (+0.5: near tie), acc[10]} with merge_best, fixed order.
//
// Several jobs may name one scan (a heading fan per robot): its beams travel once.  A scan no job
// of the chunk names is not uploaded.
//
// Off the grid.  As starts/: cell_index gives ncell for every point outside the grid, bit ncell
// of the bitmap is 0 and record ncell exists, so no lane indexes beyond either.  A job's beams
// are read at [beam_first, beam_first + n_beams) of the chunk's upload only; both come from the
// host's table, checked against the offsets before anything is launched.
//
// The bits of a raw score are those of closure/ and starts/: the same walk, the same C for the
// same beam count -- the sequential search's bits wherever it runs the small-lattice search with
// its default plan.
//
// Determinism.  As starts/: a lane's sums are its own, blocks reduce lanes over the DPP network
// and waves in wave order, the reducing block takes records r, r + 256, ... per thread.  Stream
// order is the only ordering between the launches and __syncthreads the only barrier inside
// them; no polls, no atomics.  A job's bits depend on its scan, its pose and the grid alone: not
// on the other jobs, the grouping or the chunking.
//
// LDS of the search block: kStageBeams x {ox, oy} = 16 KB, reused for one record per wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "../closure/ndt2d_walk_fn.h"
#include "ndt2d_job_groups.h"

namespace ndt2d
{

namespace
{

// One job of a chunk.
struct JobRec
{
  double x, y;
  uint32_t trig_row;     // its heading's row of the cos / sin table
  uint32_t n_beams;      // of its scan
  uint64_t beam_first;   // its scan's first beam within the chunk's beams
};
static_assert(sizeof(JobRec) == 4 * sizeof(double), "jobs travel in a buffer of doubles");

struct ScansSearchArgs
{
  GridDesc grid;             // geometry, cells_global, occ_bits
  const JobRec * jobs;       // [job of the chunk]
  const uint32_t * order;    // launch position -> job (ndt2d_job_groups.h)
  const double * trig;       // [rows][2][n_th]: cos | sin of (heading + dth[i])
  const double * beams_xy;   // the chunk's scans, [beam][2] robot frame
  const double * dth, * dlin;
  uint32_t first;            // launch position of the group's first job
  uint32_t n_th, n_lin;
  double * scores;           // optional: [job][n_th * n_lin * n_lin]
  double * partials;         // [job][n_th][kRecord]
};

// The installed grid as the lane's walk reads it: a cell is its own record.
struct InstalledMap
{
  const uint32_t * occ_bits;
  const double * cells_global;
  __device__ __forceinline__ bool find(uint32_t cell, uint32_t & rank) const
  {
    rank = cell;   // (<= ncell: bit ncell is 0)
    return ((occ_bits[cell >> 5] >> (cell & 31u)) & 1u) != 0u;
  }
  __device__ __forceinline__ const double2 * record(uint32_t rank) const
  {
    return reinterpret_cast<const double2 *>(cells_global + static_cast<size_t>(rank) * kCellStrideGlobal);
  }
};

template <int C, bool POW2>
__global__ void __launch_bounds__(kSearchMaxThreads) scans_search_kernel(const ScansSearchArgs a)
{
  __shared__ double2 rows[kStageBeams];
  const uint32_t ith = blockIdx.x;
  const uint32_t job = a.order[a.first + blockIdx.y];   // (uniform over the block)
  const uint32_t tid = threadIdx.x, n_threads = blockDim.x;
  const JobRec s = a.jobs[job];
  const InstalledMap map{a.grid.occ_bits, a.grid.cells_global};
  const double * beams = a.beams_xy + 2 * s.beam_first;
  const double * trig = a.trig + static_cast<size_t>(s.trig_row) * 2 * a.n_th;
  const double ct = trig[ith], st = trig[a.n_th + ith], dt = a.dth[ith];
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
    const double sum = lane_walk<C, POW2>(a.grid, map, rows, beams, s.n_beams, ct, st, s.x, s.y, dx, dy, valid);
    if (valid)
    {
      const double score = -sum;  // (:127)
      lane_take(score, static_cast<uint64_t>(ith) * n_cand + c, dx, dy, dt, best_s, best_i, acc);
      if (a.scores != nullptr) a.scores[(static_cast<uint64_t>(job) * a.n_th + ith) * n_cand + c] = score;
    }
  }
  // the block's record (the rows are free behind block_record's first barrier)
  block_record<false>(best_s, best_i, acc, reinterpret_cast<double *>(rows),
                      a.partials + (static_cast<size_t>(job) * a.n_th + ith) * kRecord);
}

// partials[job][n_th][kRecord] -> out[job][kRecord]
__global__ void __launch_bounds__(kReduceThreads) scans_reduce_kernel(const double * partials, uint32_t n_th,
                                                                       double * out)
{
  __shared__ double scratch[(kReduceThreads / 64) * kRecord];
  const uint32_t job = blockIdx.x;
  reduce_slot_records(partials + static_cast<size_t>(job) * n_th * kRecord, n_th, scratch,
                      out + static_cast<size_t>(job) * kRecord);
}

template <bool POW2>
void launch_search_c(uint32_t chunks, dim3 grid, dim3 block, hipStream_t stream, const ScansSearchArgs & a)
{
  switch (chunks)
  {
    case 1: hipLaunchKernelGGL((scans_search_kernel<1, POW2>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((scans_search_kernel<2, POW2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((scans_search_kernel<3, POW2>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((scans_search_kernel<4, POW2>), grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL((scans_search_kernel<5, POW2>), grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL((scans_search_kernel<6, POW2>), grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL((scans_search_kernel<7, POW2>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((scans_search_kernel<8, POW2>), grid, block, 0, stream, a); break;
  }
}

}  // namespace

}  // namespace ndt2d

// ---- the object and the C entry points ----

struct ndt2d_scans
{
  ndt2d_handle h = nullptr;
  int device = 0;
  size_t max_jobs = 0;
  std::string err;
  // one upload per chunk: [dth | dlin | beams of the chunk's scans | jobs | order | cos / sin rows]
  // (doubles), pinned and on the device
  double * h_stage = nullptr, * d_stage = nullptr;
  size_t stage_cap = 0;
  void * d_partials = nullptr;
  size_t partials_cap = 0;   // bytes
  // what comes back: [job][12] records | [job][lattice] scores (doubles), on the device and pinned
  double * d_out = nullptr, * h_out = nullptr;
  size_t out_cap = 0;
  std::vector<double> trig;                        // the chunk's cos / sin rows
  std::unordered_map<uint64_t, uint32_t> row_of;   // heading (bits) -> row
  std::vector<uint64_t> scan_first;                // scan -> its first beam within the chunk's beams (kNotSent: not sent)
  std::vector<uint32_t> sent, job_beams;           // the chunk's scans in upload order; beams per job
  ndt2d::JobGroups groups;
  bool timing = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // before the searches, behind them, behind the reduction
  bool timed = false;
};

namespace
{

using ndt2d::GridDesc;
using ndt2d::JobRec;
constexpr size_t kRec = NDT2D_MATCH_RECORD_DOUBLES;
constexpr size_t kMaxScanBeams = size_t(1) << 20;   // what ndt2d_set_beams takes
constexpr uint64_t kNotSent = ~uint64_t(0);
// all_scores wanted: jobs of one chunk, so that the scores on their way back stay within this
constexpr size_t kScoreDoublesPerLaunch = size_t(8) << 20;

void guard_note(ndt2d_scans * s, const char * what) noexcept
{
  if (s == nullptr) return;
  try
  {
    s->err = what;
  }
  catch (...)
  {
  }
}
void guard_note(std::nullptr_t, const char *) noexcept {}

int sfail(ndt2d_scans * s, int code, const std::string & msg)
{
  if (s != nullptr) s->err = msg;
  return code;
}

int sfail_hip(ndt2d_scans * s, hipError_t e, const char * what)
{
  (void)hipGetLastError();  // clear sticky state
  return sfail(s, NDT2D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define NDT2D_SCANS_HIP(s, call)                            \
  do                                                        \
  {                                                         \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return sfail_hip(s, e__, #call); \
  } while (0)

// A pinned / device pair of at least `doubles` (contents are not kept).
hipError_t grow_pair(double ** host, double ** dev, size_t * cap, size_t doubles)
{
  if (doubles <= *cap) return hipSuccess;
  *cap = 0;
  if (*host != nullptr) (void)hipHostFree(*host);
  if (*dev != nullptr) (void)hipFree(*dev);
  *host = nullptr;
  *dev = nullptr;
  const size_t want = doubles + doubles / 4 + 512;
  hipError_t e = hipHostMalloc(reinterpret_cast<void **>(host), want * sizeof(double), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(dev), want * sizeof(double));
  if (e == hipSuccess) *cap = want;
  return e;
}

void free_scans(ndt2d_scans * s)
{
  (void)hipSetDevice(s->device);
  if (s->h_stage != nullptr) (void)hipHostFree(s->h_stage);
  if (s->d_stage != nullptr) (void)hipFree(s->d_stage);
  if (s->d_partials != nullptr) (void)hipFree(s->d_partials);
  if (s->d_out != nullptr) (void)hipFree(s->d_out);
  if (s->h_out != nullptr) (void)hipHostFree(s->h_out);
  for (hipEvent_t ev : s->ev)
  {
    if (ev != nullptr) (void)hipEventDestroy(ev);
  }
  delete s;
}

// A call's arguments, checked.
struct ScansCall
{
  const double * jobs_xyt;
  const uint32_t * job_scan;   // NULL: job k uses scan k
  const double * beams_xy;
  const size_t * beam_offsets;
  size_t n_scans;
  const double * dth;
  size_t n_th;
  const double * dlin;
  size_t n_lin;
  size_t scan_of(size_t k) const { return job_scan != nullptr ? job_scan[k] : k; }
};

// Jobs [k0, k1) of a call whose arguments have been checked.  records_out / all_scores: the call's, whole.
int match_chunk(ndt2d_scans * s, const GridDesc & grid, size_t k0, size_t k1, const ScansCall & t,
                double * records_out, double * all_scores)
{
  const size_t n_slots = k1 - k0;
  const size_t n_lattice = t.n_th * t.n_lin * t.n_lin;
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));

  // the scans this chunk's jobs name, each once, in the order the jobs first name them
  s->scan_first.assign(t.n_scans, kNotSent);
  s->sent.clear();
  s->job_beams.resize(n_slots);
  size_t n_beams = 0;
  for (size_t k = k0; k < k1; ++k)
  {
    const size_t sc = t.scan_of(k);
    const size_t count = t.beam_offsets[sc + 1] - t.beam_offsets[sc];
    if (s->scan_first[sc] == kNotSent)
    {
      s->scan_first[sc] = n_beams;
      s->sent.push_back(static_cast<uint32_t>(sc));
      n_beams += count;
    }
    s->job_beams[k - k0] = static_cast<uint32_t>(count);
  }
  ndt2d::group_jobs(s->job_beams.data(), n_slots, s->groups);

  // cos / sin of (heading + dth[i]) from the host libm (:106-107), a row per distinct heading
  s->row_of.clear();
  s->trig.clear();
  std::vector<uint32_t> rows(n_slots);
  for (size_t k = k0; k < k1; ++k)
  {
    const double theta = t.jobs_xyt[3 * k + 2];
    uint64_t bits;
    std::memcpy(&bits, &theta, sizeof(bits));
    auto it = s->row_of.find(bits);
    if (it == s->row_of.end())
    {
      const uint32_t row = static_cast<uint32_t>(s->trig.size() / (2 * t.n_th));
      it = s->row_of.emplace(bits, row).first;
      s->trig.resize(s->trig.size() + 2 * t.n_th);
      double * c = s->trig.data() + static_cast<size_t>(row) * 2 * t.n_th;
      for (size_t i = 0; i < t.n_th; ++i) ndt2d_cos_sin(theta + t.dth[i], c + i, c + t.n_th + i);
    }
    rows[k - k0] = it->second;
  }

  // [dth | dlin | beams | jobs | order | cos / sin rows]
  const size_t off_beams = (t.n_th + t.n_lin + 1) & ~size_t(1);   // (beams: 16-byte loads)
  const size_t off_jobs = off_beams + 2 * n_beams;
  const size_t off_order = off_jobs + n_slots * (sizeof(JobRec) / sizeof(double));
  const size_t off_trig = off_order + (n_slots + 1) / 2;           // (two 32-bit entries to a double)
  const size_t n_stage = off_trig + s->trig.size();
  NDT2D_SCANS_HIP(s, grow_pair(&s->h_stage, &s->d_stage, &s->stage_cap, n_stage));
  const size_t partial_bytes = n_slots * t.n_th * kRec * sizeof(double);
  if (partial_bytes > s->partials_cap)
  {
    if (s->d_partials != nullptr) (void)hipFree(s->d_partials);
    s->d_partials = nullptr;
    s->partials_cap = 0;
    const size_t want = partial_bytes + partial_bytes / 4;
    NDT2D_SCANS_HIP(s, hipMalloc(&s->d_partials, want));
    s->partials_cap = want;
  }
  const size_t n_out = n_slots * (kRec + (all_scores != nullptr ? n_lattice : 0));
  NDT2D_SCANS_HIP(s, grow_pair(&s->h_out, &s->d_out, &s->out_cap, n_out));

  double * st = s->h_stage;
  std::memcpy(st, t.dth, t.n_th * sizeof(double));
  std::memcpy(st + t.n_th, t.dlin, t.n_lin * sizeof(double));
  for (uint32_t sc : s->sent)
  {
    std::memcpy(st + off_beams + 2 * s->scan_first[sc], t.beams_xy + 2 * t.beam_offsets[sc],
                2 * (t.beam_offsets[sc + 1] - t.beam_offsets[sc]) * sizeof(double));
  }
  JobRec * recs = reinterpret_cast<JobRec *>(st + off_jobs);
  for (size_t k = k0; k < k1; ++k)
  {
    recs[k - k0] = JobRec{t.jobs_xyt[3 * k], t.jobs_xyt[3 * k + 1], rows[k - k0], s->job_beams[k - k0],
                          s->scan_first[t.scan_of(k)]};
  }
  st[off_trig - 1] = 0.0;   // (the odd entry's other half)
  std::memcpy(st + off_order, s->groups.order.data(), n_slots * sizeof(uint32_t));
  std::memcpy(st + off_trig, s->trig.data(), s->trig.size() * sizeof(double));

  // the one upload of the chunk
  NDT2D_SCANS_HIP(s, hipMemcpyAsync(s->d_stage, st, n_stage * sizeof(double), hipMemcpyHostToDevice, stream));
  s->timed = false;
  if (s->timing) NDT2D_SCANS_HIP(s, hipEventRecord(s->ev[0], stream));

  ndt2d::ScansSearchArgs a{};
  a.grid = grid;
  a.jobs = reinterpret_cast<const JobRec *>(s->d_stage + off_jobs);
  a.order = reinterpret_cast<const uint32_t *>(s->d_stage + off_order);
  a.trig = s->d_stage + off_trig;
  a.beams_xy = s->d_stage + off_beams;
  a.dth = s->d_stage;
  a.dlin = s->d_stage + t.n_th;
  a.n_th = static_cast<uint32_t>(t.n_th);
  a.n_lin = static_cast<uint32_t>(t.n_lin);
  a.scores = all_scores != nullptr ? s->d_out + n_slots * kRec : nullptr;
  a.partials = static_cast<double *>(s->d_partials);
  const size_t n_cand = t.n_lin * t.n_lin;
  const uint32_t threads = static_cast<uint32_t>(std::min<size_t>(ndt2d::kSearchMaxThreads, (n_cand + 63) & ~size_t(63)));
  // a launch per C present: its blocks find their jobs through order[first ..]
  for (uint32_t g = 0; g < s->groups.n_groups; ++g)
  {
    a.first = s->groups.first[g];
    const dim3 grid_dim(static_cast<uint32_t>(t.n_th), s->groups.first[g + 1] - s->groups.first[g]);
    if (grid.pow2) ndt2d::launch_search_c<true>(s->groups.chunks[g], grid_dim, dim3(threads), stream, a);
    else ndt2d::launch_search_c<false>(s->groups.chunks[g], grid_dim, dim3(threads), stream, a);
    NDT2D_SCANS_HIP(s, hipGetLastError());
  }
  if (s->timing) NDT2D_SCANS_HIP(s, hipEventRecord(s->ev[1], stream));

  hipLaunchKernelGGL(ndt2d::scans_reduce_kernel, dim3(static_cast<uint32_t>(n_slots)), dim3(ndt2d::kReduceThreads), 0,
                     stream, a.partials, a.n_th, s->d_out);
  NDT2D_SCANS_HIP(s, hipGetLastError());
  if (s->timing) NDT2D_SCANS_HIP(s, hipEventRecord(s->ev[2], stream));
  // the one read-back of the chunk
  NDT2D_SCANS_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, stream));
  NDT2D_SCANS_HIP(s, hipStreamSynchronize(stream));
  s->timed = s->timing;
  std::memcpy(records_out + k0 * kRec, s->h_out, n_slots * kRec * sizeof(double));
  if (all_scores != nullptr)
  {
    std::memcpy(all_scores + k0 * n_lattice, s->h_out + n_slots * kRec, n_slots * n_lattice * sizeof(double));
  }
  return NDT2D_OK;
}

}  // namespace

extern "C" {

int ndt2d_scans_create(ndt2d_handle h, size_t max_jobs, ndt2d_scans ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || max_jobs == 0 || max_jobs > 4096) return NDT2D_ERR_INVALID;
  ndt2d_scans * s = new ndt2d_scans();
  s->h = h;
  s->device = ndt2d_device_id(h);
  s->max_jobs = max_jobs;
  *out = s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_scans_destroy(ndt2d_scans * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(s->h)));
  free_scans(s);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_scans_last_error(ndt2d_scans * s)
{
  return s != nullptr ? s->err.c_str() : "null scans";
}

int ndt2d_scans_set_timing(ndt2d_scans * s, int enabled)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (enabled != 0 && s->ev[0] == nullptr)
  {
    NDT2D_SCANS_HIP(s, hipSetDevice(s->device));
    for (hipEvent_t & ev : s->ev) NDT2D_SCANS_HIP(s, hipEventCreate(&ev));
  }
  s->timing = enabled != 0;
  s->timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_scans_last_ms(ndt2d_scans * s, float * search_ms, float * reduce_ms)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (!s->timed) return sfail(s, NDT2D_ERR_STATE, "ndt2d_scans_last_ms: no timed match (ndt2d_scans_set_timing)");
  float a = 0.0f, b = 0.0f;
  NDT2D_SCANS_HIP(s, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  NDT2D_SCANS_HIP(s, hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
  if (search_ms != nullptr) *search_ms = a;
  if (reduce_ms != nullptr) *reduce_ms = b;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_scans_match(ndt2d_scans * s, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                      const double * beams_xy, const size_t * beam_offsets, size_t n_scans, const double * dth,
                      size_t n_th, const double * dlin, size_t n_lin, double * records_out, double * all_scores)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  if (jobs_xyt == nullptr || records_out == nullptr || beams_xy == nullptr || beam_offsets == nullptr || dth == nullptr ||
      dlin == nullptr)
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: null argument");
  }
  // what ndt2d_set_search refuses
  if (n_th == 0 || n_lin == 0 || n_th > (1u << 24) || n_lin > 46340)
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: bad argument (lattice)");
  }
  if (n_jobs >= (1u << 24) || n_scans >= (1u << 24)) return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: bad argument (n_jobs, n_scans)");
  if (job_scan == nullptr && n_scans != n_jobs)
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: bad argument (no job_scan: job k uses scan k, n_scans must equal n_jobs)");
  }
  // every scan and every job is checked before anything is launched
  for (size_t sc = 0; sc < n_scans; ++sc)
  {
    if (beam_offsets[sc + 1] < beam_offsets[sc])
    {
      return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: scan " + std::to_string(sc) + ": beam_offsets decrease");
    }
    const size_t count = beam_offsets[sc + 1] - beam_offsets[sc];
    // (what ndt2d_set_beams refuses)
    if (count == 0 || count > kMaxScanBeams)
    {
      return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: scan " + std::to_string(sc) + ": " + std::to_string(count) +
                                             " beams (1 .. 2^20)");
    }
  }
  for (size_t k = 0; k < n_jobs; ++k)
  {
    if (!std::isfinite(jobs_xyt[3 * k]) || !std::isfinite(jobs_xyt[3 * k + 1]) || !std::isfinite(jobs_xyt[3 * k + 2]))
    {
      return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: job " + std::to_string(k) + ": the pose is not finite");
    }
    if (job_scan != nullptr && job_scan[k] >= n_scans)
    {
      return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: job " + std::to_string(k) + ": scan " +
                                             std::to_string(job_scan[k]) + " of " + std::to_string(n_scans));
    }
  }
  // the grid installed NOW; a list install's deferred map bytes are not read here and stay deferred
  ndt2d_grid_view v;
  const int vrc = ndt2d_grid_view_get(s->h, &v);
  if (vrc != NDT2D_OK) return sfail(s, vrc, vrc == NDT2D_ERR_NO_GRID ? "ndt2d_scans_match: no grid" : "ndt2d_scans_match: no grid view");
  GridDesc grid{};
  grid.cells_global = v.cells_global;
  grid.occ_bits = v.occ_bits;
  grid.size_x = v.size_x;
  grid.size_y = v.size_y;
  grid.ncell = v.ncell;
  grid.pow2 = v.pow2;
  grid.cell_size = v.cell_size;
  grid.inv_cell_size = v.inv_cell_size;
  grid.origin_x = v.origin_x;
  grid.origin_y = v.origin_y;
  if (grid.cells_global == nullptr || grid.occ_bits == nullptr)
  {
    return sfail(s, NDT2D_ERR_STATE, "ndt2d_scans_match: the installed grid has no records");
  }
  NDT2D_SCANS_HIP(s, hipSetDevice(s->device));
  const ScansCall t{jobs_xyt, job_scan, beams_xy, beam_offsets, n_scans, dth, n_th, dlin, n_lin};
  // more jobs than slots: in chunks
  size_t per_launch = s->max_jobs;
  if (all_scores != nullptr)
  {
    const size_t n_lattice = n_th * n_lin * n_lin;
    per_launch = std::min(per_launch, std::max<size_t>(1, kScoreDoublesPerLaunch / n_lattice));
  }
  for (size_t k0 = 0; k0 < n_jobs; k0 += per_launch)
  {
    const size_t k1 = std::min(n_jobs, k0 + per_launch);
    const int rc = match_chunk(s, grid, k0, k1, t, records_out, all_scores);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
