// The host side the batched searches share (closure/, starts/, scans/): the state every such
// object holds beside the context -- the pinned / device stage of a chunk's one upload, the block
// records, the pinned / device pair of what comes back, three timing events, the last error --
// with its growth, release, failure and timing helpers, and the engine of the searches on the
// installed grid (JobsEngine, match_jobs: defined in scans/ndt2d_scans.hip, used by starts/ too).
// Included by the .hip translation units only.
#ifndef NDT2D_BATCH_HOST_H_
#define NDT2D_BATCH_HOST_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "ndt2d_batch_search.h"
#include "ndt2d_hip.h"
#include "ndt2d_job_groups.h"
#include "ndt2d_refine_jobs.h"

namespace ndt2d
{

constexpr size_t kRec = NDT2D_MATCH_RECORD_DOUBLES;
// all_scores wanted: slots of one chunk, so that the scores on their way back stay within this
constexpr size_t kScoreDoublesPerLaunch = size_t(8) << 20;

struct BatchHost
{
  ndt2d_handle h = nullptr;
  int device = 0;
  std::string err;
  // one upload per chunk (doubles), pinned and on the device
  double * h_stage = nullptr, * d_stage = nullptr;
  size_t stage_cap = 0;
  void * d_partials = nullptr;   // [slot][n_th][12] block records
  size_t partials_cap = 0;       // bytes
  // what comes back: [slot][12] records | [slot][lattice] scores (doubles), on the device and pinned
  double * d_out = nullptr, * h_out = nullptr;
  size_t out_cap = 0;
  bool timing = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // around the chunk's two timed phases
  bool timed = false;
};

inline void guard_note(BatchHost * s, const char * what) noexcept
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
inline void guard_note(std::nullptr_t, const char *) noexcept {}

inline int batch_fail(BatchHost * s, int code, const std::string & msg)
{
  if (s != nullptr) s->err = msg;
  return code;
}

// The end of a setter: what it refuses (a text of batch/ndt2d_refine_jobs.h's kind), or nothing.
inline int batch_refuse(BatchHost * s, const std::string & refusal)
{
  return refusal.empty() ? NDT2D_OK : batch_fail(s, NDT2D_ERR_INVALID, refusal);
}

inline int batch_fail_hip(BatchHost * s, hipError_t e, const char * what)
{
  (void)hipGetLastError();  // clear sticky state
  return batch_fail(s, NDT2D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define NDT2D_BATCH_HIP(s, call)                                         \
  do                                                                     \
  {                                                                      \
    hipError_t e__ = (call);                                             \
    if (e__ != hipSuccess) return ndt2d::batch_fail_hip(s, e__, #call);  \
  } while (0)

// Device memory of at least `bytes` at *p (contents are not kept).
inline hipError_t grow_device(void ** p, size_t * cap, size_t bytes)
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

// A pinned / device pair of at least `doubles` (contents are not kept).
inline hipError_t grow_pair(double ** host, double ** dev, size_t * cap, size_t doubles)
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

// The stage, the block records and the out pair of a chunk of n_slots slots.
inline hipError_t batch_grow(BatchHost * s, size_t stage_doubles, size_t n_slots, size_t n_th, size_t out_doubles)
{
  hipError_t e = grow_pair(&s->h_stage, &s->d_stage, &s->stage_cap, stage_doubles);
  if (e == hipSuccess) e = grow_device(&s->d_partials, &s->partials_cap, n_slots * n_th * kRec * sizeof(double));
  if (e == hipSuccess) e = grow_pair(&s->h_out, &s->d_out, &s->out_cap, out_doubles);
  return e;
}

// Everything BatchHost owns on the device and in pinned memory (the object itself is the caller's).
inline void batch_release(BatchHost * s)
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
}

// The body of ndt2d_<noun>_destroy: the stream is waited out first.
inline void batch_drain(BatchHost * s)
{
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(s->h)));
}

// The bodies of ndt2d_<noun>_set_timing / ndt2d_<noun>_last_ms: (ev[0] -> ev[1], ev[1] -> ev[2]) of
// the last timed chunk.
inline int batch_set_timing(BatchHost * s, int enabled)
{
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (enabled != 0 && s->ev[0] == nullptr)
  {
    NDT2D_BATCH_HIP(s, hipSetDevice(s->device));
    for (hipEvent_t & ev : s->ev) NDT2D_BATCH_HIP(s, hipEventCreate(&ev));
  }
  s->timing = enabled != 0;
  s->timed = false;
  return NDT2D_OK;
}

inline int batch_last_ms(BatchHost * s, const char * noun, float * first_ms, float * second_ms)
{
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (!s->timed)
  {
    return batch_fail(s, NDT2D_ERR_STATE, std::string("ndt2d_") + noun + "_last_ms: no timed match (ndt2d_" + noun + "_set_timing)");
  }
  float a = 0.0f, b = 0.0f;
  NDT2D_BATCH_HIP(s, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  NDT2D_BATCH_HIP(s, hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
  if (first_ms != nullptr) *first_ms = a;
  if (second_ms != nullptr) *second_ms = b;
  return NDT2D_OK;
}

// The reduction launch and the one read-back of a chunk: records (and scores) of slots [k0, k0 +
// n_slots) into the call's arrays.  ev_behind: the event recorded behind the reduction, or -1.
// (static: the kernel is the including unit's own)
static inline int batch_reduce_and_fetch(BatchHost * s, hipStream_t stream, size_t k0, size_t n_slots, uint32_t n_th,
                                         size_t n_lattice, int ev_behind, double * records_out, double * all_scores)
{
  const size_t n_out = n_slots * (kRec + (all_scores != nullptr ? n_lattice : 0));
  hipLaunchKernelGGL(batch_reduce_kernel, dim3(static_cast<uint32_t>(n_slots)), dim3(kReduceThreads), 0, stream,
                     static_cast<const double *>(s->d_partials), n_th, s->d_out);
  NDT2D_BATCH_HIP(s, hipGetLastError());
  if (s->timing && ev_behind >= 0) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[ev_behind], stream));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, n_out * sizeof(double), hipMemcpyDeviceToHost, stream));
  NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
  s->timed = s->timing;
  std::memcpy(records_out + k0 * kRec, s->h_out, n_slots * kRec * sizeof(double));
  if (all_scores != nullptr)
  {
    std::memcpy(all_scores + k0 * n_lattice, s->h_out + n_slots * kRec, n_slots * n_lattice * sizeof(double));
  }
  return NDT2D_OK;
}

// Slots of one chunk: the object's limit, fewer where all_scores are wanted.
inline size_t slots_per_launch(size_t max_slots, bool want_scores, size_t n_lattice)
{
  if (!want_scores) return max_slots;
  return std::min(max_slots, std::max<size_t>(1, kScoreDoublesPerLaunch / n_lattice));
}

// cos / sin of (heading + dth[i]) from the host libm (src/scan_matcher_ndt.cpp:106-107), a row
// [cos x n_th | sin x n_th] per distinct heading (by its bits) of poses [k0, k1): the rows into
// `trig`, each pose's row into row_out[k - k0].
inline void heading_rows(const double * poses_xyt, size_t k0, size_t k1, const double * dth, size_t n_th,
                         std::unordered_map<uint64_t, uint32_t> & row_of, std::vector<double> & trig,
                         std::vector<uint32_t> & row_out)
{
  row_of.clear();
  trig.clear();
  row_out.resize(k1 - k0);
  for (size_t k = k0; k < k1; ++k)
  {
    const double theta = poses_xyt[3 * k + 2];
    uint64_t bits;
    std::memcpy(&bits, &theta, sizeof(bits));
    auto it = row_of.find(bits);
    if (it == row_of.end())
    {
      const uint32_t row = static_cast<uint32_t>(trig.size() / (2 * n_th));
      it = row_of.emplace(bits, row).first;
      trig.resize(trig.size() + 2 * n_th);
      double * c = trig.data() + static_cast<size_t>(row) * 2 * n_th;
      for (size_t i = 0; i < n_th; ++i) ndt2d_cos_sin(theta + dth[i], c + i, c + n_th + i);
    }
    row_out[k - k0] = it->second;
  }
}

// The grid installed in the context NOW, as the kernels take it; a list install's deferred map
// bytes are not read here and stay deferred.  *rc: NDT2D_OK, what ndt2d_grid_view_get says, or
// NDT2D_ERR_STATE for a grid without records.
inline GridDesc installed_grid(ndt2d_handle h, int * rc)
{
  GridDesc grid{};
  ndt2d_grid_view v;
  *rc = ndt2d_grid_view_get(h, &v);
  if (*rc != NDT2D_OK) return grid;
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
  if (grid.cells_global == nullptr || grid.occ_bits == nullptr) *rc = NDT2D_ERR_STATE;
  return grid;
}

// ---- the searches on the installed grid: K jobs, each a (scan, pose) pair ----

struct JobsEngine : BatchHost
{
  size_t max_jobs = 0;                             // slots of a chunk
  std::vector<double> trig;                        // the chunk's cos / sin rows
  std::unordered_map<uint64_t, uint32_t> row_of;   // heading (bits) -> row
  std::vector<uint32_t> rows;                      // job of the chunk -> row
  std::vector<uint64_t> scan_first;                // scan -> its first beam within the chunk's beams (or: not sent)
  std::vector<uint32_t> sent, job_beams;           // the chunk's scans in upload order; beams per job
  JobGroups groups;
};

// A call's arguments, checked by the entry point: finite poses, job_scan[k] < n_scans, every
// scan 1 .. 2^20 beams, a lattice ndt2d_set_search takes.
struct JobsCall : refine_jobs::JobList
{
  bool one_scan;   // start poses: every job uses scan 0 (n_scans = 1, no job_scan), the blocks take StartSlots
  const double * dth;
  size_t n_th;
  const double * dlin;
  size_t n_lin;
  size_t scan_of(size_t k) const { return one_scan ? 0 : JobList::scan_of(k); }
  size_t beams_of(size_t k) const { return beam_offsets[scan_of(k) + 1] - beam_offsets[scan_of(k)]; }
};

// The checked call against the grid installed now, in chunks of e->max_jobs; `who` names the
// entry point in the error texts.  Not part of the C-ABI.
__attribute__((visibility("hidden"))) int match_jobs(JobsEngine * e, const char * who, const JobsCall & t,
                                                     double * records_out, double * all_scores);

}  // namespace ndt2d

using ndt2d::guard_note;   // (NDT2D_C_CATCH of the entry points, which live outside the namespace)

#endif  // NDT2D_BATCH_HOST_H_
