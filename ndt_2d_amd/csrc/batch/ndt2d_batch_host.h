// The host side of the batched searches (closure/, starts/, scans/) on top of the state every
// batched object holds (BatchHost with its helpers: batch/ndt2d_batch_state.h, which defines no
// kernel and is all that refine/, verify/ and posegraph/ take): the stage and records of a search
// chunk, the reduction launch with its read-back, and the engine of the searches on the installed
// grid (JobsEngine, match_jobs: defined in scans/ndt2d_scans.hip, used by starts/ too).
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
#include "ndt2d_batch_state.h"
#include "ndt2d_hip.h"
#include "ndt2d_job_groups.h"
#include "ndt2d_refine_jobs.h"

namespace ndt2d
{

constexpr size_t kRec = NDT2D_MATCH_RECORD_DOUBLES;
// all_scores wanted: slots of one chunk, so that the scores on their way back stay within this
constexpr size_t kScoreDoublesPerLaunch = size_t(8) << 20;

// The stage, the block records and the out pair of a chunk of n_slots slots.
inline hipError_t batch_grow(BatchHost * s, size_t stage_doubles, size_t n_slots, size_t n_th, size_t out_doubles)
{
  hipError_t e = grow_pair(&s->h_stage, &s->d_stage, &s->stage_cap, stage_doubles);
  if (e == hipSuccess) e = grow_device(&s->d_partials, &s->partials_cap, n_slots * n_th * kRec * sizeof(double));
  if (e == hipSuccess) e = grow_pair(&s->h_out, &s->d_out, &s->out_cap, out_doubles);
  return e;
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

#endif  // NDT2D_BATCH_HOST_H_
