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
//   batch_search_kernel<C, POW2, JobSlots> (../batch/ndt2d_batch_search.h)   grid (theta step,
//       job of the launch's group), a lane per (dx, dy), as wide as the translation lattice (wider
//       lattices loop).  The block looks its job up in the group's index table, takes the job's
//       beam pointer and count, its (x, y) and its heading's cos / sin row (host libm), and walks
//       lane_walk<C, POW2> (../batch/ndt2d_walk_fn.h) on the installed grid.  C, the number of
//       partial sums, follows from the beam count of the job's scan (../batch/ndt2d_sum_chunks.h)
//       and is a template parameter of the walk, so the jobs of a chunk are grouped by C
//       (../batch/ndt2d_job_groups.h) and a chunk is one launch per C present: one when the scans
//       are subsampled to one count, eight at most.  Records and scores are written by job, in
//       the caller's order, whatever the grouping.
//   batch_reduce_kernel   one block per job: the n_theta records of its blocks ->
//       {best_score, best_index (+0.5: near tie), acc[10]} with merge_best, fixed order.
//
// The host engine here (match_jobs, match_chunk) serves starts/ too: one scan that every job names.
//
// Several jobs may name one scan (a heading fan per robot): its beams travel once.  A scan no job
// of the chunk names is not uploaded.
//
// Off the grid.  cell_index gives ncell for every point outside the grid, bit ncell
// of the bitmap is 0 and record ncell exists, so no lane indexes beyond either.  A job's beams
// are read at [beam_first, beam_first + n_beams) of the chunk's upload only; both come from the
// host's table, checked against the offsets before anything is launched.
//
// The bits of a raw score are those of closure/: the same walk, the same C for the
// same beam count -- the sequential search's bits wherever it runs the small-lattice search with
// its default plan.
//
// Determinism.  A lane's sums are its own, blocks reduce lanes over the DPP network
// and waves in wave order, the reducing block takes records r, r + 256, ... per thread.  Stream
// order is the only ordering between the launches and __syncthreads the only barrier inside
// them; no polls, no atomics.  A job's bits depend on its scan, its pose and the grid alone: not
// on the other jobs, the grouping or the chunking.
//
// LDS of the search block: kStageBeams x {ox, oy} = 16 KB, reused for one record per wave.
#include <hip/hip_runtime.h>

#include <string>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_search.h"
#include "batch/ndt2d_batch_host.h"

struct ndt2d_scans : ndt2d::JobsEngine
{
};

namespace ndt2d
{

namespace
{

// Jobs [k0, k1) of a call whose arguments have been checked.  records_out / all_scores: the call's, whole.
// t.one_scan (start poses: every job names scan 0) takes the same steps and switches three things:
// the records are StartRec (24 bytes, no beam offset or count), there is no order table in the
// upload, and the search is one launch of StartSlots with the call's beam count.  The scan table,
// the beam counts per job and the grouping are still made -- one scan, one group, its C in
// groups.chunks[0] -- since the upload of the beams and the C of the launch come from them.
int match_chunk(JobsEngine * s, const GridDesc & grid, size_t k0, size_t k1, const JobsCall & t,
                double * records_out, double * all_scores)
{
  const size_t n_slots = k1 - k0;
  const size_t n_lattice = t.n_th * t.n_lin * t.n_lin;
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));

  // the scans this chunk's jobs name, each once, in the order the jobs first name them
  const size_t n_beams = refine_jobs::plan_sent_scans(
    n_slots, [&](size_t b) { return k0 + b; }, [&](size_t k) { return t.scan_of(k); }, t.beam_offsets, t.n_scans, s->scan_first,
    s->sent);
  s->job_beams.resize(n_slots);
  for (size_t k = k0; k < k1; ++k) s->job_beams[k - k0] = static_cast<uint32_t>(t.beams_of(k));
  group_jobs(s->job_beams.data(), n_slots, s->groups);
  heading_rows(t.jobs_xyt, k0, k1, t.dth, t.n_th, s->row_of, s->trig, s->rows);

  // the one upload of the chunk: [dth | dlin | beams | jobs | order | cos / sin rows]; start poses
  // travel as the shorter StartRec, in the caller's order (one scan: one C, no order table)
  const StageLayout at = stage_layout(t.n_th, t.n_lin, n_beams, n_slots, t.one_scan ? kStartDoubles : kJobDoubles,
                                      t.one_scan ? 0 : n_slots, s->trig.size());
  const size_t n_out = n_slots * (kRec + (all_scores != nullptr ? n_lattice : 0));
  NDT2D_BATCH_HIP(s, batch_grow(s, at.total, n_slots, t.n_th, n_out));
  double * st = s->h_stage;
  std::memcpy(st + at.dth, t.dth, t.n_th * sizeof(double));
  std::memcpy(st + at.dlin, t.dlin, t.n_lin * sizeof(double));
  refine_jobs::copy_sent_scans(s->sent, s->scan_first, t.beams_xy, t.beam_offsets, st + at.beams);
  for (size_t k = k0; k < k1; ++k)
  {
    const double x = t.jobs_xyt[3 * k], y = t.jobs_xyt[3 * k + 1];
    if (t.one_scan) reinterpret_cast<StartRec *>(st + at.jobs)[k - k0] = StartRec{x, y, s->rows[k - k0], 0u};
    else reinterpret_cast<JobRec *>(st + at.jobs)[k - k0] = JobRec{x, y, s->rows[k - k0], s->job_beams[k - k0], s->scan_first[t.scan_of(k)]};
  }
  if (!t.one_scan)
  {
    st[at.trig - 1] = 0.0;   // (the odd entry's other half)
    std::memcpy(st + at.order, s->groups.order.data(), n_slots * sizeof(uint32_t));
  }
  std::memcpy(st + at.trig, s->trig.data(), s->trig.size() * sizeof(double));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_stage, st, at.total * sizeof(double), hipMemcpyHostToDevice, stream));
  s->timed = false;
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[0], stream));

  const dim3 block(batch_search_threads(t.n_lin * t.n_lin));
  const auto common = [&](auto & a)   // what the two policies' arguments share
  {
    a.slots.grid = grid;
    a.slots.trig = s->d_stage + at.trig;
    a.slots.beams_xy = s->d_stage + at.beams;
    a.dth = s->d_stage + at.dth;
    a.dlin = s->d_stage + at.dlin;
    a.n_th = static_cast<uint32_t>(t.n_th);
    a.n_lin = static_cast<uint32_t>(t.n_lin);
    a.scores = all_scores != nullptr ? s->d_out + n_slots * kRec : nullptr;
    a.partials = static_cast<double *>(s->d_partials);
  };
  if (t.one_scan)
  {
    BatchSearchArgs<StartSlots> a{};
    common(a);
    a.slots.starts = reinterpret_cast<const StartRec *>(s->d_stage + at.jobs);
    a.slots.n_beams = s->job_beams[0];
    launch_batch_search(s->groups.chunks[0], grid.pow2 != 0, dim3(a.n_th, static_cast<uint32_t>(n_slots)), block, stream, a);
    NDT2D_BATCH_HIP(s, hipGetLastError());
  }
  else
  {
    BatchSearchArgs<JobSlots> a{};
    common(a);
    a.slots.jobs = reinterpret_cast<const JobRec *>(s->d_stage + at.jobs);
    a.slots.order = reinterpret_cast<const uint32_t *>(s->d_stage + at.order);
    // a launch per C present: its blocks find their jobs through order[first ..]
    for (uint32_t g = 0; g < s->groups.n_groups; ++g)
    {
      a.slots.first = s->groups.first[g];
      const dim3 grid_dim(a.n_th, s->groups.first[g + 1] - s->groups.first[g]);
      launch_batch_search(s->groups.chunks[g], grid.pow2 != 0, grid_dim, block, stream, a);
      NDT2D_BATCH_HIP(s, hipGetLastError());
    }
  }
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[1], stream));
  return batch_reduce_and_fetch(s, stream, k0, n_slots, static_cast<uint32_t>(t.n_th), n_lattice, 2, records_out, all_scores);
}

}  // namespace

int match_jobs(JobsEngine * e, const char * who, const JobsCall & t, double * records_out, double * all_scores)
{
  int rc = NDT2D_OK;
  const GridDesc grid = installed_grid(e->h, &rc);
  if (rc != NDT2D_OK)
  {
    return batch_fail(e, rc, std::string(who) + (rc == NDT2D_ERR_NO_GRID ? ": no grid"
                                                 : rc == NDT2D_ERR_STATE ? ": the installed grid has no records"
                                                                         : ": no grid view"));
  }
  NDT2D_BATCH_HIP(e, hipSetDevice(e->device));
  // more jobs than slots: in chunks
  const size_t per_launch = slots_per_launch(e->max_jobs, all_scores != nullptr, t.n_th * t.n_lin * t.n_lin);
  for (size_t k0 = 0; k0 < t.n_jobs; k0 += per_launch)
  {
    rc = match_chunk(e, grid, k0, std::min(t.n_jobs, k0 + per_launch), t, records_out, all_scores);
    if (rc != NDT2D_OK) return rc;
  }
  return NDT2D_OK;
}

}  // namespace ndt2d

using ndt2d::batch_fail;

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
  ndt2d::batch_drain(s);
  ndt2d::batch_release(s);
  delete s;
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
  return ndt2d::batch_set_timing(s, enabled);
  NDT2D_C_CATCH(s)
}

int ndt2d_scans_last_ms(ndt2d_scans * s, float * search_ms, float * reduce_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(s, "scans", search_ms, reduce_ms);
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
    return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: null argument");
  }
  // what ndt2d_set_search refuses
  if (n_th == 0 || n_lin == 0 || n_th > (1u << 24) || n_lin > 46340)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_scans_match: bad argument (lattice)");
  }
  // every scan and every job is checked before anything is launched: the shared text
  const std::string refusal = ndt2d::refine_jobs::refusal("ndt2d_scans_match", jobs_xyt, job_scan, n_jobs, beam_offsets, n_scans);
  if (!refusal.empty()) return batch_fail(s, NDT2D_ERR_INVALID, refusal);
  const ndt2d::JobsCall t{{jobs_xyt, job_scan, n_jobs, beams_xy, beam_offsets, n_scans}, false, dth, n_th, dlin, n_lin};
  return ndt2d::match_jobs(s, "ndt2d_scans_match", t, records_out, all_scores);
  NDT2D_C_CATCH(s)
}

}  // extern "C"
