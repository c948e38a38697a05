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
// The kernel, its job record and its arguments are refine/ndt2d_refine_kernel.h (the loop closure
// instantiates the same text on its candidate slots); here: the object, the chunk on the installed
// grid -- InstalledSource, batch/ndt2d_installed_map.h -- and the C entry points.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "batch/ndt2d_refine_jobs.h"
#include "batch/ndt2d_stage_layout.h"
#include "refine/ndt2d_refine_kernel.h"

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

// CELLS: the neighbourhood of a point, 1 or 9.
template <uint32_t CELLS>
void launch_refine(bool pow2, dim3 blocks, dim3 threads, hipStream_t stream, const InstalledArgs & a)
{
  if (pow2) hipLaunchKernelGGL((refine_kernel<true, CELLS, InstalledSource>), blocks, threads, 0, stream, a);
  else hipLaunchKernelGGL((refine_kernel<false, CELLS, InstalledSource>), blocks, threads, 0, stream, a);
}

struct RefineCall : refine_jobs::JobList
{
  refine::Rules rules;
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
  refine_jobs::copy_sent_scans(s->sent, s->scan_first, t.beams_xy, t.beam_offsets, st + at.beams);
  for (size_t k = k0; k < k1; ++k)
  {
    const double * p = t.jobs_xyt + 3 * k;
    reinterpret_cast<RefineJob *>(st + at.jobs)[k - k0] =
      RefineJob{p[0], p[1], p[2], static_cast<uint32_t>(t.beams_of(k)), 0u, s->scan_first[t.scan_of(k)]};
    // cos / sin of the start heading from the host libm, as everywhere in this library
    ndt2d_cos_sin(p[2], st + at.trig + 2 * (k - k0), st + at.trig + 2 * (k - k0) + 1);
  }
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_stage, st, at.total * sizeof(double), hipMemcpyHostToDevice, stream));

  InstalledArgs a{};
  a.source.g = grid;
  a.jobs = reinterpret_cast<const RefineJob *>(s->d_stage + at.jobs);
  a.trig = s->d_stage + at.trig;
  a.beams_xy = s->d_stage + at.beams;
  a.rules = t.rules;
  a.records = s->d_out;
  const int rc = batch_round_trip(s, stream, n_slots * kRefineRec, [&] {
    const dim3 blocks(static_cast<uint32_t>(n_slots)), threads(kRefineThreads);
    if (s->cells == 9) launch_refine<9>(grid.pow2 != 0, blocks, threads, stream, a);
    else launch_refine<1>(grid.pow2 != 0, blocks, threads, stream, a);
    return NDT2D_OK;
  });
  if (rc != NDT2D_OK) return rc;
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
  const ndt2d::RefineCall t{{jobs_xyt, job_scan, n_jobs, beams_xy, beam_offsets, n_scans}, {max_evals, tol_lin, tol_ang}};
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
