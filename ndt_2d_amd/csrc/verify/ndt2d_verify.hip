// Match verification of K (scan, pose) jobs against the grid INSTALLED in the context: which
// beams of each scan the map explains at the job's pose -- a class per beam (off the grid, unseen,
// outlier, inlier), whether the ray from the robot to the beam's end passes through a cell's
// Gaussian on its way (pierced), and integer counts per job -- in one upload, ONE kernel launch
// and one read-back per chunk (gfx950 / MI355X).  The classes, the ray and the records are the
// contract of include/ndt2d_hip.h ("Match verification"); the line walk and the closest approach
// are verify/ndt2d_verify_ray.h.
//
// The kernel, its job record, its arguments, the settings and the layout of what comes back are
// verify/ndt2d_verify_kernel.h (the loop closure instantiates the same text on its candidate
// slots); here: the object, the chunk on the installed grid -- InstalledSource,
// batch/ndt2d_installed_map.h -- and the C entry points.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "batch/ndt2d_refine_jobs.h"
#include "batch/ndt2d_stage_layout.h"
#include "verify/ndt2d_verify_kernel.h"

struct ndt2d_verify : ndt2d::BatchHost
{
  size_t max_jobs = 0;                // slots of a chunk
  ndt2d::VerifySettings set;          // neighbourhood, gates, rays
  std::vector<uint64_t> scan_first;  // scan -> its first beam within the chunk's beams (or: not sent)
  std::vector<uint32_t> sent;         // the chunk's scans in upload order
  std::vector<size_t> job_first;      // job of the call -> its first beam within the caller's per-beam arrays
};

namespace ndt2d
{

namespace
{

using InstalledVerifyArgs = VerifyArgs<InstalledSource>;

// CELLS: the neighbourhood of a point, 1 or 9.
template <uint32_t CELLS>
void launch_verify(bool pow2, dim3 blocks, dim3 threads, hipStream_t stream, const InstalledVerifyArgs & a)
{
  if (pow2) hipLaunchKernelGGL((verify_kernel<true, CELLS, InstalledSource>), blocks, threads, 0, stream, a);
  else hipLaunchKernelGGL((verify_kernel<false, CELLS, InstalledSource>), blocks, threads, 0, stream, a);
}

// Jobs [k0, k1) of a call whose arguments have been checked; they hold n_out beams.
int verify_chunk(ndt2d_verify * s, const GridDesc & grid, size_t k0, size_t k1, size_t n_out, const VerifyCall & t)
{
  const size_t n_slots = k1 - k0;
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));

  // the scans this chunk's jobs name, each once, in the order the jobs first name them
  const size_t n_beams = refine_jobs::plan_sent_scans(
    n_slots, [&](size_t b) { return k0 + b; }, [&](size_t k) { return t.scan_of(k); }, t.beam_offsets, t.n_scans, s->scan_first,
    s->sent);

  // the one upload of the chunk: [beams | jobs | cos / sin pairs]
  const StageLayout at = stage_layout(0, 0, n_beams, n_slots, kVerifyJobDoubles, 0, 2 * n_slots);
  const VerifyOutLayout out = verify_out_layout(n_slots, n_out, t);
  NDT2D_BATCH_HIP(s, grow_pair(&s->h_stage, &s->d_stage, &s->stage_cap, at.total));
  NDT2D_BATCH_HIP(s, grow_pair(&s->h_out, &s->d_out, &s->out_cap, out.total));
  double * st = s->h_stage;
  refine_jobs::copy_sent_scans(s->sent, s->scan_first, t.beams_xy, t.beam_offsets, st + at.beams);
  const size_t out0 = s->job_first[k0];
  for (size_t k = k0; k < k1; ++k)
  {
    const double * p = t.jobs_xyt + 3 * k;
    reinterpret_cast<VerifyJob *>(st + at.jobs)[k - k0] =
      VerifyJob{p[0], p[1], static_cast<uint32_t>(t.beams_of(k)), 0u, s->scan_first[t.scan_of(k)], s->job_first[k] - out0};
    // cos / sin of the heading from the host libm, as everywhere in this library
    ndt2d_cos_sin(p[2], st + at.trig + 2 * (k - k0), st + at.trig + 2 * (k - k0) + 1);
  }
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_stage, st, at.total * sizeof(double), hipMemcpyHostToDevice, stream));

  InstalledVerifyArgs a{};
  a.source.g = grid;
  a.jobs = reinterpret_cast<const VerifyJob *>(s->d_stage + at.jobs);
  a.trig = s->d_stage + at.trig;
  a.beams_xy = s->d_stage + at.beams;
  a.rules = s->set.rules();
  a.records = reinterpret_cast<uint32_t *>(s->d_out);
  a.beam_m2 = t.beam_m2_out != nullptr ? s->d_out + out.m2 : nullptr;
  a.beam_cells = t.beam_cells_out != nullptr ? reinterpret_cast<uint32_t *>(s->d_out + out.cells) : nullptr;
  a.beam_class = t.beam_class_out != nullptr ? reinterpret_cast<uint8_t *>(s->d_out + out.classes) : nullptr;
  const int rc = batch_round_trip(s, stream, out.total, [&] {
    const dim3 blocks(static_cast<uint32_t>(n_slots)), threads(kVerifyThreads);
    if (s->set.cells == 9) launch_verify<9>(grid.pow2 != 0, blocks, threads, stream, a);
    else launch_verify<1>(grid.pow2 != 0, blocks, threads, stream, a);
    return NDT2D_OK;
  });
  if (rc != NDT2D_OK) return rc;
  std::memcpy(t.records_out + k0 * kVerifyRec, s->h_out, n_slots * kVerifyRec * sizeof(uint32_t));
  if (t.beam_m2_out != nullptr) std::memcpy(t.beam_m2_out + out0, s->h_out + out.m2, n_out * sizeof(double));
  if (t.beam_cells_out != nullptr) std::memcpy(t.beam_cells_out + 2 * out0, s->h_out + out.cells, n_out * 2 * sizeof(uint32_t));
  if (t.beam_class_out != nullptr) std::memcpy(t.beam_class_out + out0, s->h_out + out.classes, n_out);
  return NDT2D_OK;
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_verify_create(ndt2d_handle h, size_t max_jobs, ndt2d_verify ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || max_jobs == 0 || max_jobs > ndt2d::kVerifyMaxJobs) return NDT2D_ERR_INVALID;
  ndt2d_verify * v = new ndt2d_verify();
  v->h = h;
  v->device = ndt2d_device_id(h);
  v->max_jobs = max_jobs;
  *out = v;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_verify_destroy(ndt2d_verify * v)
{
  NDT2D_C_TRY
  if (v == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::batch_drain(v);
  ndt2d::batch_release(v);
  delete v;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_verify_last_error(ndt2d_verify * v)
{
  return v != nullptr ? v->err.c_str() : "null verify";
}

int ndt2d_verify_set_timing(ndt2d_verify * v, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(v, enabled);
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_last_ms(ndt2d_verify * v, float * kernel_ms, float * fetch_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(v, "verify", kernel_ms, fetch_ms);
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_set_neighbourhood(ndt2d_verify * v, uint32_t cells)
{
  NDT2D_C_TRY
  if (v == nullptr) return NDT2D_ERR_INVALID;
  return ndt2d::batch_refuse(v, v->set.set_cells("ndt2d_verify_set_neighbourhood", cells));
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_neighbourhood(ndt2d_verify * v, uint32_t * out)
{
  NDT2D_C_TRY
  if (v == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = v->set.cells;
  return NDT2D_OK;
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_set_gates(ndt2d_verify * v, double gate_inlier, double gate_pierce)
{
  NDT2D_C_TRY
  if (v == nullptr) return NDT2D_ERR_INVALID;
  return ndt2d::batch_refuse(v, v->set.set_gates("ndt2d_verify_set_gates", gate_inlier, gate_pierce));
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_gates(ndt2d_verify * v, double * gate_inlier_out, double * gate_pierce_out)
{
  NDT2D_C_TRY
  if (v == nullptr || gate_inlier_out == nullptr || gate_pierce_out == nullptr) return NDT2D_ERR_INVALID;
  *gate_inlier_out = v->set.gate_inlier;
  *gate_pierce_out = v->set.gate_pierce;
  return NDT2D_OK;
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_set_rays(ndt2d_verify * v, int enabled)
{
  NDT2D_C_TRY
  if (v == nullptr) return NDT2D_ERR_INVALID;
  return ndt2d::batch_refuse(v, v->set.set_rays("ndt2d_verify_set_rays", enabled));
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_rays(ndt2d_verify * v, int * out)
{
  NDT2D_C_TRY
  if (v == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = v->set.rays ? 1 : 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(v)
}

int ndt2d_verify_run(ndt2d_verify * v, const double * jobs_xyt, const uint32_t * job_scan, size_t n_jobs,
                     const double * beams_xy, const size_t * beam_offsets, size_t n_scans, uint32_t * records_out,
                     uint8_t * beam_class_out, double * beam_m2_out, uint32_t * beam_cells_out)
{
  NDT2D_C_TRY
  if (v == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  if (jobs_xyt == nullptr || records_out == nullptr || beams_xy == nullptr || beam_offsets == nullptr)
  {
    return batch_fail(v, NDT2D_ERR_INVALID, "ndt2d_verify_run: null argument");
  }
  // every scan and every job are checked before anything is launched: what the registration
  // refuses about them
  const std::string refusal = ndt2d::refine_jobs::refusal("ndt2d_verify_run", jobs_xyt, job_scan, n_jobs, beam_offsets, n_scans);
  if (!refusal.empty()) return batch_fail(v, NDT2D_ERR_INVALID, refusal);
  int rc = NDT2D_OK;
  const ndt2d::GridDesc grid = ndt2d::installed_grid(v->h, &rc);
  if (rc != NDT2D_OK)
  {
    return batch_fail(v, rc, std::string("ndt2d_verify_run") + (rc == NDT2D_ERR_NO_GRID ? ": no grid"
                                                                : rc == NDT2D_ERR_STATE ? ": the installed grid has no records"
                                                                                        : ": no grid view"));
  }
  if (v->set.rays && (grid.size_x > ndt2d::verify::kMaxGridSide || grid.size_y > ndt2d::verify::kMaxGridSide))
  {
    return batch_fail(v, NDT2D_ERR_INVALID, "ndt2d_verify_run: a grid side above 2^24 cells (rays enabled)");
  }
  NDT2D_BATCH_HIP(v, hipSetDevice(v->device));
  const ndt2d::VerifyCall t{{jobs_xyt, job_scan, n_jobs, beams_xy, beam_offsets, n_scans},
                            records_out, beam_class_out, beam_m2_out, beam_cells_out};
  // job k's beams start at the sum of the earlier jobs' scan lengths
  v->job_first.resize(n_jobs + 1);
  v->job_first[0] = 0;
  for (size_t k = 0; k < n_jobs; ++k) v->job_first[k + 1] = v->job_first[k] + t.beams_of(k);
  // more jobs than slots, or more beams than a chunk's results take: in chunks
  for (size_t k0 = 0; k0 < n_jobs;)
  {
    size_t k1 = k0 + 1;
    while (k1 < n_jobs && k1 - k0 < v->max_jobs && v->job_first[k1 + 1] - v->job_first[k0] <= ndt2d::kVerifyChunkBeams) ++k1;
    rc = ndt2d::verify_chunk(v, grid, k0, k1, v->job_first[k1] - v->job_first[k0], t);
    if (rc != NDT2D_OK) return rc;
    k0 = k1;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(v)
}

}  // extern "C"
