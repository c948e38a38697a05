// The dense covariance of the pose graph on the device (include/ndt2d_hip.h, "Dense covariance"):
// every node's 3 x 3 diagonal block and chosen (a, b) blocks of
// (H_FF + damping clamp(diag H_FF))^-1 by a dense Cholesky, at a cost that does not depend on the
// closures (gfx950 / MI355X).  The object stands beside an ndt2d_posegraph and reads its graph,
// weighting and loss; the kernels are covariance/ndt2d_covariance_kernel.h, the panels, the chunk
// size and the launch list covariance/ndt2d_covariance_plan.h, the launch path of the factor and the
// inverse covariance/ndt2d_covariance_launch.h.  What an object beside the graph is made of, the
// prelude of a call and a chunk's poses are posegraph/ndt2d_posegraph_state.h; what the call refuses
// about its arguments is posegraph/ndt2d_posegraph_args.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "covariance/ndt2d_covariance_kernel.h"
#include "covariance/ndt2d_covariance_launch.h"
#include "covariance/ndt2d_covariance_plan.h"
#include "posegraph/ndt2d_posegraph_args.h"
#include "posegraph/ndt2d_posegraph_state.h"

struct ndt2d_covariance : ndt2d::PgCompanion
{
  // on the device, from the first compute on: the chunk's poses where the caller gives them, the pairs
  ndt2d::PgPoses poses;
  void * d_pairs = nullptr;
  size_t pairs_cap = 0;
  std::vector<ndt2d::covariance::Launch> launches;
};

using ndt2d::batch_fail;

extern "C" {

int ndt2d_covariance_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_covariance ** out)
{
  NDT2D_C_TRY
  return ndt2d::pg_companion_create(posegraph, workspace_bytes, out);
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_covariance_destroy(ndt2d_covariance * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::pg_companion_release(s);
  for (void * p : {s->poses.d, s->d_pairs})
  {
    if (p != nullptr) (void)hipFree(p);
  }
  delete s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_covariance_last_error(ndt2d_covariance * s)
{
  return s != nullptr ? s->err.c_str() : "null covariance";
}

int ndt2d_covariance_set_timing(ndt2d_covariance * s, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(s, enabled);
  NDT2D_C_CATCH(s)
}

int ndt2d_covariance_last_ms(ndt2d_covariance * s, float * kernel_ms, float * fetch_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(s, "covariance", kernel_ms, fetch_ms);
  NDT2D_C_CATCH(s)
}

int ndt2d_covariance_compute(ndt2d_covariance * s, const uint8_t * enabled, size_t n_jobs, const double * poses, double damping,
                             const uint32_t * pairs, size_t n_pairs, double * diagonal_out, double * pairs_out, double * records_out)
{
  NDT2D_C_TRY
  namespace cov = ndt2d::covariance;
  namespace args = ndt2d::pg_args;
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  const char * const entry = "ndt2d_covariance_compute";
  const std::string who = std::string(entry) + ": ";
  if (diagonal_out == nullptr || records_out == nullptr || (n_pairs != 0 && (pairs == nullptr || pairs_out == nullptr)))
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + "null argument");
  }
  int rc = ndt2d::batch_refuse(s, args::damping_refusal(entry, damping));
  if (rc != NDT2D_OK) return rc;
  ndt2d_posegraph * g = s->graph;
  const size_t P = n_pairs;
  size_t job_bytes = 0, chunk = 0;
  ndt2d::PgCall call;
  rc = ndt2d::pg_begin_call(s, g, entry, &call, [&] {
    if (P > 0x7FFFFFFFu - g->n) return who + "more than 2^31 - 1 blocks a job";
    std::string refusal = args::nodes_refusal(entry, "pair", pairs, P, 2, g->n);
    if (refusal.empty()) refusal = args::poses_refusal(entry, poses, n_jobs, g->n);
    if (!refusal.empty()) return refusal;
    job_bytes = cov::job_doubles(g->n) * sizeof(double);
    chunk = cov::chunk_jobs(g->max_jobs, s->workspace_bytes, job_bytes);
    return args::dense_refusal(entry, g->n, cov::kMaxDim, chunk, job_bytes, s->workspace_bytes);
  });
  if (rc != NDT2D_OK) return rc;
  const hipStream_t stream = call.stream;
  const ndt2d::PgGraph & G = call.G;
  const size_t n = g->n;
  // the workspace: what the call's largest chunk needs, never more than the budget
  rc = ndt2d::pg_companion_workspace(s, std::min(chunk, n_jobs) * job_bytes);
  if (rc != NDT2D_OK) return rc;
  if (P != 0)
  {
    NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_pairs, &s->pairs_cap, 2 * P * sizeof(uint32_t)));
    NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_pairs, pairs, 2 * P * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  }
  ndt2d::cov_launch_list(3 * n, true, &s->launches);
  ndt2d::CovFactorLaunch a{};
  a.damping = damping;
  a.workspace = static_cast<double *>(s->d_workspace);
  for (size_t k0 = 0; k0 < n_jobs; k0 += chunk)
  {
    const size_t k1 = std::min(n_jobs, k0 + chunk), kc = k1 - k0;
    rc = ndt2d::pg_relay(s, g, ndt2d::pg_send_masks(g, stream, enabled, k0, k1, &a.d_en));
    if (rc != NDT2D_OK) return rc;
    rc = ndt2d::pg_chunk_poses(s, stream, &s->poses, poses, k0, kc, n, G, &a.poses, &a.pose_stride);
    if (rc != NDT2D_OK) return rc;
    // what comes back: [diagonal kc n 9 | pairs kc P 9 | records kc 3]
    const size_t at_pairs = kc * n * 9, at_rec = at_pairs + kc * P * 9, total = at_rec + kc * ndt2d::kCovRec;
    NDT2D_BATCH_HIP(s, ndt2d::grow_pair(&s->h_out, &s->d_out, &s->out_cap, total));
    a.jobs = static_cast<uint32_t>(kc);
    a.records = s->d_out + at_rec;
    // a chunk in stream order: the factor and the inverse, then the blocks
    rc = ndt2d::batch_round_trip(s, stream, total, [&] {
      ndt2d::cov_enqueue_factor<ndt2d::CovJob, true>(g, stream, G, a, s->launches);
      hipLaunchKernelGGL(ndt2d::covariance_blocks_kernel, dim3(static_cast<uint32_t>(n + P), 1, a.jobs), dim3(ndt2d::kWave), 0, stream,
                         static_cast<uint32_t>(n), static_cast<const uint32_t *>(s->d_pairs), a.workspace, a.records, s->d_out,
                         s->d_out + at_pairs);
      return NDT2D_OK;
    });
    if (rc != NDT2D_OK) return rc;
    std::memcpy(diagonal_out + k0 * n * 9, s->h_out, kc * n * 9 * sizeof(double));
    if (P != 0) std::memcpy(pairs_out + k0 * P * 9, s->h_out + at_pairs, kc * P * 9 * sizeof(double));
    std::memcpy(records_out + k0 * ndt2d::kCovRec, s->h_out + at_rec, kc * ndt2d::kCovRec * sizeof(double));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
