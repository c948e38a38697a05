// The dense covariance of the pose graph on the device (include/ndt2d_hip.h, "Dense covariance"):
// every node's 3 x 3 diagonal block and chosen (a, b) blocks of
// (H_FF + damping clamp(diag H_FF))^-1 by a dense Cholesky, at a cost that does not depend on the
// closures (gfx950 / MI355X).  The object stands beside an ndt2d_posegraph and reads its graph,
// weighting and loss; the kernels are covariance/ndt2d_covariance_kernel.h, the panels, the chunk
// size and the launch list covariance/ndt2d_covariance_plan.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "covariance/ndt2d_covariance_kernel.h"
#include "covariance/ndt2d_covariance_plan.h"
#include "posegraph/ndt2d_posegraph_state.h"

struct ndt2d_covariance : ndt2d::BatchHost
{
  ndt2d_posegraph * graph = nullptr;   // (the caller keeps it alive)
  size_t workspace_bytes = 0;          // the budget
  // on the device, from the first compute on: the chunk's jobs, the chunk's poses where the caller
  // gives them, the pairs
  void * d_workspace = nullptr, * d_poses = nullptr, * d_pairs = nullptr;
  size_t workspace_cap = 0, poses_cap = 0, pairs_cap = 0;
  std::vector<ndt2d::covariance::Launch> launches;
};

namespace ndt2d
{

namespace
{

namespace cov = covariance;

// What the graph's own call left in its object, as this object's error.
int cov_from_graph(ndt2d_covariance * s, int rc)
{
  if (rc != NDT2D_OK) s->err = s->graph->err;
  return rc;
}

// What a chunk's launches take.
struct CovLaunch
{
  uint32_t jobs, n, n_pairs;
  const uint8_t * d_en;
  const double * poses;
  size_t pose_stride;      // 0: the graph's poses for every job
  double damping;
  double * workspace;
  const uint32_t * pairs;
  double * diagonal_out, * pairs_out, * records;
};

// A chunk in stream order: the nodes, the fill, the assembly, the plan's launches, the blocks.
void cov_launch(const ndt2d_covariance * s, hipStream_t stream, const PgGraph & G, const CovLaunch & a)
{
  const uint32_t ld = static_cast<uint32_t>(cov::padded(3 * static_cast<size_t>(a.n)));
  const dim3 per_node((a.n + kCovNodeThreads - 1) / kCovNodeThreads, 1, a.jobs);
  hipLaunchKernelGGL(covariance_nodes_kernel<>, per_node, dim3(kCovNodeThreads), 0, stream, G, a.d_en, a.poses, a.pose_stride, a.workspace);
  hipLaunchKernelGGL(covariance_fill_kernel<>, dim3((ld + kCovFillThreads - 1) / kCovFillThreads, ld, a.jobs), dim3(kCovFillThreads), 0, stream, a.n,
                     a.workspace);
  pg_dispatch(s->graph, [&](auto, auto loss) {
    hipLaunchKernelGGL(covariance_assemble_kernel<decltype(loss)::value>, per_node, dim3(kCovNodeThreads), 0, stream, G, a.d_en, a.poses,
                       a.pose_stride, a.damping, nullptr, size_t(0), a.workspace);
  });
  for (const cov::Launch & l : s->launches)
  {
    const dim3 grid(l.groups, 1, a.jobs);
    switch (l.kind)
    {
      case cov::kFactor:
        hipLaunchKernelGGL(covariance_factor_kernel<>, grid, dim3(kCovFactorThreads), 0, stream, a.n, l.panel, a.workspace, a.records);
        break;
      case cov::kSolveBelow:
        hipLaunchKernelGGL(covariance_solve_kernel<false>, grid, dim3(kWave), 0, stream, a.n, l.panel, a.workspace);
        break;
      case cov::kUpdate:
        hipLaunchKernelGGL(covariance_update_kernel<false>, grid, dim3(kCovUpdateThreads), 0, stream, a.n, l.panel, a.workspace);
        break;
      case cov::kSolveRow:
        hipLaunchKernelGGL(covariance_solve_kernel<true>, grid, dim3(kWave), 0, stream, a.n, l.panel, a.workspace);
        break;
      default:
        hipLaunchKernelGGL(covariance_update_kernel<true>, grid, dim3(kCovUpdateThreads), 0, stream, a.n, l.panel, a.workspace);
        break;
    }
  }
  hipLaunchKernelGGL(covariance_blocks_kernel, dim3(a.n + a.n_pairs, 1, a.jobs), dim3(kWave), 0, stream, a.n, a.pairs, a.workspace, a.records,
                     a.diagonal_out, a.pairs_out);
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_covariance_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_covariance ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (posegraph == nullptr || workspace_bytes == 0) return NDT2D_ERR_INVALID;
  ndt2d_covariance * s = new ndt2d_covariance();
  s->graph = posegraph;
  s->h = posegraph->h;
  s->device = posegraph->device;
  s->workspace_bytes = workspace_bytes;
  *out = s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_covariance_destroy(ndt2d_covariance * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::batch_drain(s);
  ndt2d::batch_release(s);
  for (void * p : {s->d_workspace, s->d_poses, s->d_pairs})
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
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  const std::string who = "ndt2d_covariance_compute: ";
  if (diagonal_out == nullptr || records_out == nullptr || (n_pairs != 0 && (pairs == nullptr || pairs_out == nullptr)))
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + "null argument");
  }
  if (!(damping >= 0.0) || !std::isfinite(damping)) return batch_fail(s, NDT2D_ERR_INVALID, who + "the damping is negative or not finite");
  ndt2d_posegraph * g = s->graph;
  int rc = ndt2d::cov_from_graph(s, ndt2d::pg_ready(g, "ndt2d_covariance_compute"));
  if (rc != NDT2D_OK) return rc;
  const size_t n = g->n, P = n_pairs;
  if (P > 0x7FFFFFFFu - n) return batch_fail(s, NDT2D_ERR_INVALID, who + "more than 2^31 - 1 blocks a job");
  for (size_t q = 0; q < 2 * P; ++q)
  {
    if (pairs[q] >= n)
    {
      return batch_fail(s, NDT2D_ERR_INVALID, who + "pair " + std::to_string(q / 2) + " names node " + std::to_string(pairs[q]) + " of " +
                                                std::to_string(n));
    }
  }
  if (poses != nullptr)
  {
    for (size_t i = 0; i < n_jobs * n * 3; ++i)
    {
      if (!std::isfinite(poses[i]))
      {
        return batch_fail(s, NDT2D_ERR_INVALID, who + "job " + std::to_string(i / (3 * n)) + " pose " + std::to_string(i / 3 % n) + " is not finite");
      }
    }
  }
  if (3 * n > cov::kMaxDim)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + std::to_string(n) + " poses, a dense matrix holds " + std::to_string(cov::kMaxDim / 3));
  }
  const size_t job_bytes = cov::job_doubles(n) * sizeof(double);
  const size_t chunk = cov::chunk_jobs(g->max_jobs, s->workspace_bytes, job_bytes);
  if (chunk == 0)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + "a job of " + std::to_string(n) + " poses needs " + std::to_string(job_bytes) +
                                              " bytes, the workspace is " + std::to_string(s->workspace_bytes));
  }
  NDT2D_BATCH_HIP(s, hipSetDevice(s->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));
  rc = ndt2d::cov_from_graph(s, ndt2d::pg_send_weights(g, stream));
  if (rc != NDT2D_OK) return rc;
  rc = ndt2d::cov_from_graph(s, ndt2d::pg_send_loss(g, stream));
  if (rc != NDT2D_OK) return rc;
  const ndt2d::PgGraph G = ndt2d::pg_device_graph(g);
  // the workspace: what the call's largest chunk needs, never more than the budget
  const size_t need = std::min(chunk, n_jobs) * job_bytes;
  if (need > s->workspace_cap)
  {
    if (s->d_workspace != nullptr) (void)hipFree(s->d_workspace);
    s->d_workspace = nullptr;
    s->workspace_cap = 0;
    NDT2D_BATCH_HIP(s, hipMalloc(&s->d_workspace, need));
    s->workspace_cap = need;
  }
  if (P != 0)
  {
    NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_pairs, &s->pairs_cap, 2 * P * sizeof(uint32_t)));
    NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_pairs, pairs, 2 * P * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  }
  s->launches.resize(cov::launch_list(3 * n, nullptr));
  (void)cov::launch_list(3 * n, s->launches.data());
  ndt2d::CovLaunch a{};
  a.n = static_cast<uint32_t>(n);
  a.n_pairs = static_cast<uint32_t>(P);
  a.damping = damping;
  a.workspace = static_cast<double *>(s->d_workspace);
  a.pairs = static_cast<const uint32_t *>(s->d_pairs);
  for (size_t k0 = 0; k0 < n_jobs; k0 += chunk)
  {
    const size_t k1 = std::min(n_jobs, k0 + chunk), kc = k1 - k0;
    rc = ndt2d::cov_from_graph(s, ndt2d::pg_send_masks(g, stream, enabled, k0, k1, &a.d_en));
    if (rc != NDT2D_OK) return rc;
    if (poses != nullptr)
    {
      NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_poses, &s->poses_cap, kc * n * 3 * sizeof(double)));
      NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_poses, poses + k0 * n * 3, kc * n * 3 * sizeof(double), hipMemcpyHostToDevice, stream));
      a.poses = static_cast<const double *>(s->d_poses);
      a.pose_stride = 3 * n;
    }
    else
    {
      a.poses = G.poses;
      a.pose_stride = 0;
    }
    // what comes back: [diagonal kc n 9 | pairs kc P 9 | records kc 3]
    const size_t at_pairs = kc * n * 9, at_rec = at_pairs + kc * P * 9, total = at_rec + kc * ndt2d::kCovRec;
    NDT2D_BATCH_HIP(s, ndt2d::grow_pair(&s->h_out, &s->d_out, &s->out_cap, total));
    a.jobs = static_cast<uint32_t>(kc);
    a.diagonal_out = s->d_out;
    a.pairs_out = s->d_out + at_pairs;
    a.records = s->d_out + at_rec;
    rc = ndt2d::batch_round_trip(s, stream, total, [&] {
      ndt2d::cov_launch(s, stream, G, a);
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
