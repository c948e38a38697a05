// The direct pose-graph solve on the device (include/ndt2d_hip.h, "Direct solve"): the CG solver's
// problem and Levenberg-Marquardt rules with an exact linear step, L L^T delta = -g on the dense
// covariance's blocked Cholesky of H_FF + lambda clamp(diag H_FF) -- a cost per iteration that does
// not depend on the closures, in launches that span the chip (gfx950 / MI355X).  The object stands
// beside an ndt2d_posegraph and reads its graph, weighting and loss; the kernels are
// direct/ndt2d_direct_kernel.h and covariance/ndt2d_covariance_kernel.h, the decisions
// direct/ndt2d_direct_step.h, a job's doubles direct/ndt2d_direct_plan.h, the panels and the factor's
// launches covariance/ndt2d_covariance_plan.h, their launch path -- the dense covariance's, on this
// unit's layout and without the inversion -- covariance/ndt2d_covariance_launch.h.  What an object
// beside the graph is made of and the prelude of a call are posegraph/ndt2d_posegraph_state.h; what
// the call refuses about its arguments is posegraph/ndt2d_posegraph_args.h.
//
// The host enqueues one iteration's launches for the chunk, reads the jobs' small states back and
// stops when no job is iterating: one read-back per LM iteration, no waiting on the device.
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
#include "direct/ndt2d_direct_kernel.h"
#include "direct/ndt2d_direct_plan.h"
#include "direct/ndt2d_direct_step.h"
#include "posegraph/ndt2d_posegraph_args.h"
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "posegraph/ndt2d_posegraph_state.h"

struct ndt2d_direct : ndt2d::PgCompanion
{
  // from the first solve on: the states of the chunk's jobs as read back (pinned)
  double * h_state = nullptr;
  size_t state_cap = 0;                // doubles
  std::vector<ndt2d::covariance::Launch> launches;   // the factor's part of the plan's list
};

namespace ndt2d
{

namespace
{

// One LM iteration of a chunk in stream order: the nodes, the fill, the assembly at each job's
// lambda, the factor's launches, the substitutions, the step.
void direct_iteration(const ndt2d_direct * s, hipStream_t stream, const PgGraph & G, const uint8_t * d_en, const DirectChunk & c, uint32_t jobs,
                      const PgRules & rules)
{
  const uint32_t n = G.n;
  CovFactorLaunch a{};
  a.jobs = jobs;
  a.d_en = d_en;
  a.poses = c.work + c.work_front;   // (PgWork's x leads a job's node arrays)
  a.pose_stride = c.work_stride;
  a.job_damping = c.state + offsetof(direct::State, lambda) / sizeof(double);
  a.damping_stride = kDirectLm;
  a.workspace = c.dense;
  a.records = c.factor;
  cov_enqueue_factor<DirectJob, false>(s->graph, stream, G, a, s->launches);
  hipLaunchKernelGGL(direct_substitute_kernel<>, dim3(jobs), dim3(kPgThreads), 0, stream, n, c, rules);
  pg_dispatch(s->graph, [&](auto, auto loss) {
    hipLaunchKernelGGL(direct_step_kernel<decltype(loss)::value>, dim3(jobs), dim3(kPgThreads), 0, stream, G, d_en, c, rules);
  });
}

// The chunk's states to the host; *iterating: whether a job takes another iteration.
int direct_fetch_states(ndt2d_direct * s, hipStream_t stream, const DirectChunk & c, size_t jobs, const direct::Rules & rules, bool * iterating)
{
  NDT2D_BATCH_HIP(s, hipGetLastError());
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_state, c.state, jobs * kDirectLm * sizeof(double), hipMemcpyDeviceToHost, stream));
  NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
  *iterating = false;
  for (size_t k = 0; k < jobs; ++k)
  {
    direct::State st;
    std::memcpy(&st, s->h_state + k * kDirectLm, sizeof(st));
    if (direct::iterating(st, rules)) *iterating = true;
  }
  return NDT2D_OK;
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_direct_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_direct ** out)
{
  NDT2D_C_TRY
  return ndt2d::pg_companion_create(posegraph, workspace_bytes, out);
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_direct_destroy(ndt2d_direct * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::pg_companion_release(s);
  if (s->h_state != nullptr) (void)hipHostFree(s->h_state);
  delete s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_direct_last_error(ndt2d_direct * s)
{
  return s != nullptr ? s->err.c_str() : "null direct";
}

int ndt2d_direct_set_timing(ndt2d_direct * s, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(s, enabled);
  NDT2D_C_CATCH(s)
}

int ndt2d_direct_last_ms(ndt2d_direct * s, float * kernel_ms, float * fetch_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(s, "direct", kernel_ms, fetch_ms);
  NDT2D_C_CATCH(s)
}

int ndt2d_direct_solve(ndt2d_direct * s, const uint8_t * enabled, size_t n_jobs, uint32_t max_iterations, double gradient_tolerance,
                       double function_tolerance, double parameter_tolerance, double * poses_out, double * records_out, double * chi2_out)
{
  NDT2D_C_TRY
  namespace cov = ndt2d::covariance;
  namespace direct = ndt2d::direct;
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  namespace args = ndt2d::pg_args;
  const char * const entry = "ndt2d_direct_solve";
  if (poses_out == nullptr || records_out == nullptr) return batch_fail(s, NDT2D_ERR_INVALID, std::string(entry) + ": null argument");
  int rc = ndt2d::batch_refuse(s, args::tolerances_refusal(entry, gradient_tolerance, function_tolerance, parameter_tolerance));
  if (rc != NDT2D_OK) return rc;
  ndt2d_posegraph * g = s->graph;
  bool loss = false;
  size_t job_bytes = 0, chunk = 0;
  ndt2d::PgCall call;
  rc = ndt2d::pg_begin_call(s, g, entry, &call, [&] {
    loss = g->loss != ndt2d::pg::kLossTrivial;
    job_bytes = direct::job_doubles(g->n, g->m, loss) * sizeof(double);
    chunk = cov::chunk_jobs(g->max_jobs, s->workspace_bytes, job_bytes);
    return args::dense_refusal(entry, g->n, cov::kMaxDim, chunk, job_bytes, s->workspace_bytes);
  });
  if (rc != NDT2D_OK) return rc;
  const hipStream_t stream = call.stream;
  const ndt2d::PgGraph & G = call.G;
  const size_t n = g->n, m = g->m;
  const ndt2d::PgRules rules{max_iterations, gradient_tolerance, function_tolerance, parameter_tolerance};
  const direct::Rules lm{max_iterations, gradient_tolerance, function_tolerance, parameter_tolerance};
  // the workspace: what the call's largest chunk needs, never more than the budget
  const size_t held = std::min(chunk, n_jobs);
  rc = ndt2d::pg_companion_workspace(s, held * job_bytes);
  if (rc != NDT2D_OK) return rc;
  if (held * ndt2d::kDirectLm > s->state_cap)
  {
    if (s->h_state != nullptr) (void)hipHostFree(s->h_state);
    s->h_state = nullptr;
    s->state_cap = 0;
    NDT2D_BATCH_HIP(s, hipHostMalloc(reinterpret_cast<void **>(&s->h_state), held * ndt2d::kDirectLm * sizeof(double), hipHostMallocDefault));
    s->state_cap = held * ndt2d::kDirectLm;
  }
  ndt2d::cov_launch_list(3 * n, false, &s->launches);   // the factor's launches only
  // the regions of the workspace: [held] dense | work | state | the factor's records
  ndt2d::DirectChunk c{};
  c.dense = static_cast<double *>(s->d_workspace);
  c.work = c.dense + held * direct::dense_doubles(n);
  c.work_stride = direct::work_doubles(n, m, loss);
  c.work_front = loss ? m : 0;
  c.state = c.work + held * c.work_stride;
  c.factor = c.state + held * ndt2d::kDirectLm;
  for (size_t k0 = 0; k0 < n_jobs; k0 += chunk)
  {
    const size_t k1 = std::min(n_jobs, k0 + chunk), kc = k1 - k0;
    const uint32_t jobs = static_cast<uint32_t>(kc);
    const uint8_t * d_en = nullptr;
    rc = ndt2d::pg_relay(s, g, ndt2d::pg_send_masks(g, stream, enabled, k0, k1, &d_en));
    if (rc != NDT2D_OK) return rc;
    // what comes back: [poses kc n 3 | records kc 8 | chi2 kc 2 m (start, end)]
    const size_t at_rec = kc * n * 3, at_chi2 = at_rec + kc * ndt2d::kDirectRec;
    const size_t total = at_chi2 + (chi2_out != nullptr ? kc * 2 * m : 0);
    NDT2D_BATCH_HIP(s, ndt2d::grow_pair(&s->h_out, &s->d_out, &s->out_cap, total));
    rc = ndt2d::batch_round_trip(s, stream, total, [&]() -> int {
      if (chi2_out != nullptr)
      {
        hipLaunchKernelGGL(ndt2d::direct_chi2_kernel, dim3(jobs), dim3(ndt2d::kPgThreads), 0, stream, G, G.poses, size_t(0), s->d_out + at_chi2,
                           2 * m);
      }
      ndt2d::pg_dispatch(g, [&](auto, auto loss_kind) {
        hipLaunchKernelGGL(ndt2d::direct_begin_kernel<decltype(loss_kind)::value>, dim3(jobs), dim3(ndt2d::kPgThreads), 0, stream, G, d_en, c,
                           rules);
      });
      bool iterating = false;
      int rc_fetch = ndt2d::direct_fetch_states(s, stream, c, kc, lm, &iterating);
      if (rc_fetch != NDT2D_OK) return rc_fetch;
      for (uint32_t it = 0; it < max_iterations && iterating; ++it)
      {
        ndt2d::direct_iteration(s, stream, G, d_en, c, jobs, rules);
        rc_fetch = ndt2d::direct_fetch_states(s, stream, c, kc, lm, &iterating);
        if (rc_fetch != NDT2D_OK) return rc_fetch;
      }
      hipLaunchKernelGGL(ndt2d::direct_finish_kernel, dim3(jobs), dim3(ndt2d::kDirectFinishThreads), 0, stream, static_cast<uint32_t>(n), c,
                         s->d_out, s->d_out + at_rec);
      if (chi2_out != nullptr)
      {
        NDT2D_BATCH_HIP(s, hipGetLastError());
        hipLaunchKernelGGL(ndt2d::direct_chi2_kernel, dim3(jobs), dim3(ndt2d::kPgThreads), 0, stream, G, s->d_out, 3 * n, s->d_out + at_chi2 + m,
                           2 * m);
      }
      return NDT2D_OK;
    });
    if (rc != NDT2D_OK) return rc;
    std::memcpy(poses_out + k0 * n * 3, s->h_out, kc * n * 3 * sizeof(double));
    std::memcpy(records_out + k0 * ndt2d::kDirectRec, s->h_out + at_rec, kc * ndt2d::kDirectRec * sizeof(double));
    if (chi2_out != nullptr && m != 0) std::memcpy(chi2_out + k0 * 2 * m, s->h_out + at_chi2, kc * 2 * m * sizeof(double));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
