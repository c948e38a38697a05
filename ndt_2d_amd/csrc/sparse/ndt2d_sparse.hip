// The sparse pose-graph solve on the device (include/ndt2d_hip.h, "Sparse solve"): the direct solve's
// problem and Levenberg-Marquardt rules with the exact linear step taken sparsely -- the graph's
// chain by one block cyclic reduction over the interior nodes, the nodes closures touch by a dense
// Cholesky of their Schur complement -- so that an iteration costs O(n) + O(s^3) and needs no
// 3n x 3n matrix (gfx950 / MI355X).  The object stands beside an ndt2d_posegraph and reads its graph,
// weighting and loss; the new kernels are sparse/ndt2d_sparse_kernel.h, the plan and the tables
// sparse/ndt2d_sparse_plan.h, the linear step's arithmetic sparse/ndt2d_sparse_schur.h; the begin,
// step, finish, chi2 and substitution kernels are direct/ndt2d_direct_kernel.h's, the decisions
// direct/ndt2d_direct_step.h, the factor of the separators' matrix covariance/ndt2d_covariance_kernel.h
// through covariance/ndt2d_covariance_launch.h.  What an object beside the graph is made of and the
// prelude of a call are posegraph/ndt2d_posegraph_state.h.
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
#include "direct/ndt2d_direct_step.h"
#include "posegraph/ndt2d_posegraph_args.h"
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "posegraph/ndt2d_posegraph_state.h"
#include "sparse/ndt2d_sparse_kernel.h"
#include "sparse/ndt2d_sparse_plan.h"

struct ndt2d_sparse : ndt2d::PgCompanion
{
  // from the first solve on: the states of the chunk's jobs as read back (pinned), the layout of
  // the graph as the last solve found it and its tables on the device
  double * h_state = nullptr;
  size_t state_cap = 0;                // doubles
  ndt2d::sparse::Layout layout;
  void * d_tables = nullptr;
  size_t tables_cap = 0;
  std::vector<ndt2d::covariance::Launch> launches;   // the factor's part of the plan's list for 3 s unknowns
};

namespace ndt2d
{

namespace
{

// The layout of the graph in place (its begin and end as the host keeps them).
void sparse_layout_of(const ndt2d_posegraph * g, sparse::Layout * out)
{
  sparse::make_layout(g->n, g->m, g->index.data(), g->index.data() + g->m, out);
}

// One LM iteration of a chunk in stream order: the fill of S, the band and S's own blocks at each
// job's lambda, the reduction, the Schur terms, S's factor, the substitution on it, the expansion,
// the step.  Without a separator nothing dense is launched.
void sparse_iteration(const ndt2d_sparse * s, hipStream_t stream, const PgGraph & G, const uint8_t * d_en, const SparseChunk & c,
                      const sparse::Tables & t, uint32_t jobs, const PgRules & rules)
{
  const uint32_t n = G.n;
  const dim3 per_node((n + kSparseNodeThreads - 1) / kSparseNodeThreads, 1, jobs);
  if (t.s != 0) cov_enqueue_fill<SparseJob>(stream, t.s, jobs, c.dense);
  pg_dispatch(s->graph, [&](auto, auto loss) {
    hipLaunchKernelGGL(sparse_assemble_kernel<decltype(loss)::value>, per_node, dim3(kSparseNodeThreads), 0, stream, G, d_en, c, t);
  });
  if (t.s != 0)
  {
    hipLaunchKernelGGL(sparse_reduce_kernel<sparse::kColumns>, dim3(jobs), dim3(kPgThreads), 0, stream, c, t.ni, rules);
    hipLaunchKernelGGL(sparse_schur_kernel, dim3((t.s + kSparseNodeThreads - 1) / kSparseNodeThreads, 1, jobs), dim3(kSparseNodeThreads), 0, stream, n,
                       c, t);
    cov_enqueue_launches<SparseJob, false>(stream, t.s, jobs, c.dense, c.factor, s->launches);
    hipLaunchKernelGGL(direct_substitute_kernel<SparseChunk>, dim3(jobs), dim3(kPgThreads), 0, stream, t.s, c, rules);
  }
  else
  {
    hipLaunchKernelGGL(sparse_reduce_kernel<1>, dim3(jobs), dim3(kPgThreads), 0, stream, c, t.ni, rules);
  }
  hipLaunchKernelGGL(sparse_expand_kernel, dim3((n + kSparseExpandThreads - 1) / kSparseExpandThreads, 1, jobs), dim3(kSparseExpandThreads), 0, stream,
                     n, c, t);
  pg_dispatch(s->graph, [&](auto, auto loss) {
    hipLaunchKernelGGL(direct_step_kernel<decltype(loss)::value>, dim3(jobs), dim3(kPgThreads), 0, stream, G, d_en, c.lm, rules);
  });
}

// The chunk's states to the host; *iterating: whether a job takes another iteration.
int sparse_fetch_states(ndt2d_sparse * s, hipStream_t stream, const SparseChunk & c, size_t jobs, const direct::Rules & rules, bool * iterating)
{
  NDT2D_BATCH_HIP(s, hipGetLastError());
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_state, c.lm.state, jobs * kDirectLm * sizeof(double), hipMemcpyDeviceToHost, stream));
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

int ndt2d_sparse_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_sparse ** out)
{
  NDT2D_C_TRY
  return ndt2d::pg_companion_create(posegraph, workspace_bytes, out);
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_sparse_destroy(ndt2d_sparse * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::pg_companion_release(s);
  if (s->h_state != nullptr) (void)hipHostFree(s->h_state);
  if (s->d_tables != nullptr) (void)hipFree(s->d_tables);
  delete s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_sparse_last_error(ndt2d_sparse * s)
{
  return s != nullptr ? s->err.c_str() : "null sparse";
}

int ndt2d_sparse_set_timing(ndt2d_sparse * s, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(s, enabled);
  NDT2D_C_CATCH(s)
}

int ndt2d_sparse_last_ms(ndt2d_sparse * s, float * kernel_ms, float * fetch_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(s, "sparse", kernel_ms, fetch_ms);
  NDT2D_C_CATCH(s)
}

int ndt2d_sparse_layout(ndt2d_sparse * s, size_t * n_separators, size_t * n_interior)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_separators == nullptr || n_interior == nullptr) return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_sparse_layout: null argument");
  const int rc = ndt2d::pg_relay(s, s->graph, ndt2d::pg_ready(s->graph, "ndt2d_sparse_layout"));
  if (rc != NDT2D_OK) return rc;
  ndt2d::sparse_layout_of(s->graph, &s->layout);
  *n_separators = s->layout.s;
  *n_interior = s->layout.ni;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_sparse_solve(ndt2d_sparse * s, const uint8_t * enabled, size_t n_jobs, uint32_t max_iterations, double gradient_tolerance,
                       double function_tolerance, double parameter_tolerance, double * poses_out, double * records_out, double * chi2_out)
{
  NDT2D_C_TRY
  namespace cov = ndt2d::covariance;
  namespace direct = ndt2d::direct;
  namespace sparse = ndt2d::sparse;
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  namespace args = ndt2d::pg_args;
  const char * const entry = "ndt2d_sparse_solve";
  if (poses_out == nullptr || records_out == nullptr) return batch_fail(s, NDT2D_ERR_INVALID, std::string(entry) + ": null argument");
  int rc = ndt2d::batch_refuse(s, args::tolerances_refusal(entry, gradient_tolerance, function_tolerance, parameter_tolerance));
  if (rc != NDT2D_OK) return rc;
  ndt2d_posegraph * g = s->graph;
  bool loss = false;
  size_t job_bytes = 0, chunk = 0;
  ndt2d::PgCall call;
  rc = ndt2d::pg_begin_call(s, g, entry, &call, [&] {
    loss = g->loss != ndt2d::pg::kLossTrivial;
    ndt2d::sparse_layout_of(g, &s->layout);
    job_bytes = sparse::job_doubles(g->n, s->layout.s, g->m, loss) * sizeof(double);
    chunk = sparse::chunk_jobs(g->max_jobs, s->workspace_bytes, job_bytes);
    return sparse::refusal(entry, g->n, s->layout.s, chunk, job_bytes, s->workspace_bytes);
  });
  if (rc != NDT2D_OK) return rc;
  const hipStream_t stream = call.stream;
  const ndt2d::PgGraph & G = call.G;
  const size_t n = g->n, m = g->m, ns = s->layout.s, ni = s->layout.ni;
  const ndt2d::PgRules rules{max_iterations, gradient_tolerance, function_tolerance, parameter_tolerance};
  const direct::Rules lm{max_iterations, gradient_tolerance, function_tolerance, parameter_tolerance};
  // the tables on the device
  NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_tables, &s->tables_cap, s->layout.words.size() * sizeof(uint32_t)));
  if (!s->layout.words.empty())
  {
    NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_tables, s->layout.words.data(), s->layout.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  }
  const sparse::Tables t = sparse::tables_at(static_cast<const uint32_t *>(s->d_tables), n, ns);
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
  ndt2d::cov_launch_list(3 * ns, false, &s->launches);   // the factor's launches only
  // the regions of the workspace: [held] schur | interior | vectors | work | state | the factor's records | the reduction's flags
  ndt2d::SparseChunk c{};
  c.dense = static_cast<double *>(s->d_workspace);
  c.interior = c.dense + held * sparse::schur_doubles(ns);
  c.vectors = c.interior + held * sparse::interior_doubles(ni);
  c.lm.dense = nullptr;
  c.lm.work = c.vectors + held * sparse::vector_doubles(ns);
  c.lm.work_stride = sparse::work_doubles(n, m, loss);
  c.lm.work_front = loss ? m : 0;
  c.lm.state = c.lm.work + held * c.lm.work_stride;
  c.lm.factor = c.lm.state + held * ndt2d::kDirectLm;
  c.factor = c.lm.factor;
  c.reduction = c.factor + held * ndt2d::kCovRec;
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
        hipLaunchKernelGGL(ndt2d::direct_begin_kernel<decltype(loss_kind)::value>, dim3(jobs), dim3(ndt2d::kPgThreads), 0, stream, G, d_en, c.lm,
                           rules);
      });
      bool iterating = false;
      int rc_fetch = ndt2d::sparse_fetch_states(s, stream, c, kc, lm, &iterating);
      if (rc_fetch != NDT2D_OK) return rc_fetch;
      for (uint32_t it = 0; it < max_iterations && iterating; ++it)
      {
        ndt2d::sparse_iteration(s, stream, G, d_en, c, t, jobs, rules);
        rc_fetch = ndt2d::sparse_fetch_states(s, stream, c, kc, lm, &iterating);
        if (rc_fetch != NDT2D_OK) return rc_fetch;
      }
      hipLaunchKernelGGL(ndt2d::direct_finish_kernel, dim3(jobs), dim3(ndt2d::kDirectFinishThreads), 0, stream, static_cast<uint32_t>(n), c.lm,
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
