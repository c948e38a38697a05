// The sparse covariance of the pose graph on the device (include/ndt2d_hip.h, "Sparse covariance"):
// every node's 3 x 3 diagonal block and chosen (a, b) blocks of
// (H_FF + damping clamp(diag H_FF))^-1 from the sparse solve's factorisation -- the block cyclic
// reduction of the interior chain and the dense Cholesky of the separators' Schur complement S --
// in O(n) + O(s^3), without a dense 3n x 3n matrix (gfx950 / MI355X).  The object stands beside an
// ndt2d_posegraph and reads its graph, weighting and loss.  The new kernels are
// sparsecov/ndt2d_sparsecov_kernel.h, the plan and the lists sparsecov/ndt2d_sparsecov_plan.h, the
// arithmetic sparsecov/ndt2d_sparsecov_select.h.  Launched, not copied: the sparse solve's assemble,
// reduce and Schur kernels (sparse/ndt2d_sparse_kernel.h), the dense fill, factor and inversion
// (covariance/ndt2d_covariance_kernel.h through covariance/ndt2d_covariance_launch.h).  What an object
// beside the graph is made of, the prelude of a call and a chunk's poses are
// posegraph/ndt2d_posegraph_state.h; what the call refuses about its arguments is
// posegraph/ndt2d_posegraph_args.h.
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
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "posegraph/ndt2d_posegraph_state.h"
#include "sparse/ndt2d_sparse_kernel.h"
#include "sparse/ndt2d_sparse_plan.h"
#include "sparsecov/ndt2d_sparsecov_kernel.h"
#include "sparsecov/ndt2d_sparsecov_plan.h"

struct ndt2d_sparsecov : ndt2d::PgCompanion
{
  // from the first compute on: the layout of the graph as the last call found it, the lists of the
  // last call's pairs, both on the device in one array of words, the chunk's poses where the caller
  // gives them
  ndt2d::sparse::Layout layout;
  ndt2d::sparsecov::Lists lists;
  void * d_words = nullptr;
  size_t words_cap = 0;
  ndt2d::PgPoses poses;
  std::vector<ndt2d::covariance::Launch> launches;   // the factor's and the inversion's for 3 s unknowns
};

namespace ndt2d
{

namespace
{

// What a chunk's launches take beside the chunk itself.
struct SparsecovLaunch
{
  uint32_t jobs;
  const uint8_t * d_en;
  const double * poses;
  size_t pose_stride;
  double damping;
  double * diagonal_out, * pairs_out, * records_out;
};

// A chunk in stream order: the linearisation at each job's poses with lambda = the damping, the fill
// of S and T, the band and S's own blocks, the reduction, the Schur terms, S = L L^T and T = L^-1,
// the blocks of S^-1, the selected inversion, the column passes, the diagonal, the pairs.  Without a
// separator nothing dense is launched.
void sparsecov_enqueue(const ndt2d_sparsecov * s, hipStream_t stream, const PgGraph & G, const SparsecovChunk & c, const sparse::Tables & t,
                       const SparsecovLaunch & a)
{
  const uint32_t n = G.n, jobs = a.jobs;
  const PgRules once{1u, 0.0, 0.0, 0.0};   // the sparse solve's kernels work on a job that has an iteration to take
  const dim3 per_node((n + kSparseNodeThreads - 1) / kSparseNodeThreads, 1, jobs);
  pg_dispatch(s->graph, [&](auto, auto loss) {
    hipLaunchKernelGGL(sparsecov_begin_kernel<decltype(loss)::value>, dim3(jobs), dim3(kPgThreads), 0, stream, G, a.d_en, a.poses, a.pose_stride,
                       a.damping, c);
  });
  if (t.s != 0) cov_enqueue_fill<SparsecovJob>(stream, t.s, jobs, c.sparse.dense);
  pg_dispatch(s->graph, [&](auto, auto loss) {
    hipLaunchKernelGGL(sparse_assemble_kernel<decltype(loss)::value>, per_node, dim3(kSparseNodeThreads), 0, stream, G, a.d_en, c.sparse, t);
  });
  if (t.s != 0)
  {
    hipLaunchKernelGGL(sparse_reduce_kernel<sparse::kColumns>, dim3(jobs), dim3(kPgThreads), 0, stream, c.sparse, t.ni, once);
    hipLaunchKernelGGL(sparse_schur_kernel, dim3((t.s + kSparseNodeThreads - 1) / kSparseNodeThreads, 1, jobs), dim3(kSparseNodeThreads), 0, stream, n,
                       c.sparse, t);
    cov_enqueue_launches<SparsecovJob, true>(stream, t.s, jobs, c.sparse.dense, c.sparse.factor, s->launches);
    hipLaunchKernelGGL(sparsecov_blocks_kernel, dim3(c.n_blocks, 1, jobs), dim3(kWave), 0, stream, t.s, c);
  }
  else
  {
    hipLaunchKernelGGL(sparse_reduce_kernel<1>, dim3(jobs), dim3(kPgThreads), 0, stream, c.sparse, t.ni, once);
  }
  if (t.ni != 0) hipLaunchKernelGGL(sparsecov_select_kernel, dim3(jobs), dim3(kPgThreads), 0, stream, c, t.ni);
  if (t.ni != 0 && c.n_passes != 0) hipLaunchKernelGGL(sparsecov_columns_kernel, dim3(jobs), dim3(kPgThreads), 0, stream, c, t);
  hipLaunchKernelGGL(sparsecov_diagonal_kernel, dim3((n + kSparsecovThreads - 1) / kSparsecovThreads, 1, jobs), dim3(kSparsecovThreads), 0, stream, n, c,
                     t, a.diagonal_out, a.records_out);
  if (c.n_pairs != 0)
  {
    hipLaunchKernelGGL(sparsecov_pairs_kernel, dim3((c.n_pairs + kSparsecovThreads - 1) / kSparsecovThreads, 1, jobs), dim3(kSparsecovThreads), 0,
                       stream, n, c, t, a.pairs_out);
  }
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_sparsecov_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, ndt2d_sparsecov ** out)
{
  NDT2D_C_TRY
  return ndt2d::pg_companion_create(posegraph, workspace_bytes, out);
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_sparsecov_destroy(ndt2d_sparsecov * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::pg_companion_release(s);
  for (void * p : {s->poses.d, s->d_words})
  {
    if (p != nullptr) (void)hipFree(p);
  }
  delete s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_sparsecov_last_error(ndt2d_sparsecov * s)
{
  return s != nullptr ? s->err.c_str() : "null sparsecov";
}

int ndt2d_sparsecov_set_timing(ndt2d_sparsecov * s, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(s, enabled);
  NDT2D_C_CATCH(s)
}

int ndt2d_sparsecov_last_ms(ndt2d_sparsecov * s, float * kernel_ms, float * fetch_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(s, "sparsecov", kernel_ms, fetch_ms);
  NDT2D_C_CATCH(s)
}

int ndt2d_sparsecov_compute(ndt2d_sparsecov * s, const uint8_t * enabled, size_t n_jobs, const double * poses, double damping,
                            const uint32_t * pairs, size_t n_pairs, double * diagonal_out, double * pairs_out, double * records_out)
{
  NDT2D_C_TRY
  namespace sparse = ndt2d::sparse;
  namespace sparsecov = ndt2d::sparsecov;
  namespace args = ndt2d::pg_args;
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  const char * const entry = "ndt2d_sparsecov_compute";
  const std::string who = std::string(entry) + ": ";
  if (diagonal_out == nullptr || records_out == nullptr || (n_pairs != 0 && (pairs == nullptr || pairs_out == nullptr)))
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + "null argument");
  }
  int rc = ndt2d::batch_refuse(s, args::damping_refusal(entry, damping));
  if (rc != NDT2D_OK) return rc;
  ndt2d_posegraph * g = s->graph;
  const size_t P = n_pairs;
  bool loss = false;
  size_t job_bytes = 0, chunk = 0;
  ndt2d::PgCall call;
  rc = ndt2d::pg_begin_call(s, g, entry, &call, [&] {
    if (P > 0x7FFFFFFFu - g->n) return who + "more than 2^31 - 1 blocks a job";
    std::string refusal = args::nodes_refusal(entry, "pair", pairs, P, 2, g->n);
    if (refusal.empty()) refusal = args::poses_refusal(entry, poses, n_jobs, g->n);
    if (!refusal.empty()) return refusal;
    loss = g->loss != ndt2d::pg::kLossTrivial;
    sparse::make_layout(g->n, g->m, g->index.data(), g->index.data() + g->m, &s->layout);
    sparsecov::make_lists(s->layout.tables(), pairs, P, &s->lists);
    job_bytes = sparsecov::job_doubles(g->n, s->layout.s, g->m, loss, s->lists.n_blocks(), P) * sizeof(double);
    chunk = sparsecov::chunk_jobs(g->max_jobs, s->workspace_bytes, job_bytes);
    return sparsecov::refusal(entry, g->n, s->layout.s, s->lists.n_blocks(), P, chunk, job_bytes, s->workspace_bytes);
  });
  if (rc != NDT2D_OK) return rc;
  const hipStream_t stream = call.stream;
  const ndt2d::PgGraph & G = call.G;
  const size_t n = g->n, m = g->m, ns = s->layout.s, ni = s->layout.ni;
  const size_t n_blocks = s->lists.n_blocks(), n_passes = s->lists.n_passes();
  // the tables and the lists on the device: [tables | blocks | pairs | passes]
  const size_t table_words = s->layout.words.size(), words = table_words + sparsecov::list_words(n_blocks, P, n_passes);
  NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_words, &s->words_cap, words * sizeof(uint32_t)));
  uint32_t * d_words = static_cast<uint32_t *>(s->d_words);
  const auto send = [&](size_t at, const std::vector<uint32_t> & from) -> hipError_t {
    if (from.empty()) return hipSuccess;
    return hipMemcpyAsync(d_words + at, from.data(), from.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
  };
  NDT2D_BATCH_HIP(s, send(0, s->layout.words));
  NDT2D_BATCH_HIP(s, send(table_words, s->lists.blocks));
  NDT2D_BATCH_HIP(s, send(table_words + 2 * n_blocks, s->lists.pairs));
  NDT2D_BATCH_HIP(s, send(table_words + 2 * n_blocks + sparsecov::kPairWords * P, s->lists.passes));
  const sparse::Tables t = sparse::tables_at(d_words, n, ns);
  // the workspace: what the call's largest chunk needs, never more than the budget
  const size_t held = std::min(chunk, n_jobs);
  rc = ndt2d::pg_companion_workspace(s, held * job_bytes);
  if (rc != NDT2D_OK) return rc;
  ndt2d::cov_launch_list(3 * ns, true, &s->launches);
  // the regions of the workspace: [held] inverse (descending) | schur | interior | select | vectors | blocks | columns | work | state |
  // the factor's records | the reduction's flags
  ndt2d::SparsecovChunk c{};
  c.sparse.dense = static_cast<double *>(s->d_workspace) + held * sparsecov::inverse_doubles(ns);
  c.sparse.interior = c.sparse.dense + held * sparse::schur_doubles(ns);
  c.select = c.sparse.interior + held * sparse::interior_doubles(ni);
  c.sparse.vectors = c.select + held * sparsecov::select_doubles(ni);
  c.blocks = c.sparse.vectors + held * sparse::vector_doubles(ns);
  c.columns = c.blocks + held * 9 * n_blocks;
  c.sparse.lm.dense = nullptr;
  c.sparse.lm.work = c.columns + held * 9 * P;
  c.sparse.lm.work_stride = sparse::work_doubles(n, m, loss);
  c.sparse.lm.work_front = loss ? m : 0;
  c.sparse.lm.state = c.sparse.lm.work + held * c.sparse.lm.work_stride;
  c.sparse.lm.factor = c.sparse.lm.state + held * ndt2d::kDirectLm;
  c.sparse.factor = c.sparse.lm.factor;
  c.sparse.reduction = c.sparse.factor + held * ndt2d::kCovRec;
  c.n_blocks = static_cast<uint32_t>(n_blocks);
  c.n_pairs = static_cast<uint32_t>(P);
  c.n_passes = static_cast<uint32_t>(n_passes);
  c.block_list = d_words + table_words;
  c.pair_list = c.block_list + 2 * n_blocks;
  c.pass_list = c.pair_list + sparsecov::kPairWords * P;
  ndt2d::SparsecovLaunch a{};
  a.damping = damping;
  for (size_t k0 = 0; k0 < n_jobs; k0 += chunk)
  {
    const size_t k1 = std::min(n_jobs, k0 + chunk), kc = k1 - k0;
    rc = ndt2d::pg_relay(s, g, ndt2d::pg_send_masks(g, stream, enabled, k0, k1, &a.d_en));
    if (rc != NDT2D_OK) return rc;
    rc = ndt2d::pg_chunk_poses(s, stream, &s->poses, poses, k0, kc, n, G, &a.poses, &a.pose_stride);
    if (rc != NDT2D_OK) return rc;
    // what comes back: [diagonal kc n 9 | pairs kc P 9 | records kc 3]
    const size_t at_pairs = kc * n * 9, at_rec = at_pairs + kc * P * 9, total = at_rec + kc * ndt2d::kSparsecovRec;
    NDT2D_BATCH_HIP(s, ndt2d::grow_pair(&s->h_out, &s->d_out, &s->out_cap, total));
    a.jobs = static_cast<uint32_t>(kc);
    a.diagonal_out = s->d_out;
    a.pairs_out = s->d_out + at_pairs;
    a.records_out = s->d_out + at_rec;
    rc = ndt2d::batch_round_trip(s, stream, total, [&] {
      ndt2d::sparsecov_enqueue(s, stream, G, c, t, a);
      return NDT2D_OK;
    });
    if (rc != NDT2D_OK) return rc;
    std::memcpy(diagonal_out + k0 * n * 9, s->h_out, kc * n * 9 * sizeof(double));
    if (P != 0) std::memcpy(pairs_out + k0 * P * 9, s->h_out + at_pairs, kc * P * 9 * sizeof(double));
    std::memcpy(records_out + k0 * ndt2d::kSparsecovRec, s->h_out + at_rec, kc * ndt2d::kSparsecovRec * sizeof(double));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
