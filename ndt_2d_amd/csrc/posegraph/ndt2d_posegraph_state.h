// The pose-graph object and what the units round it share on the host (posegraph/ndt2d_posegraph.hip:
// the object's life, the graph, evaluate and solve; posegraph/ndt2d_posegraph_robust.hip: the losses'
// entry points; posegraph/ndt2d_posegraph_marginals.hip: the marginal covariances): the object, the
// graph as its kernels take it, the uploads a call makes before its first launch, and the one place
// where the object's preconditioner and loss become a kernel's template arguments.
// Included by the .hip translation units only.
#ifndef NDT2D_POSEGRAPH_STATE_H_
#define NDT2D_POSEGRAPH_STATE_H_

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "posegraph/ndt2d_posegraph_kernel.h"

struct ndt2d_posegraph : ndt2d::BatchHost
{
  size_t max_nodes = 0, max_constraints = 0, max_jobs = 0;
  bool information_weighting = false;   // W = L^T instead of L
  bool chain = false;                   // the CG's preconditioner: "chain" instead of "jacobi"
  bool has_graph = false, weights_sent = false;
  int loss = ndt2d::posegraph::kLossTrivial;   // the loss (kLoss*), its scale, and whether the device has them
  double loss_scale = 1.0;
  bool loss_sent = false;
  std::vector<uint8_t> robust;          // [m] the constraints the loss applies to; empty: every one
  size_t n = 0, m = 0, fixed = 0;
  std::vector<double> chol;             // [m][9] the lower Cholesky factors
  std::vector<double> stage;            // what an upload is put together in
  std::vector<uint32_t> index;
  // on the device: [poses 3 n | transforms 3 m | W 9 m | the loss's a, b], [begin m | end m | node_ptr n + 1 |
  // node_con 2 m | the loss's selection, m bytes], the chunk's masks, the chunk's workspaces
  void * d_graph = nullptr, * d_index = nullptr, * d_enabled = nullptr, * d_work = nullptr;
  size_t graph_cap = 0, index_cap = 0, enabled_cap = 0, work_cap = 0;
  // marginal covariances, from the first ndt2d_marginals_columns on: the chunk's job blocks and
  // (job, query) workspaces, the chunk's poses where the caller gives them, the query nodes
  void * d_marginals = nullptr, * d_marginal_poses = nullptr, * d_marginal_nodes = nullptr;
  size_t marginals_cap = 0, marginal_poses_cap = 0, marginal_nodes_cap = 0;
  size_t compute_units = 0;             // of the device, asked at the first ndt2d_marginals_columns
};

namespace ndt2d
{

namespace
{

// (inline here, not among the declarations below: PgGraph is each unit's own type, as its kernels are)
inline PgGraph pg_device_graph(const ndt2d_posegraph * s)
{
  PgGraph G{};
  const double * d = static_cast<const double *>(s->d_graph);
  const uint32_t * u = static_cast<const uint32_t *>(s->d_index);
  G.poses = d;
  G.transform = d + 3 * s->n;
  G.W = d + 3 * s->n + 3 * s->m;
  G.begin = u;
  G.end = u + s->m;
  G.node_ptr = u + 2 * s->m;
  G.node_con = u + 2 * s->m + s->n + 1;
  G.n = static_cast<uint32_t>(s->n);
  G.m = static_cast<uint32_t>(s->m);
  G.fixed = static_cast<uint32_t>(s->fixed);
  return G;
}

constexpr const char * kPgLossNames[3] = {"trivial", "huber", "cauchy"};

// The object's preconditioner and loss as compile-time constants: f(prec, loss) with
// std::integral_constant<int, kPgJacobi or kPgChain> and <int, pg::kLossTrivial, kLossHuber or
// kLossCauchy>, for a launch to take its template arguments from.
template <class F>
void pg_dispatch(const ndt2d_posegraph * s, F f)
{
  const auto with = [&](auto loss) {
    if (s->chain) f(std::integral_constant<int, kPgChain>{}, loss);
    else f(std::integral_constant<int, kPgJacobi>{}, loss);
  };
  if (s->loss == pg::kLossHuber) with(std::integral_constant<int, pg::kLossHuber>{});
  else if (s->loss == pg::kLossCauchy) with(std::integral_constant<int, pg::kLossCauchy>{});
  else with(std::integral_constant<int, pg::kLossTrivial>{});
}

}  // namespace

// ---- defined in posegraph/ndt2d_posegraph.hip; not part of the C-ABI ----

// W of every constraint by the weighting in force, behind a change of either.
__attribute__((visibility("hidden"))) int pg_send_weights(ndt2d_posegraph * s, hipStream_t stream);
// The loss's scale and selection beside the graph (PgLoss), behind a change of either; nothing
// without a loss.
__attribute__((visibility("hidden"))) int pg_send_loss(ndt2d_posegraph * s, hipStream_t stream);
// The masks of jobs [k0, k1) on the device, or NULL for none.
__attribute__((visibility("hidden"))) int pg_send_masks(ndt2d_posegraph * s, hipStream_t stream, const uint8_t * enabled, size_t k0, size_t k1, const uint8_t ** out);
// A job's workspace in doubles: the node arrays, the chain's where it is selected, rho' per
// constraint under a loss.
__attribute__((visibility("hidden"))) size_t pg_job_doubles(const ndt2d_posegraph * s);
// kLoss* of a loss's name, -1 for none.
__attribute__((visibility("hidden"))) int pg_loss_kind(const char * kind);
// NDT2D_OK, or NDT2D_ERR_STATE with its text where the object has no graph yet.
__attribute__((visibility("hidden"))) int pg_ready(ndt2d_posegraph * s, const char * who);

}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_STATE_H_
