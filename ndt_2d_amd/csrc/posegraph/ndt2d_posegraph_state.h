// The pose-graph object and what the units round it share on the host (posegraph/ndt2d_posegraph.hip:
// the object's life, the graph, evaluate and solve; posegraph/ndt2d_posegraph_robust.hip: the losses'
// entry points; posegraph/ndt2d_posegraph_marginals.hip: the marginal covariances; the dense
// covariance's and the direct solve's units, whose objects stand beside this one): the object, the
// graph as its kernels take it, the one prelude every call makes before its first launch
// (pg_begin_call), a chunk's poses (pg_chunk_poses), what an object beside the graph is made of
// (PgCompanion), and the one place where the object's preconditioner and loss become a kernel's
// template arguments.  What the calls refuse about their arguments is posegraph/ndt2d_posegraph_args.h.
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

namespace ndt2d
{

// A chunk's poses on the device where the caller gives them (pg_chunk_poses).
struct PgPoses
{
  void * d = nullptr;
  size_t cap = 0;
};

}  // namespace ndt2d

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
  void * d_marginals = nullptr, * d_marginal_nodes = nullptr;
  size_t marginals_cap = 0, marginal_nodes_cap = 0;
  ndt2d::PgPoses marginal_poses;
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

// ---- what every call on a graph begins with, and the objects that stand beside one ----

// What a call of the graph's own left in the graph, as the error of the object the call was made on
// (the graph itself, or an object beside it).
inline int pg_relay(BatchHost * owner, const ndt2d_posegraph * g, int rc)
{
  if (rc != NDT2D_OK && owner != g) owner->err = g->err;
  return rc;
}

namespace
{

// What a call launches on: the context's stream and the graph as the kernels take it.
struct PgCall
{
  hipStream_t stream;
  PgGraph G;
};

// The prelude of every call on a graph, in this order: the graph is there (pg_ready), what the entry
// refuses about arguments that are checked against the graph (refuse(): a text of
// posegraph/ndt2d_posegraph_args.h's kind, or an empty string), the device, the stream, W and the
// loss on the device, the graph as the kernels take it.  owner: the object whose `err` receives the
// text -- the graph, or the object beside it the call was made on.
template <class REFUSE>
int pg_begin_call(BatchHost * owner, ndt2d_posegraph * g, const char * entry, PgCall * call, REFUSE refuse)
{
  int rc = pg_relay(owner, g, pg_ready(g, entry));
  if (rc != NDT2D_OK) return rc;
  rc = batch_refuse(owner, refuse());
  if (rc != NDT2D_OK) return rc;
  NDT2D_BATCH_HIP(owner, hipSetDevice(owner->device));
  call->stream = static_cast<hipStream_t>(ndt2d_get_stream(owner->h));
  rc = pg_relay(owner, g, pg_send_weights(g, call->stream));
  if (rc != NDT2D_OK) return rc;
  rc = pg_relay(owner, g, pg_send_loss(g, call->stream));
  if (rc != NDT2D_OK) return rc;
  call->G = pg_device_graph(g);
  return NDT2D_OK;
}

inline int pg_begin_call(BatchHost * owner, ndt2d_posegraph * g, const char * entry, PgCall * call)
{
  return pg_begin_call(owner, g, entry, call, [] { return std::string(); });
}

// The poses of the chunk's jobs [k0, k0 + kc) of n nodes: the caller's, uploaded into `buffer`, a
// job 3 n doubles behind the last; or (poses NULL) the graph's for every job, at a stride of 0.
inline int pg_chunk_poses(BatchHost * owner, hipStream_t stream, PgPoses * buffer, const double * poses, size_t k0, size_t kc, size_t n,
                          const PgGraph & G, const double ** out, size_t * stride)
{
  *out = G.poses;
  *stride = 0;
  if (poses == nullptr) return NDT2D_OK;
  const size_t bytes = kc * n * 3 * sizeof(double);
  NDT2D_BATCH_HIP(owner, grow_device(&buffer->d, &buffer->cap, bytes));
  NDT2D_BATCH_HIP(owner, hipMemcpyAsync(buffer->d, poses + k0 * n * 3, bytes, hipMemcpyHostToDevice, stream));
  *out = static_cast<const double *>(buffer->d);
  *stride = 3 * n;
  return NDT2D_OK;
}

}  // namespace

// An object beside a graph (the dense covariance's, the direct solve's): it reads the graph's
// constraints, weighting and loss, and holds a workspace on the device within a budget of its own.
struct PgCompanion : BatchHost
{
  ndt2d_posegraph * graph = nullptr;   // (the caller keeps it alive)
  size_t workspace_bytes = 0;          // the budget
  void * d_workspace = nullptr;        // the chunk's jobs, from the first call on
  size_t workspace_cap = 0;
};

// The body of ndt2d_<noun>_create.
template <class T>
int pg_companion_create(ndt2d_posegraph * posegraph, size_t workspace_bytes, T ** out)
{
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (posegraph == nullptr || workspace_bytes == 0) return NDT2D_ERR_INVALID;
  T * s = new T();
  s->graph = posegraph;
  s->h = posegraph->h;
  s->device = posegraph->device;
  s->workspace_bytes = workspace_bytes;
  *out = s;
  return NDT2D_OK;
}

// In front of `delete` in ndt2d_<noun>_destroy: the stream waited out, then what BatchHost and this
// hold (what the object holds beyond them is its unit's).
inline void pg_companion_release(PgCompanion * s)
{
  batch_drain(s);
  batch_release(s);
  if (s->d_workspace != nullptr) (void)hipFree(s->d_workspace);
}

// The workspace at `need` bytes, what the call's largest chunk takes: exactly that where it grows,
// without grow_device's slack, so never more than the budget.
inline int pg_companion_workspace(PgCompanion * s, size_t need)
{
  if (need <= s->workspace_cap) return NDT2D_OK;
  if (s->d_workspace != nullptr) (void)hipFree(s->d_workspace);
  s->d_workspace = nullptr;
  s->workspace_cap = 0;
  NDT2D_BATCH_HIP(s, hipMalloc(&s->d_workspace, need));
  s->workspace_cap = need;
  return NDT2D_OK;
}

}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_STATE_H_
