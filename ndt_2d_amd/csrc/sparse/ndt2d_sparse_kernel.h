// The kernels of the sparse pose-graph solve (sparse/ndt2d_sparse.hip; include/ndt2d_hip.h, "Sparse
// solve"), all FP64, gfx950 / MI355X: the direct solve's Levenberg-Marquardt with its linear step
// (H_FF + lambda clamp(diag)) delta = -g taken by a Schur complement on the separators -- the nodes
// closures touch -- over a block cyclic reduction of all interior nodes.  The plan and the tables are
// sparse/ndt2d_sparse_plan.h, the per-node arithmetic sparse/ndt2d_sparse_schur.h and
// posegraph/ndt2d_posegraph_chain.h; the cost, the linearisation, the decisions, the begin, step,
// finish and substitution kernels are the direct solve's (direct/ndt2d_direct_kernel.h), the factor
// of the separators' matrix the dense covariance's (covariance/ndt2d_covariance_kernel.h) on the
// layout SparseJob.
//
// One LM iteration of a chunk is a fixed list of launches (sparse/ndt2d_sparse.hip, sparse_iteration):
// the fill of S, the band assemble, the reduction, the Schur terms, S's factor, the substitution, the
// expansion, the step.  A job is blockIdx.z of the per-node launches and blockIdx.x of the reduction.
// A job that is not iterating is left alone by the reduction, the substitution and the step: what
// the other launches compute for it is not read.
//
// Determinism.  No atomics.  Every block of the band, of S and of the right-hand sides has one
// writer, which sums a node's constraints in ascending constraint index; a level of the reduction
// writes each node by one thread, levels are separated by a barrier; the Schur terms of a block row
// are its separator's thread's, summed in a fixed order.
//
// Bounds.  Every loop is bounded by n, n_i, s, a node's degree or the number of levels before it
// starts; the tables' indices are the plan's (below n_i or s, or kNone, which is tested).
//
// LDS: the reduction 1,280 bytes (the block's reduction of its flag).  Registers and scratch:
// DESIGN.md 3.18.6.
// Included by the .hip translation units only.
#ifndef NDT2D_SPARSE_KERNEL_H_
#define NDT2D_SPARSE_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>

#include "covariance/ndt2d_covariance_kernel.h"
#include "covariance/ndt2d_covariance_plan.h"
#include "direct/ndt2d_direct_kernel.h"
#include "direct/ndt2d_direct_step.h"
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "sparse/ndt2d_sparse_plan.h"
#include "sparse/ndt2d_sparse_schur.h"

namespace ndt2d
{

namespace
{

static_assert(sparse::kNodeDoubles == kPgNodeDoubles, "the plan's PgWork");
static_assert(sparse::kStateDoubles == kDirectLm + kCovRec + 1, "the plan's state");
static_assert(sparse::kMaxNodes == kPgMaxNodes, "the solver's limit");
constexpr uint32_t kSparseNodeThreads = 64;     // nodes (or separators) a workgroup of the per-node kernels
constexpr uint32_t kSparseExpandThreads = 256;

// A job's dense part, as the covariance's kernels and the substitution take a layout: S, its diagonal,
// the substitution's vector.  n: the number of separators.
struct SparseJob
{
  static constexpr bool kInverse = false;
  double * A, * diag, * rhs;
  __device__ __forceinline__ SparseJob(double * workspace, size_t n, size_t job)
  {
    const size_t ld = cov::padded(3 * n);
    A = workspace + job * sparse::schur_doubles(n);
    diag = A + ld * ld;
    rhs = diag + ld;
  }
};

// Where the substitution on S takes its right-hand side from (it negates g) and leaves delta_s.
struct SparseVectors
{
  double * g, * d;
};

// A chunk's workspace as the kernels take it.
struct SparseChunk
{
  double * dense;       // [job][schur_doubles(s)]
  double * interior;    // [job][interior_doubles(n_i)]
  double * vectors;     // [job][6 s]: g_s + A_si y, then delta_s
  double * reduction;   // [job] non-zero: a pivot of the reduction was not positive
  DirectChunk lm;       // work, state and the factor's records, as the direct solve's kernels take them
  using Job = SparseJob;
  __device__ __forceinline__ direct::State * state_of(size_t job) const { return lm.state_of(job); }
  __device__ __forceinline__ SparseVectors vectors_of(size_t job, size_t s) const
  {
    double * at = vectors + job * sparse::vector_doubles(s);
    return SparseVectors{at, at + 3 * s};
  }
  __device__ __forceinline__ sparse::Interior interior_of(size_t job, size_t ni) const
  {
    return sparse::interior_at(interior + job * sparse::interior_doubles(ni), ni);
  }
  // (the substitution reads the factor's records as chunk.factor)
  double * factor;
};

// (W E_i)^T (W E_o) of constraint c as node i's side sees it, weighted by rho' under a loss.
template <int kLoss>
__device__ __forceinline__ void sparse_coupling(const PgGraph & G, const PgWork & w, uint32_t entry, uint32_t c, uint32_t a, uint32_t b, double * X)
{
  const pg::Frame f = pg_frame(w, a, b);
  const double * W = G.W + 9 * static_cast<size_t>(c);
  double Ei[9], Eo[9], Ji[9], Jo[9];
  if (entry & 1u)
  {
    pg::jacobian_b(f, Ei);
    pg::jacobian_a(f, Eo);
  }
  else
  {
    pg::jacobian_a(f, Ei);
    pg::jacobian_b(f, Eo);
  }
  pg::chain::mm(W, Ei, Ji);
  pg::chain::mm(W, Eo, Jo);
  pg::chain::mtm(Ji, Jo, X);
  if constexpr (kLoss != 0)
  {
    const double rw = pg_weights(G, w)[c];
#pragma unroll
    for (int j = 0; j < 9; ++j) X[j] = rw * X[j];
  }
}

//   sparse_assemble_kernel   grid (nodes / 64, 1, job): a thread per node, behind the linearisation
//       (g, the diagonal blocks, the free flags and rho' in the job's PgWork) and the fill of S.  The
//       node's diagonal block + lambda clamp(diag) (the identity where the node is not free) goes to
//       the reduction's D or to S; its couplings, gathered over its incident enabled constraints in
//       ascending constraint index and zero where either node is not free: an interior node's to
//       node + 1 to U (an interior node) or Cr (a separator), to a separator at node - 1 to Cl, then
//       its seven right-hand sides; a separator's to every separator before it, chain edge or
//       closure, into its block row of S.
template <int kLoss>
__global__ void __launch_bounds__(kSparseNodeThreads) sparse_assemble_kernel(const PgGraph G, const uint8_t * enabled, const SparseChunk chunk,
                                                                             const sparse::Tables t)
{
  const size_t job = blockIdx.z, n = G.n;
  const uint32_t i = blockIdx.x * kSparseNodeThreads + threadIdx.x;
  if (i >= G.n) return;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  const PgWork w(chunk.lm.work_of(job), n);
  const double lambda = chunk.state_of(job)->lambda;
  const size_t at = static_cast<size_t>(i);
  const bool active = w.act[at] != 0.0;
  double S[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
  if (active)
  {
#pragma unroll
    for (int j = 0; j < 6; ++j) S[j] = w.hd[6 * at + j];
    S[0] += lambda * pg_clamp_diag(S[0]);
    S[3] += lambda * pg_clamp_diag(S[3]);
    S[5] += lambda * pg_clamp_diag(S[5]);
  }
  const uint32_t k0 = G.node_ptr[i], k1 = G.node_ptr[i + 1];
  if (t.separator(i))
  {
    const SparseJob dense(chunk.dense, t.s, job);
    const size_t ld = cov::padded(3 * static_cast<size_t>(t.s)), row = 3 * static_cast<size_t>(t.index(i));
    if (active)
    {
      for (uint32_t k = k0; k < k1; ++k)
      {
        const uint32_t entry = G.node_con[k], c = entry >> 1;
        if (en != nullptr && en[c] == 0) continue;
        const uint32_t a = G.begin[c], b = G.end[c], other = (entry & 1u) ? a : b;
        if (other >= i || !t.separator(other) || w.act[other] == 0.0) continue;
        double X[9];
        sparse_coupling<kLoss>(G, w, entry, c, a, b, X);
        double * block = dense.A + row * ld + 3 * static_cast<size_t>(t.index(other));
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
#pragma unroll
          for (int q = 0; q < 3; ++q) block[r * ld + q] += X[3 * r + q];
        }
      }
    }
    double * block = dense.A + row * ld + row;
    block[0] = S[0];
    block[1] = S[1];
    block[2] = S[2];
    block[ld] = S[1];
    block[ld + 1] = S[3];
    block[ld + 2] = S[4];
    block[2 * ld] = S[2];
    block[2 * ld + 1] = S[4];
    block[2 * ld + 2] = S[5];
    return;
  }
  const sparse::Interior in = chunk.interior_of(job, t.ni);
  const size_t ii = t.index(i);
  double next[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, prev[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const bool to_next = active && i + 1u < G.n && w.act[at + 1] != 0.0;
  const bool to_prev = active && i > 0u && t.separator(i - 1u) && w.act[at - 1] != 0.0;
  if (to_next || to_prev)
  {
    for (uint32_t k = k0; k < k1; ++k)
    {
      const uint32_t entry = G.node_con[k], c = entry >> 1;
      if (en != nullptr && en[c] == 0) continue;
      const uint32_t a = G.begin[c], b = G.end[c], other = (entry & 1u) ? a : b;
      const bool up = to_next && other == i + 1u, down = to_prev && other + 1u == i;
      if (!up && !down) continue;
      double X[9];
      sparse_coupling<kLoss>(G, w, entry, c, a, b, X);
#pragma unroll
      for (int j = 0; j < 9; ++j)
      {
        if (up) next[j] += X[j];
        else prev[j] += X[j];
      }
    }
  }
  const bool next_separator = i + 1u < G.n && t.separator(i + 1u);
#pragma unroll
  for (int j = 0; j < 6; ++j) in.m.D[6 * ii + j] = S[j];
#pragma unroll
  for (int j = 0; j < 9; ++j)
  {
    in.m.U[9 * ii + j] = next_separator ? 0.0 : next[j];
    in.Cr[9 * ii + j] = next_separator ? next[j] : 0.0;
    in.Cl[9 * ii + j] = prev[j];
  }
  sparse::set_columns(in, ii, w.g + 3 * at);
}

//   sparse_reduce_kernel   grid (job), 1,024 threads: the block cyclic reduction of the job's interior
//       system -- chain's factor levels, then the K columns (7, or 1 without a separator: -g alone)
//       through the right-hand-side levels, the root and the back-substitution levels, one barrier a
//       level.  The q-th staying (or eliminated) node of a level goes to thread q mod 1,024.  The
//       job's flag: whether a pivot was not positive.
template <int K>
__global__ void __launch_bounds__(kPgThreads) sparse_reduce_kernel(const SparseChunk chunk, uint32_t interior, const PgRules rules)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  const size_t job = blockIdx.x, ni = interior;
  const direct::State s = direct_load_state(chunk.state_of(job));
  if (!direct::iterating(s, direct_rules(rules))) return;
  const sparse::Interior in = chunk.interior_of(job, ni);
  double bad = 0.0;
  for (size_t stride = 1; stride < ni; stride <<= 1)
  {
    const size_t count = pg::chain::stay_count(ni, stride);
    for (size_t q = pg_tid(); q < count; q += kPgThreads)
    {
      if (!pg::chain::factor_node(in.m, ni, pg::chain::stay_node(stride, q), stride)) bad = 1.0;
    }
    __syncthreads();
  }
  if (ni != 0 && pg_tid() == 0u && !pg::chain::factor_root(in.m)) bad = 1.0;
  bad = pg_block_max(bad, sc, parity);   // (its barrier also orders the root's pivot)
  if (threadIdx.x == 0) chunk.reduction[job] = bad;
  for (size_t stride = 1; stride < ni; stride <<= 1)
  {
    const size_t count = pg::chain::stay_count(ni, stride);
    for (size_t q = pg_tid(); q < count; q += kPgThreads) sparse::forward_columns<K>(in.m, in.b, ni, pg::chain::stay_node(stride, q), stride);
    __syncthreads();
  }
  if (ni != 0 && pg_tid() == 0u) sparse::root_columns<K>(in.m, in.b, in.x);
  __syncthreads();
  for (size_t stride = pg::chain::top_stride(ni); stride >= 1; stride >>= 1)
  {
    const size_t count = pg::chain::gone_count(ni, stride);
    for (size_t q = pg_tid(); q < count; q += kPgThreads) sparse::back_columns<K>(in.m, in.b, in.x, ni, pg::chain::gone_node(stride, q), stride);
    __syncthreads();
  }
}

//   sparse_schur_kernel   grid (separators / 64, 1, job): a thread per separator, its block row of
//       S -= A_si Z, S's diagonal, and g_s + A_si y (sparse::schur_separator).
[[maybe_unused]] __global__ void __launch_bounds__(kSparseNodeThreads) sparse_schur_kernel(uint32_t n, const SparseChunk chunk, const sparse::Tables t)
{
  const size_t job = blockIdx.z;
  const uint32_t si = blockIdx.x * kSparseNodeThreads + threadIdx.x;
  if (si >= t.s) return;
  const PgWork w(chunk.lm.work_of(job), n);
  const SparseJob dense(chunk.dense, t.s, job);
  sparse::schur_separator(t, chunk.interior_of(job, t.ni), w.g, si, dense.A, cov::padded(3 * static_cast<size_t>(t.s)), dense.diag,
                          chunk.vectors_of(job, t.s).g);
}

//   sparse_expand_kernel   grid (nodes / 256, 1, job): a thread per node, delta into the job's PgWork
//       (sparse::expand_node).  The first thread of a job settles the record the step kernel reads:
//       a failed reduction fails the factorisation, and without a separator -- no dense launch -- the
//       record is the reduction's alone, with a pivot ratio of 1.
[[maybe_unused]] __global__ void __launch_bounds__(kSparseExpandThreads) sparse_expand_kernel(uint32_t n, const SparseChunk chunk, const sparse::Tables t)
{
  const size_t job = blockIdx.z;
  const uint32_t i = blockIdx.x * kSparseExpandThreads + threadIdx.x;
  if (i == 0)
  {
    double * rec = chunk.factor + job * kCovRec;
    const double bad = chunk.reduction[job];
    if (t.s == 0)
    {
      rec[0] = bad;
      rec[1] = -1.0;
      rec[2] = 1.0;
    }
    else if (bad != 0.0)
    {
      rec[0] = 1.0;
    }
  }
  if (i >= n) return;
  const PgWork w(chunk.lm.work_of(job), n);
  sparse::expand_node(t, chunk.interior_of(job, t.ni), chunk.vectors_of(job, t.s).d, i, w.d);
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_SPARSE_KERNEL_H_
