// The kernels of the sparse covariance (sparsecov/ndt2d_sparsecov.hip; include/ndt2d_hip.h, "Sparse
// covariance"), all FP64, gfx950 / MI355X: blocks of (H_FF + damping clamp(diag H_FF))^-1 from the
// sparse solve's factorisation, without a dense 3n x 3n matrix.  The plan and the lists are
// sparsecov/ndt2d_sparsecov_plan.h, the per-node and per-pair arithmetic
// sparsecov/ndt2d_sparsecov_select.h.  What exists is launched from the unit, not copied here: the
// sparse solve's assemble, reduce and Schur kernels (sparse/ndt2d_sparse_kernel.h) on its layout, the
// dense covariance's fill, factor and inversion (covariance/ndt2d_covariance_kernel.h) on the layout
// SparsecovJob.
//
// A chunk in stream order (sparsecov/ndt2d_sparsecov.hip): begin, the fill of S and T, the band
// assemble, the reduction, the Schur terms, S = L L^T and T = L^-1, the blocks of S^-1, the selected
// inversion, the column passes, the diagonal, the pairs.  A job is blockIdx.z of the per-node, per-pair
// and per-block launches and blockIdx.x of begin, select and columns.
//
// Determinism.  No atomics.  A block of S^-1 is each lane's strided partial in ascending k, the wave
// by an xor butterfly, as the dense covariance's blocks; a level of the selected inversion and of a
// column pass writes each node by one thread, levels are separated by a barrier; a block of Sigma is
// one thread's, summed in sparsecov/ndt2d_sparsecov_select.h's fixed order.  Nothing a job computes
// reads another job's, and a pair's block reads of the other pairs only where its own blocks lie.
//
// Bounds.  Every loop is bounded by n, n_i, the number of pairs, passes or levels, or 3 s before it
// starts; the lists' indices are the plan's (below n, n_i, s or the number of blocks, or kNone, which
// is tested).
//
// LDS: begin 1,280 bytes (the block's reductions), the others none.  Registers and scratch:
// DESIGN.md 3.18.7.
// Included by the .hip translation units only.
#ifndef NDT2D_SPARSECOV_KERNEL_H_
#define NDT2D_SPARSECOV_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>

#include "covariance/ndt2d_covariance_kernel.h"
#include "covariance/ndt2d_covariance_plan.h"
#include "direct/ndt2d_direct_kernel.h"
#include "direct/ndt2d_direct_step.h"
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "sparse/ndt2d_sparse_kernel.h"
#include "sparse/ndt2d_sparse_plan.h"
#include "sparse/ndt2d_sparse_schur.h"
#include "sparsecov/ndt2d_sparsecov_plan.h"
#include "sparsecov/ndt2d_sparsecov_select.h"

namespace ndt2d
{

namespace
{

constexpr uint32_t kSparsecovThreads = 256;   // nodes (or pairs) a workgroup of the diagonal and pairs kernels
constexpr size_t kSparsecovRec = NDT2D_COVARIANCE_RECORD_DOUBLES;

// A job's dense part as the dense covariance's kernels take a layout, with the inverse: S, its
// diagonal (the sparse solve's SparseJob, which its assemble and Schur kernels write), and T in the
// region in front, the jobs in descending order.  n: the number of separators.
struct SparsecovJob
{
  static constexpr bool kInverse = true;
  double * A, * T, * diag;
  __device__ __forceinline__ SparsecovJob(double * workspace, size_t n, size_t job)
  {
    const size_t ld = cov::padded(3 * n);
    A = workspace + job * sparse::schur_doubles(n);
    diag = A + ld * ld;
    T = workspace - (job + 1) * ld * ld;
  }
};

// A chunk's workspace as the new kernels take it: the sparse solve's chunk and what the plan adds.
struct SparsecovChunk
{
  SparseChunk sparse;
  double * select;      // [job][select_doubles(n_i)]
  double * blocks;      // [job][9 n_blocks]
  double * columns;     // [job][9 n_pairs]
  uint32_t n_blocks, n_pairs, n_passes;
  const uint32_t * block_list, * pair_list, * pass_list;
  __device__ __forceinline__ double * select_of(size_t job, size_t ni) const { return select + job * sparsecov::select_doubles(ni); }
  __device__ __forceinline__ double * blocks_of(size_t job) const { return blocks + job * 9 * static_cast<size_t>(n_blocks); }
  __device__ __forceinline__ double * columns_of(size_t job) const { return columns + job * 9 * static_cast<size_t>(n_pairs); }
  // whether the job's factorisation holds: the reduction's flag, and with separators the dense factor's record
  __device__ __forceinline__ bool factored(size_t job, uint32_t s) const
  {
    return sparse.reduction[job] == 0.0 && (s == 0 || sparse.factor[job * kCovRec] == 0.0);
  }
};

//   sparsecov_begin_kernel   grid (job), 1,024 threads: x = the job's poses, g, the diagonal blocks,
//       the free flags and rho' there (the solver's linearisation), and the state the sparse solve's
//       kernels read: one iteration to take, lambda = the damping.
template <int kLoss>
__global__ void __launch_bounds__(kPgThreads) sparsecov_begin_kernel(const PgGraph G, const uint8_t * enabled, const double * poses, size_t pose_stride,
                                                                      double damping, const SparsecovChunk chunk)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  const size_t job = blockIdx.x, n = G.n;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  const PgWork w(chunk.sparse.lm.work_of(job), n);
  const double * xs = poses + job * pose_stride;
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
#pragma unroll
    for (int j = 0; j < 3; ++j) w.x[3 * at + j] = xs[3 * at + j];
  }
  pg_trig(w.x, w.cs, G.n);
  __syncthreads();
  const double gmax = pg_linearize<kPgJacobi, kLoss>(G, en, w, sc, parity);
  if (threadIdx.x == 0)
  {
    direct::State s{};
    s.status = direct::kMaxIterations;
    s.gradient = gmax;
    s.pivot_ratio = 1.0;
    s.lambda = damping;
    s.nu = 2.0;
    *chunk.sparse.state_of(job) = s;
  }
}

//   sparsecov_blocks_kernel   grid (block, 1, job), one wave: block (x, y), x <= y, of S^-1 = T^T T
//       into the job's table -- the sum over the rows k >= 3 y of T[k, x]^T T[k, y] (T is lower
//       triangular), lane l the rows first + l, first + l + 64, ... in ascending order, the wave an
//       xor butterfly: the dense covariance's block sum on the separators' T.  (x, x) is symmetric
//       bit for bit.
[[maybe_unused]] __global__ void __launch_bounds__(kWave) sparsecov_blocks_kernel(uint32_t s, const SparsecovChunk chunk)
{
  const size_t job = blockIdx.z;
  const SparsecovJob w(chunk.sparse.dense, s, job);
  const size_t d = 3 * static_cast<size_t>(s), ld = cov::padded(d);
  const uint32_t x = chunk.block_list[2 * blockIdx.x], y = chunk.block_list[2 * blockIdx.x + 1];
  const size_t first = cov::unknown(y, 0), cx = cov::unknown(x, 0), cy = first;
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (size_t k = first + threadIdx.x; k < d; k += kWave)
  {
    const double * row = w.T + k * ld;
    const double tx[3] = {row[cx], row[cx + 1], row[cx + 2]}, ty[3] = {row[cy], row[cy + 1], row[cy + 2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * i + j] += tx[i] * ty[j];
    }
  }
  double * out = chunk.blocks_of(job) + 9 * static_cast<size_t>(blockIdx.x);
#pragma unroll
  for (int j = 0; j < 9; ++j)
  {
    const double v = pg_wave_sum(acc[j]);
    if (threadIdx.x == 0) out[j] = v;
  }
}

//   sparsecov_select_kernel   grid (job), 1,024 threads: the selected inversion of the job's interior
//       system down the levels the reduction factored -- the root, then from the top stride to 1 the
//       q-th eliminated node of a level by thread q mod 1,024 (sparsecov::select_node), one barrier a
//       level.  A job whose reduction failed is left alone: its blocks are zero.
[[maybe_unused]] __global__ void __launch_bounds__(kPgThreads) sparsecov_select_kernel(const SparsecovChunk chunk, uint32_t interior)
{
  const size_t job = blockIdx.x, ni = interior;
  if (ni == 0 || pg_uniform(chunk.sparse.reduction[job]) != 0.0) return;
  const sparse::Interior in = chunk.sparse.interior_of(job, ni);
  double * sel = chunk.select_of(job, ni);
  if (pg_tid() == 0u) sparsecov::select_root(in.m, sel);
  __syncthreads();
  for (size_t stride = pg::chain::top_stride(ni); stride >= 1; stride >>= 1)
  {
    const size_t count = pg::chain::gone_count(ni, stride);
    for (size_t q = pg_tid(); q < count; q += kPgThreads) sparsecov::select_node(in.m, sel, ni, pg::chain::gone_node(stride, q), stride);
    __syncthreads();
  }
}

//   sparsecov_columns_kernel   grid (job), 1,024 threads: the column passes.  Pass p solves
//       A_ii G_.,b = E_b for its node b through the reduction's right-hand-side levels, root and back
//       levels with three columns (sparse::forward_columns<3>, root_columns<3>, back_columns<3>), in
//       the first 18 doubles of each node's b; then the pairs of the pass take their G_ab.  One
//       barrier a level.  A pass does not read what another left: every node is seeded anew.
[[maybe_unused]] __global__ void __launch_bounds__(kPgThreads) sparsecov_columns_kernel(const SparsecovChunk chunk, const sparse::Tables t)
{
  const size_t job = blockIdx.x, ni = t.ni;
  if (ni == 0 || pg_uniform(chunk.sparse.reduction[job]) != 0.0) return;
  const sparse::Interior in = chunk.sparse.interior_of(job, ni);
  double * solution = in.b + sparsecov::kPassSolution;
  double * columns = chunk.columns_of(job);
  for (uint32_t p = 0; p < chunk.n_passes; ++p)
  {
    const size_t column = chunk.pass_list[p];
    for (size_t ii = pg_tid(); ii < ni; ii += kPgThreads) sparsecov::pass_seed(in.b, ii, column);
    __syncthreads();
    for (size_t stride = 1; stride < ni; stride <<= 1)
    {
      const size_t count = pg::chain::stay_count(ni, stride);
      for (size_t q = pg_tid(); q < count; q += kPgThreads)
      {
        sparse::forward_columns<sparsecov::kPassColumns>(in.m, in.b, ni, pg::chain::stay_node(stride, q), stride);
      }
      __syncthreads();
    }
    if (pg_tid() == 0u) sparse::root_columns<sparsecov::kPassColumns>(in.m, in.b, solution);
    __syncthreads();
    for (size_t stride = pg::chain::top_stride(ni); stride >= 1; stride >>= 1)
    {
      const size_t count = pg::chain::gone_count(ni, stride);
      for (size_t q = pg_tid(); q < count; q += kPgThreads)
      {
        sparse::back_columns<sparsecov::kPassColumns>(in.m, in.b, solution, ni, pg::chain::gone_node(stride, q), stride);
      }
      __syncthreads();
    }
    for (uint32_t q = pg_tid(); q < chunk.n_pairs; q += kPgThreads)
    {
      const uint32_t * words = chunk.pair_list + sparsecov::kPairWords * static_cast<size_t>(q);
      if (words[6] == p) sparsecov::pass_gather(in.b, t.index(words[0]), columns + 9 * static_cast<size_t>(q));
    }
    __syncthreads();
  }
}

//   sparsecov_diagonal_kernel   grid (nodes / 256, 1, job): a thread per node, Sigma_kk
//       (sparsecov::diagonal_block) -- zero where the node is not free, and everywhere in a job whose
//       factorisation failed.  The first thread of a job writes its record {status, stage, S's pivot
//       ratio}.
[[maybe_unused]] __global__ void __launch_bounds__(kSparsecovThreads) sparsecov_diagonal_kernel(uint32_t n, const SparsecovChunk chunk, const sparse::Tables t,
                                                                                               double * diagonal_out, double * records_out)
{
  const size_t job = blockIdx.z;
  const uint32_t i = blockIdx.x * kSparsecovThreads + threadIdx.x;
  const bool ok = chunk.factored(job, t.s);
  if (i == 0)
  {
    const bool reduced = chunk.sparse.reduction[job] == 0.0;
    double * rec = records_out + job * kSparsecovRec;
    rec[0] = ok ? static_cast<double>(NDT2D_COVARIANCE_OK) : static_cast<double>(NDT2D_COVARIANCE_NOT_POSITIVE_DEFINITE);
    rec[1] = ok ? 0.0 : (reduced ? 2.0 : 1.0);
    rec[2] = t.s == 0 ? 1.0 : chunk.sparse.factor[job * kCovRec + 2];
  }
  if (i >= n) return;
  const PgWork w(chunk.sparse.lm.work_of(job), n);
  double B[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (ok && w.act[i] != 0.0)
  {
    sparsecov::diagonal_block(t, chunk.sparse.interior_of(job, t.ni), chunk.select_of(job, t.ni), chunk.blocks_of(job), i, B);
  }
  double * out = diagonal_out + (job * n + i) * 9;
#pragma unroll
  for (int j = 0; j < 9; ++j) out[j] = B[j];
}

//   sparsecov_pairs_kernel   grid (pairs / 256, 1, job): a thread per asked pair
//       (sparsecov::pair_block), behind the column passes; zero where either node is not free, and in
//       a job whose factorisation failed.
[[maybe_unused]] __global__ void __launch_bounds__(kSparsecovThreads) sparsecov_pairs_kernel(uint32_t n, const SparsecovChunk chunk, const sparse::Tables t,
                                                                                            double * pairs_out)
{
  const size_t job = blockIdx.z;
  const uint32_t q = blockIdx.x * kSparsecovThreads + threadIdx.x;
  if (q >= chunk.n_pairs) return;
  const uint32_t * words = chunk.pair_list + sparsecov::kPairWords * static_cast<size_t>(q);
  const PgWork w(chunk.sparse.lm.work_of(job), n);
  double B[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (chunk.factored(job, t.s) && w.act[words[0]] != 0.0 && w.act[words[1]] != 0.0)
  {
    sparsecov::pair_block(t, chunk.sparse.interior_of(job, t.ni), chunk.select_of(job, t.ni), chunk.blocks_of(job), words,
                          chunk.columns_of(job) + 9 * static_cast<size_t>(q), B);
  }
  double * out = pairs_out + (job * chunk.n_pairs + q) * 9;
#pragma unroll
  for (int j = 0; j < 9; ++j) out[j] = B[j];
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_SPARSECOV_KERNEL_H_
