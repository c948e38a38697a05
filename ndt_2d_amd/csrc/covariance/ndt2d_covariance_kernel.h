// The kernels of the dense covariance (covariance/ndt2d_covariance.hip; include/ndt2d_hip.h, "Dense
// covariance"), all FP64, gfx950 / MI355X: a job's A = H_FF + damping clamp(diag H_FF) assembled
// densely, A = L L^T by a blocked right-looking Cholesky without pivoting, T = L^-1 by the same
// panels, and the asked 3 x 3 blocks of Sigma = T^T T.  The plan -- panels, tiles, launches -- is
// covariance/ndt2d_covariance_plan.h; the arithmetic of a constraint is the solver's
// (posegraph/ndt2d_posegraph_fn.h, ..._loss.h, ..._kernel.h).
//
// A job is blockIdx.z of every launch.  Its matrices are row-major [ld][ld], ld = padded(3 n); a node
// that is not free (the fixed one, or without an enabled constraint) and the padding keep the rows
// and columns of the identity, so the dimension is the same for every mask.
//
// Determinism.  No floating-point operation's order depends on another job, on the chunk or on the
// run: a block of A has one writer, which sums the node's constraints in ascending constraint index;
// every element of a panel, of a substitution and of a tile of an update is summed over k in
// ascending order by one thread or one wave; a block of Sigma is each lane's strided partial in
// ascending k, the wave by an xor butterfly.  No split-K.
//
// Bounds.  Every loop is bounded by ld, kPanel or a node's degree before it starts.  A job whose
// pivot failed runs through the same launches with the values it has (NaN, mostly); only the
// factor kernel's one owner thread notes it, and the blocks kernel writes zeros for it.
//
// LDS: factor 18,816 bytes, the substitutions 18,816, the updates 37,632.  Registers and scratch:
// DESIGN.md 3.18.4.
// Included by the .hip translation units only.
#ifndef NDT2D_COVARIANCE_KERNEL_H_
#define NDT2D_COVARIANCE_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>

#include "covariance/ndt2d_covariance_plan.h"
#include "posegraph/ndt2d_posegraph_fn.h"
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "posegraph/ndt2d_posegraph_loss.h"

namespace ndt2d
{

namespace
{

namespace cov = covariance;

constexpr uint32_t kCovNodeThreads = 64;     // nodes a workgroup of the node and assemble kernels
constexpr uint32_t kCovFillThreads = 256;
constexpr uint32_t kCovFactorLanes = 16;     // threads a row of the diagonal block's factorisation
constexpr uint32_t kCovFactorThreads = cov::kPanel * kCovFactorLanes;
constexpr uint32_t kCovUpdateThreads = 192;  // three waves, a row of three tiles each
constexpr uint32_t kCovLds = cov::kPanel + 1;   // the row stride of a 48 x 48 block in LDS
constexpr size_t kCovRec = NDT2D_COVARIANCE_RECORD_DOUBLES;

typedef double cov_d4 __attribute__((ext_vector_type(4)));

// A job's part of the workspace.  The kernels that walk a job's matrices take the layout as a template
// argument, CovJob by default: the direct solve (direct/ndt2d_direct_kernel.h) runs the assembly and
// the factorisation on a layout of its own, without T (kInverse = false).
struct CovJob
{
  static constexpr bool kInverse = true;
  double * A, * T, * diag, * cs, * act;
  __device__ __forceinline__ CovJob(double * workspace, size_t n, size_t job)
  {
    const size_t ld = cov::padded(3 * n);
    A = workspace + job * cov::job_doubles(n);
    T = A + ld * ld;
    diag = T + ld * ld;
    cs = diag + ld;
    act = cs + 2 * n;
  }
};

//   covariance_nodes_kernel   grid (nodes / 64, 1, job): cos and sin of each pose's heading (the
//       device library's, as the solver's node cache) and whether the node is free.
template <class Job = CovJob>
__global__ void __launch_bounds__(kCovNodeThreads) covariance_nodes_kernel(const PgGraph G, const uint8_t * enabled, const double * poses,
                                                                           size_t pose_stride, double * workspace)
{
  const size_t job = blockIdx.z, n = G.n;
  const uint32_t i = blockIdx.x * kCovNodeThreads + threadIdx.x;
  if (i >= G.n) return;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  const Job w(workspace, n, job);
  const double * xs = poses + job * pose_stride;
  double sn, cs;
  sincos(xs[3 * static_cast<size_t>(i) + 2], &sn, &cs);
  w.cs[2 * static_cast<size_t>(i)] = cs;
  w.cs[2 * static_cast<size_t>(i) + 1] = sn;
  uint32_t count = 0;
  const uint32_t k1 = G.node_ptr[i + 1];
  for (uint32_t k = G.node_ptr[i]; k < k1; ++k)
  {
    const uint32_t c = G.node_con[k] >> 1;
    if (en == nullptr || en[c] != 0) ++count;
  }
  w.act[i] = count != 0u && i != G.fixed ? 1.0 : 0.0;
}

//   covariance_fill_kernel   grid (ld / 256, row, job): A = 0 but the padding's unit diagonal,
//       T = the identity (where the layout has one).
template <class Job = CovJob>
__global__ void __launch_bounds__(kCovFillThreads) covariance_fill_kernel(uint32_t n, double * workspace)
{
  const Job w(workspace, n, blockIdx.z);
  const size_t d = 3 * static_cast<size_t>(n), ld = cov::padded(d);
  const size_t r = blockIdx.y, c = static_cast<size_t>(blockIdx.x) * kCovFillThreads + threadIdx.x;
  if (c >= ld) return;
  w.A[r * ld + c] = r == c && r >= d ? 1.0 : 0.0;
  if constexpr (Job::kInverse) w.T[r * ld + c] = r == c ? 1.0 : 0.0;
  if (r == 0 && c >= d) w.diag[c] = 1.0;
}

//   covariance_assemble_kernel   grid (nodes / 64, 1, job): a thread per node sums its block row of
//       the lower triangle over its incident constraints in ascending constraint index -- the
//       diagonal block as pg_linearize does (the same bits), block (i, j) for the free j < i as
//       (W E_i)^T (W E_j), under a loss each weighted by the constraint's rho' taken from the node's
//       own r -- duplicates and reversed edges included.  The diagonal block gets
//       + damping clamp(diag); job_damping: NULL, or the jobs' own dampings at
//       job_damping[job x damping_stride] in place of `damping` (the direct solve's lambda).  A block
//       has one writer: this thread.  Behind the node and fill kernels.
template <int kLoss, class Job = CovJob>
__global__ void __launch_bounds__(kCovNodeThreads) covariance_assemble_kernel(const PgGraph G, const uint8_t * enabled, const double * poses,
                                                                              size_t pose_stride, double damping, const double * job_damping,
                                                                              size_t damping_stride, double * workspace)
{
  const size_t job = blockIdx.z, n = G.n, ld = cov::padded(3 * n);
  if (job_damping != nullptr) damping = job_damping[job * damping_stride];
  const uint32_t i = blockIdx.x * kCovNodeThreads + threadIdx.x;
  if (i >= G.n) return;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  const Job w(workspace, n, job);
  const double * xs = poses + job * pose_stride;
  const size_t at = cov::unknown(i, 0);
  double S[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
  if (w.act[i] != 0.0)
  {
#pragma unroll
    for (int j = 0; j < 6; ++j) S[j] = 0.0;
    const uint32_t k1 = G.node_ptr[i + 1];
    for (uint32_t k = G.node_ptr[i]; k < k1; ++k)
    {
      const uint32_t entry = G.node_con[k], c = entry >> 1;
      if (en != nullptr && en[c] == 0) continue;
      const uint32_t a = G.begin[c], b = G.end[c];
      const pg::Frame f = pg::frame(w.cs[2 * static_cast<size_t>(a)], w.cs[2 * static_cast<size_t>(a) + 1], xs + 3 * static_cast<size_t>(a),
                                    xs + 3 * static_cast<size_t>(b));
      const double * W = G.W + 9 * static_cast<size_t>(c);
      [[maybe_unused]] double rw = 1.0;
      if constexpr (kLoss != 0)
      {
        double e[3], r[3];
        pg::error(f, xs[3 * static_cast<size_t>(a) + 2], xs[3 * static_cast<size_t>(b) + 2], G.transform + 3 * static_cast<size_t>(c), e);
        pg::mul(W, e, r);
        rw = PgLoss<kLoss>(G).weight(c, (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
      }
      double Ei[9], Eo[9];
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
      if constexpr (kLoss == 0)
      {
        pg::add_jtj(W, Ei, S);
      }
      else
      {
        double Q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        pg::add_jtj(W, Ei, Q);
#pragma unroll
        for (int j = 0; j < 6; ++j) S[j] += rw * Q[j];
      }
      const uint32_t other = (entry & 1u) ? a : b;
      if (other < i && w.act[other] != 0.0)
      {
        double Ji[9], Jo[9], X[9];
        pg::chain::mm(W, Ei, Ji);
        pg::chain::mm(W, Eo, Jo);
        pg::chain::mtm(Ji, Jo, X);
        double * block = w.A + at * ld + cov::unknown(other, 0);
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
#pragma unroll
          for (int q = 0; q < 3; ++q)
          {
            if constexpr (kLoss == 0) block[r * ld + q] += X[3 * r + q];
            else block[r * ld + q] += rw * X[3 * r + q];
          }
        }
      }
    }
    S[0] += damping * pg_clamp_diag(S[0]);
    S[3] += damping * pg_clamp_diag(S[3]);
    S[5] += damping * pg_clamp_diag(S[5]);
  }
  double * block = w.A + at * ld + at;
  block[0] = S[0];
  block[1] = S[1];
  block[2] = S[2];
  block[ld] = S[1];
  block[ld + 1] = S[3];
  block[ld + 2] = S[4];
  block[2 * ld] = S[2];
  block[2 * ld + 1] = S[4];
  block[2 * ld + 2] = S[5];
  w.diag[at] = S[0];
  w.diag[at + 1] = S[3];
  w.diag[at + 2] = S[5];
}

// The 48 x 48 block of M at (row0, col0) into LDS, by `threads` threads; kTranspose: block[c][r].
template <bool kTranspose>
__device__ __forceinline__ void cov_load_block(const double * M, size_t ld, size_t row0, size_t col0, double (*block)[kCovLds], uint32_t threads)
{
  for (uint32_t e = threadIdx.x; e < cov::kPanel * cov::kPanel; e += threads)
  {
    const uint32_t r = e / cov::kPanel, c = e % cov::kPanel;
    const double v = M[(row0 + r) * ld + col0 + c];
    if constexpr (kTranspose) block[c][r] = v;
    else block[r][c] = v;
  }
}

//   covariance_factor_kernel   grid (1, 1, job), 768 threads: the diagonal block of panel p factored
//       in LDS, unblocked and right-looking; row t of the block has 16 threads, which share the
//       columns of its update (c = j + 1 + lane, + 16, ...).  An element meets the same operations in
//       the same order whatever the number of lanes.  Thread 0 owns the job's record {failed, the
//       first failing unknown or -1, the smallest pivot / diagonal of A} with plain stores: panel 0
//       starts it, every panel reads it back.  A pivot <= 0 or not finite fails.
template <class Job = CovJob>
__global__ void __launch_bounds__(kCovFactorThreads) covariance_factor_kernel(uint32_t n, uint32_t p, double * workspace, double * records)
{
  __shared__ double S[cov::kPanel][kCovLds];
  const Job w(workspace, n, blockIdx.z);
  const size_t d = 3 * static_cast<size_t>(n), ld = cov::padded(d), j0 = static_cast<size_t>(p) * cov::kPanel;
  const uint32_t t = threadIdx.x / kCovFactorLanes, lane = threadIdx.x % kCovFactorLanes;
  cov_load_block<false>(w.A, ld, j0, j0, S, kCovFactorThreads);
  double * rec = records + blockIdx.z * kCovRec;
  double failed = 0.0, first = -1.0, ratio = 1.0;
  if (threadIdx.x == 0 && p != 0)
  {
    failed = rec[0];
    first = rec[1];
    ratio = rec[2];
  }
  __syncthreads();
  for (uint32_t j = 0; j < cov::kPanel; ++j)
  {
    const double pivot = S[j][j];
    const double root = sqrt(pivot);
    __syncthreads();
    if (threadIdx.x == 0 && j0 + j < d)
    {
      // (the ratio: up to and with the first failing pivot, fmin passing a NaN by)
      if (failed == 0.0) ratio = fmin(ratio, pivot / w.diag[j0 + j]);
      if (!(pivot > 0.0) || !(pivot <= 1.7976931348623157e308))
      {
        if (failed == 0.0) first = static_cast<double>(j0 + j);
        failed = 1.0;
      }
    }
    if (lane == 0 && t == j) S[j][j] = root;
    if (lane == 0 && t > j) S[t][j] = S[t][j] / root;
    __syncthreads();
    if (t > j)
    {
      const double lt = S[t][j];
      for (uint32_t c = j + 1 + lane; c <= t; c += kCovFactorLanes) S[t][c] -= lt * S[c][j];
    }
    __syncthreads();
  }
  for (uint32_t e = threadIdx.x; e < cov::kPanel * cov::kPanel; e += kCovFactorThreads)
  {
    const uint32_t r = e / cov::kPanel, c = e % cov::kPanel;
    if (c <= r) w.A[(j0 + r) * ld + j0 + c] = S[r][c];
  }
  if (threadIdx.x == 0)
  {
    rec[0] = failed;
    rec[1] = first;
    rec[2] = ratio;
  }
}

//   covariance_solve_kernel   grid (64 rows or columns a workgroup, 1, job), one wave, L[p, p] in LDS.
//       kRow = false: a thread per row i below the panel, L[i, p] = A[i, p] L[p, p]^-T by
//       substitution along the row.  kRow = true: a thread per column c < 48 (p + 1),
//       T[p, c] = L[p, p]^-1 T[p, c] by substitution down the column.  The 48 values stay in registers.
template <bool kRow, class Job = CovJob>
__global__ void __launch_bounds__(kWave) covariance_solve_kernel(uint32_t n, uint32_t p, double * workspace)
{
  __shared__ double L[cov::kPanel][kCovLds];
  const Job w(workspace, n, blockIdx.z);
  const size_t ld = cov::padded(3 * static_cast<size_t>(n)), j0 = static_cast<size_t>(p) * cov::kPanel;
  cov_load_block<false>(w.A, ld, j0, j0, L, kWave);
  __syncthreads();
  const size_t lane = static_cast<size_t>(blockIdx.x) * cov::kRows + threadIdx.x;
  // the thread's 48 values: M[at + k stride]
  double * M;
  size_t stride;
  if constexpr (kRow)
  {
    if (lane >= j0 + cov::kPanel) return;
    M = w.T + j0 * ld + lane;
    stride = ld;
  }
  else
  {
    const size_t row = j0 + cov::kPanel + lane;
    if (row >= ld) return;
    M = w.A + row * ld + j0;
    stride = 1;
  }
  double x[cov::kPanel];
#pragma unroll
  for (uint32_t c = 0; c < cov::kPanel; ++c) x[c] = M[c * stride];
#pragma unroll
  for (uint32_t c = 0; c < cov::kPanel; ++c)
  {
    double v = x[c];
#pragma unroll
    for (uint32_t k = 0; k < c; ++k) v -= x[k] * L[c][k];
    x[c] = v / L[c][c];
  }
#pragma unroll
  for (uint32_t c = 0; c < cov::kPanel; ++c) M[c * stride] = x[c];
}

//   covariance_update_kernel   grid (block, 1, job), three waves: C -= P Q^T of one 48 x 48 block on
//       the matrix cores, v_mfma_f64_16x16x4_f64.  kRect = false: C = A[bi, bj] over the lower
//       blocks behind panel p, P = L[bi, p], Q = L[bj, p].  kRect = true: C = T[bi, bq], P = L[bi, p],
//       Q^T = T[p, bq].  P and Q lie in LDS as [row][k]; lane l gives the instruction
//       A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15], one double each, and holds
//       D[row (l >> 4) + 4 reg][col l & 15] in reg = 0 .. 3.  Wave v has the block's tile row v:
//       three accumulators, each summed over the panel's 48 k in ascending order from zero, then
//       subtracted from C once.
template <bool kRect, class Job = CovJob>
__global__ void __launch_bounds__(kCovUpdateThreads) covariance_update_kernel(uint32_t n, uint32_t p, double * workspace)
{
  __shared__ double P[cov::kPanel][kCovLds];
  __shared__ double Q[cov::kPanel][kCovLds];
  const Job w(workspace, n, blockIdx.z);
  const size_t ld = cov::padded(3 * static_cast<size_t>(n)), j0 = static_cast<size_t>(p) * cov::kPanel;
  uint32_t bi, bj;
  cov::update_block(kRect ? cov::kUpdateRect : cov::kUpdate, p, blockIdx.x, &bi, &bj);
  const size_t row0 = static_cast<size_t>(bi) * cov::kPanel, col0 = static_cast<size_t>(bj) * cov::kPanel;
  cov_load_block<false>(w.A, ld, row0, j0, P, kCovUpdateThreads);
  if constexpr (kRect) cov_load_block<true>(w.T, ld, j0, col0, Q, kCovUpdateThreads);
  else cov_load_block<false>(w.A, ld, col0, j0, Q, kCovUpdateThreads);
  __syncthreads();
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const uint32_t lo = lane & 15u, hi = lane >> 4;
  cov_d4 acc[3];
#pragma unroll
  for (int tj = 0; tj < 3; ++tj) acc[tj] = cov_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (uint32_t k0 = 0; k0 < cov::kPanel; k0 += 4)
  {
    const double a = P[cov::kTile * wave + lo][k0 + hi];
#pragma unroll
    for (int tj = 0; tj < 3; ++tj)
    {
      const double b = Q[cov::kTile * tj + lo][k0 + hi];
      acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[tj], 0, 0, 0);
    }
  }
  double * C;
  if constexpr (kRect) C = w.T + (row0 + cov::kTile * wave) * ld + col0;
  else C = w.A + (row0 + cov::kTile * wave) * ld + col0;
#pragma unroll
  for (int tj = 0; tj < 3; ++tj)
  {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
    {
      double * at = C + (hi + 4u * reg) * ld + cov::kTile * tj + lo;
      *at = *at - acc[tj][reg];
    }
  }
}

//   covariance_blocks_kernel   grid (n + pairs, 1, job), one wave: block (a, b) of Sigma = T^T T,
//       sum over the rows k >= 3 max(a, b) of T[k, a]^T T[k, b] (T is lower triangular) -- (a, a)
//       for workgroup a < n, the asked pair behind.  Lane l takes the rows first + l, first + l + 64,
//       ... in ascending order, the wave an xor butterfly.  (a, b) and (b, a) run the same products
//       in the same order: transposes bit for bit, and (a, a) is symmetric.  Zero where a or b is
//       not free, and everywhere in a job that failed.  ([[maybe_unused]]: the one kernel here that is
//       not a template, in a header that the direct solve's unit takes for the factor alone.)
[[maybe_unused]] __global__ void __launch_bounds__(kWave) covariance_blocks_kernel(uint32_t n, const uint32_t * pairs, double * workspace, const double * records,
                                                                  double * diagonal_out, double * pairs_out)
{
  const size_t job = blockIdx.z;
  const CovJob w(workspace, n, job);
  const size_t d = 3 * static_cast<size_t>(n), ld = cov::padded(d);
  const uint32_t n_pairs = gridDim.x - n;
  uint32_t a, b;
  double * out;
  if (blockIdx.x < n)
  {
    a = b = blockIdx.x;
    out = diagonal_out + (job * n + blockIdx.x) * 9;
  }
  else
  {
    const uint32_t q = blockIdx.x - n;
    a = pairs[2 * q];
    b = pairs[2 * q + 1];
    out = pairs_out + (job * n_pairs + q) * 9;
  }
  const size_t first = cov::unknown(a > b ? a : b, 0), ca = cov::unknown(a, 0), cb = cov::unknown(b, 0);
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (size_t k = first + threadIdx.x; k < d; k += kWave)
  {
    const double * row = w.T + k * ld;
    const double ta[3] = {row[ca], row[ca + 1], row[ca + 2]}, tb[3] = {row[cb], row[cb + 1], row[cb + 2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * i + j] += ta[i] * tb[j];
    }
  }
  const bool keep = records[job * kCovRec] == 0.0 && w.act[a] != 0.0 && w.act[b] != 0.0;
#pragma unroll
  for (int j = 0; j < 9; ++j)
  {
    const double v = pg_wave_sum(acc[j]);
    if (threadIdx.x == 0) out[j] = keep ? v : 0.0;
  }
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_COVARIANCE_KERNEL_H_
