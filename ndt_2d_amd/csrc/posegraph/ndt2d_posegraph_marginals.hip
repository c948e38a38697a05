// Marginal covariances of the pose graph on the device (include/ndt2d_hip.h, "Marginal
// covariances"): block columns of (H_FF + damping clamp(diag H_FF))^-1 at given poses, each column
// one preconditioned CG from 0 on the solver's own operator (gfx950 / MI355X).
//
//   marginals_linearize_kernel, marginals_columns_kernel   a job's linearisation and preconditioner
//       once, then a workgroup per (job, query node) whose three columns run one CG loop in
//       lockstep, or three workgroups with a column each.  Their heads below say the rest.
//
// Both are built from posegraph/ndt2d_posegraph_kernel.h -- the solver's pg_linearize, its chain
// preconditioner and its reductions, under that header's contract of determinism, bounds and LDS
// (1,280 bytes; registers and scratch: DESIGN.md 3.18.3) -- and pg_matvec3 here, the solver's
// matrix-vector product with three vectors.  The object, the prelude a call begins with and a
// chunk's poses are posegraph/ndt2d_posegraph_state.h, what the call refuses about the damping, the
// query nodes and the poses posegraph/ndt2d_posegraph_args.h; `relative` and `distance`, host only,
// are posegraph/ndt2d_posegraph_relative.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "posegraph/ndt2d_posegraph_args.h"
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "posegraph/ndt2d_posegraph_relative.h"
#include "posegraph/ndt2d_posegraph_state.h"

namespace ndt2d
{

namespace
{

constexpr size_t kPgMargRec = NDT2D_MARGINALS_RECORD_DOUBLES;
constexpr size_t kPgMargDeviceRec = 9;   // what the columns kernel writes per pair: 3 x {status, iterations, |r|_2}
// per (job, query) workgroup and node: x, r, p, z, Hp of the three columns (9 each); "chain" adds
// the reduced right-hand sides (9)
constexpr size_t kPgColumnDoubles = 5 * 9, kPgColumnChainDoubles = 9;

// A job's read-only block is a solver workspace (pg_job_doubles: PgWork, under a loss rho' in front,
// "chain"'s arrays behind) in which x, cos / sin, act, H's blocks, the preconditioner's inverses and
// the chain's factors are filled in; one double behind it says whether the chain's pivots held.
template <int kPrec>
__device__ __forceinline__ size_t pg_marginals_flag(size_t n)
{
  return (kPrec == kPgChain ? kPgNodeDoubles + kPgChainDoubles : kPgNodeDoubles) * n;
}

//   marginals_linearize_kernel   grid (job of the chunk), 1,024 threads.  At the job's poses: trig,
//       active flags, rho' and H's diagonal blocks by pg_linearize, the Jacobi inverses at `damping`,
//       and for "chain" the couplings and the factors of the band, once.
template <int kPrec, int kLoss>
__global__ void __launch_bounds__(kPgThreads) marginals_linearize_kernel(const PgGraph G, const uint8_t * enabled, const double * poses,
                                                                          size_t pose_stride, double * blocks, size_t block_doubles,
                                                                          double damping)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  const size_t job = blockIdx.x, n = G.n;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  double * const base = blocks + job * block_doubles + (kLoss == 0 ? 0 : G.m);
  const PgWork w(base, n);
  const double * xs = poses + job * pose_stride;
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
#pragma unroll
    for (int j = 0; j < 3; ++j) w.x[3 * at + j] = xs[3 * at + j];
  }
  pg_trig(w.x, w.cs, G.n);
  __syncthreads();
  (void)pg_linearize<kPrec, kLoss>(G, en, w, sc, parity);
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
    double S[6], M[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) S[j] = w.hd[6 * at + j];
    S[0] += damping * pg_clamp_diag(S[0]);
    S[3] += damping * pg_clamp_diag(S[3]);
    S[5] += damping * pg_clamp_diag(S[5]);
    if (w.act[at] == 0.0 || !pg::invert_sym(S, M))
    {
#pragma unroll
      for (int j = 0; j < 6; ++j) M[j] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) w.mi[6 * at + j] = M[j];
  }
  double held = 0.0;
  if constexpr (kPrec == kPgChain)
  {
    const PgChainWork ch(base + kPgNodeDoubles * n, n);
    pg_chain_couplings<kLoss>(G, en, w, ch);
    held = pg_chain_factor(G, w, ch, damping, sc, parity) ? 1.0 : 0.0;
  }
  if (threadIdx.x == 0) base[pg_marginals_flag<kPrec>(n)] = held;
}

// hp = (H + damping D) p of the live columns among three, the thread's nodes; php: the thread's
// shares of p . hp.  pg_matvec with three vectors: a gathered constraint's W, end nodes, trig and
// frame are taken once, each column has the operations of pg_matvec in its order.  Vectors are
// [column][node][3].
template <int kLoss>
__device__ __forceinline__ void pg_matvec3(const PgGraph & G, const uint8_t * en, const PgWork & w, const double * P, double * HP, double damping,
                                           const bool (&live)[3], double (&php)[3])
{
  const size_t n3 = 3 * static_cast<size_t>(G.n);
  php[0] = php[1] = php[2] = 0.0;
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
    double acc[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (w.act[at] != 0.0)
    {
      const uint32_t k1 = G.node_ptr[i + 1];
      for (uint32_t k = G.node_ptr[i]; k < k1; ++k)
      {
        const uint32_t entry = G.node_con[k], c = entry >> 1;
        if (en != nullptr && en[c] == 0) continue;
        const uint32_t a = G.begin[c], b = G.end[c];
        const pg::Frame f = pg_frame(w, a, b);
        const double * W = G.W + 9 * static_cast<size_t>(c);
        [[maybe_unused]] double rw = 1.0;
        if constexpr (kLoss != 0) rw = pg_weights(G, w)[c];
#pragma unroll
        for (int col = 0; col < 3; ++col)
        {
          if (!live[col]) continue;
          double va[3], vb[3], v[3], u[3], t[3], y[3];
          pg::apply_a(f, P + col * n3 + 3 * static_cast<size_t>(a), va);
          pg::apply_b(f, P + col * n3 + 3 * static_cast<size_t>(b), vb);
          v[0] = va[0] + vb[0];
          v[1] = va[1] + vb[1];
          v[2] = va[2] + vb[2];
          pg::mul(W, v, u);
          pg::mul_t(W, u, t);
          if (entry & 1u) pg::apply_bt(f, t, y);
          else pg::apply_at(f, t, y);
          if constexpr (kLoss == 0)
          {
            acc[col][0] += y[0];
            acc[col][1] += y[1];
            acc[col][2] += y[2];
          }
          else
          {
            acc[col][0] += rw * y[0];
            acc[col][1] += rw * y[1];
            acc[col][2] += rw * y[2];
          }
        }
      }
      const double * S = w.hd + 6 * at;
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (!live[col]) continue;
        const double * pi = P + col * n3 + 3 * at;
        acc[col][0] += damping * pg_clamp_diag(S[0]) * pi[0];
        acc[col][1] += damping * pg_clamp_diag(S[3]) * pi[1];
        acc[col][2] += damping * pg_clamp_diag(S[5]) * pi[2];
        php[col] += (pi[0] * acc[col][0] + pi[1] * acc[col][1]) + pi[2] * acc[col][2];
      }
    }
#pragma unroll
    for (int col = 0; col < 3; ++col)
    {
      if (!live[col]) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) HP[col * n3 + 3 * at + j] = acc[col][j];
    }
  }
}

//   marginals_columns_kernel   grid ((job, query) pair of the chunk), 1,024 threads: the three
//       columns of the query node advance in lockstep through one CG loop on the job's block, which
//       it only reads.  They share every barrier, every load of a constraint and its frame, and the
//       reductions (pg_block_sum<3>); each has its own alpha, beta and stop.  A column that has
//       stopped is frozen: its x, r and p are not written again, and nothing of it enters a live
//       column's arithmetic -- a column's bits do not depend on its siblings, nor on the other
//       pairs.  "chain": the job's factors, applied per live column to the column's own right-hand
//       side; the Jacobi blocks where a pivot of the band did not hold.
//       kCols = 3 is that form.  kCols = 1: three workgroups per pair, each with one column live from
//       the start -- the same operations in the same order per column, so the same bits.  Which form a
//       chunk takes is the host's choice by the chunk's size (pg_marginals_form; DESIGN.md 3.18.3 has
//       the measurement): it changes no output.  records: [pair][kPgMargDeviceRec] = per column the
//       status, the iteration it stopped at and |r|_2, each written by the workgroup that has the column.
template <int kPrec, int kLoss, int kCols>
__global__ void __launch_bounds__(kPgThreads) marginals_columns_kernel(const PgGraph G, const uint8_t * enabled, const double * blocks,
                                                                        size_t block_doubles, double * workspace, const uint32_t * nodes,
                                                                        uint32_t n_nodes, size_t first_pair, size_t first_job, double damping,
                                                                        double tolerance, uint32_t cg_cap, double * blocks_out,
                                                                        double * columns_out, double * records)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  static_assert(kCols == 3 || kCols == 1, "three columns in lockstep, or one a workgroup");
  const size_t slot = kCols == 3 ? blockIdx.x : blockIdx.x / 3;   // the pair's place in the chunk
  [[maybe_unused]] const int only = static_cast<int>(blockIdx.x % 3);   // kCols = 1: this workgroup's column
  const size_t n = G.n, n3 = 3 * n, pair = first_pair + slot;
  const size_t job = pair / n_nodes - first_job;
  const uint32_t node = nodes[pair % n_nodes];
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  double * const base = const_cast<double *>(blocks) + job * block_doubles + (kLoss == 0 ? 0 : G.m);   // (read only)
  const PgWork w(base, n);
  constexpr size_t per_node = kPrec == kPgChain ? kPgColumnDoubles + kPgColumnChainDoubles : kPgColumnDoubles;
  double * const X = workspace + blockIdx.x * per_node * n;
  double * const R = X + 3 * n3, * const P = R + 3 * n3, * const Z = P + 3 * n3, * const HP = Z + 3 * n3;
  [[maybe_unused]] double * const B = HP + 3 * n3;
  [[maybe_unused]] bool chain = false;
  if constexpr (kPrec == kPgChain) chain = pg_uniform(base[pg_marginals_flag<kPrec>(n)]) != 0.0;
  const bool is_free = pg_uniform(w.act[node]) != 0.0;
  const bool mine[3] = {kCols == 3 || only == 0, kCols == 3 || only == 1, kCols == 3 || only == 2};
  bool live[3] = {is_free && mine[0], is_free && mine[1], is_free && mine[2]};

  // x = 0, r = the unit vectors of the node's three unknowns, z = M^-1 r, p = z
  double rz[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
#pragma unroll
    for (int col = 0; col < 3; ++col)
    {
      double r[3], z[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) r[j] = is_free && i == node && j == col ? 1.0 : 0.0;
      pg::mul_sym(w.mi + 6 * at, r, z);
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        X[col * n3 + 3 * at + j] = 0.0;
        R[col * n3 + 3 * at + j] = r[j];
        Z[col * n3 + 3 * at + j] = z[j];
        P[col * n3 + 3 * at + j] = z[j];
        HP[col * n3 + 3 * at + j] = 0.0;
        if constexpr (kPrec == kPgChain) B[col * n3 + 3 * at + j] = r[j];
      }
      rz[col] += (r[0] * z[0] + r[1] * z[1]) + r[2] * z[2];
    }
  }
  if constexpr (kPrec == kPgChain)
  {
    if (chain && is_free)
    {
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (!live[col]) continue;
        PgWork wc = w;
        wc.r = R + col * n3;
        wc.z = Z + col * n3;
        wc.p = P + col * n3;
        PgChainWork cc(base + kPgNodeDoubles * n, n);
        cc.b = B + col * n3;
        pg_chain_apply(G, wc, cc);
        rz[col] = pg_chain_rz<true>(G, wc);
      }
    }
  }
  pg_block_sum(rz, sc, parity);   // (its barrier: p is whole)

  constexpr uint32_t kLive = 0xFFFFFFFFu;
  uint32_t status[3] = {kLive, kLive, kLive}, stopped[3] = {0u, 0u, 0u}, iterations = 0;
  double rr[3] = {live[0] ? 1.0 : 0.0, live[1] ? 1.0 : 0.0, live[2] ? 1.0 : 0.0};
  while ((live[0] || live[1] || live[2]) && iterations < cg_cap)
  {
    double s3[3], alpha[3] = {0.0, 0.0, 0.0};
    pg_matvec3<kLoss>(G, en, w, P, HP, damping, live, s3);
    pg_block_sum(s3, sc, parity);
#pragma unroll
    for (int col = 0; col < 3; ++col)
    {
      if (!live[col]) continue;
      if (!(s3[col] > 0.0) || !(rz[col] > 0.0) || !isfinite(s3[col]) || !isfinite(rz[col]))
      {
        live[col] = false;
        status[col] = NDT2D_MARGINALS_BREAKDOWN;
        stopped[col] = iterations;
      }
      else
      {
        alpha[col] = rz[col] / s3[col];
      }
    }
    s3[0] = s3[1] = s3[2] = 0.0;
    for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
    {
      const size_t at = static_cast<size_t>(i);
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (!live[col]) continue;
        double r[3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
          const size_t e = col * n3 + 3 * at + j;
          X[e] += alpha[col] * P[e];
          r[j] = R[e] - alpha[col] * HP[e];
          R[e] = r[j];
          if constexpr (kPrec == kPgChain) B[e] = r[j];
        }
        s3[col] += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
      }
    }
    pg_block_sum(s3, sc, parity);
    ++iterations;
#pragma unroll
    for (int col = 0; col < 3; ++col)
    {
      if (!live[col]) continue;
      rr[col] = s3[col];
      stopped[col] = iterations;
      const double norm = sqrt(s3[col]);
      if (!isfinite(norm))
      {
        live[col] = false;
        status[col] = NDT2D_MARGINALS_BREAKDOWN;
      }
      else if (norm <= tolerance)
      {
        live[col] = false;
        status[col] = NDT2D_MARGINALS_CONVERGED;
      }
    }
    if (!(live[0] || live[1] || live[2])) break;
    // z = M^-1 r, r . z, p = z + beta p of the live columns
    s3[0] = s3[1] = s3[2] = 0.0;
    bool jacobi = true;
    if constexpr (kPrec == kPgChain)
    {
      if (chain)
      {
        jacobi = false;
#pragma unroll
        for (int col = 0; col < 3; ++col)
        {
          if (!live[col]) continue;
          PgWork wc = w;
          wc.r = R + col * n3;
          wc.z = Z + col * n3;
          wc.p = P + col * n3;
          PgChainWork cc(base + kPgNodeDoubles * n, n);
          cc.b = B + col * n3;
          pg_chain_apply(G, wc, cc);
          s3[col] = pg_chain_rz<false>(G, wc);
        }
      }
    }
    if (jacobi)
    {
      for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
      {
        const size_t at = static_cast<size_t>(i);
#pragma unroll
        for (int col = 0; col < 3; ++col)
        {
          if (!live[col]) continue;
          const double * r = R + col * n3 + 3 * at;
          double z[3];
          pg::mul_sym(w.mi + 6 * at, r, z);
#pragma unroll
          for (int j = 0; j < 3; ++j) Z[col * n3 + 3 * at + j] = z[j];
          s3[col] += (r[0] * z[0] + r[1] * z[1]) + r[2] * z[2];
        }
      }
    }
    pg_block_sum(s3, sc, parity);
    double beta[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int col = 0; col < 3; ++col)
    {
      if (!live[col]) continue;
      beta[col] = s3[col] / rz[col];
      rz[col] = s3[col];
    }
    for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
    {
      const size_t at = static_cast<size_t>(i);
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (!live[col]) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
          const size_t e = col * n3 + 3 * at + j;
          P[e] = Z[e] + beta[col] * P[e];
        }
      }
    }
    __syncthreads();
  }
  __syncthreads();   // (x is whole, whichever way the loop was left or passed by)

  // the query's block column: block (i, this query) of every query node i, row-major rows of node i
  for (uint32_t q = pg_tid(); q < n_nodes; q += kPgThreads)
  {
    const size_t at = static_cast<size_t>(nodes[q]);
    double * out = blocks_out + (slot * static_cast<size_t>(n_nodes) + q) * 9;
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (mine[col]) out[3 * j + col] = X[col * n3 + 3 * at + j];
      }
    }
  }
  if (columns_out != nullptr)
  {
    for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
    {
      const size_t at = static_cast<size_t>(i);
      double * out = columns_out + (slot * n + at) * 9;
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
#pragma unroll
        for (int col = 0; col < 3; ++col)
        {
          if (mine[col]) out[3 * j + col] = X[col * n3 + 3 * at + j];
        }
      }
    }
  }
  if (threadIdx.x == 0)
  {
    double * rec = records + slot * kPgMargDeviceRec;
#pragma unroll
    for (int col = 0; col < 3; ++col)
    {
      if (!mine[col]) continue;
      // (a column still live here met the cap)
      const uint32_t st = !is_free ? NDT2D_MARGINALS_NOT_FREE : status[col] == kLive ? NDT2D_MARGINALS_CG_CAP : status[col];
      rec[col] = static_cast<double>(st);
      rec[3 + col] = static_cast<double>(stopped[col]);
      rec[6 + col] = sqrt(rr[col]);
    }
  }
}

// The columns a workgroup of marginals_columns_kernel advances for a chunk of `pairs` on a device of
// `units` compute units: one -- three workgroups a pair, three times the pairs' workspace -- while
// those workgroups find a compute unit each, three in lockstep beyond.  Measured (DESIGN.md 3.18.3,
// 1,000 poses, 256 compute units): one column a workgroup takes 0.41 to 0.58 of lockstep's time up
// to 85 pairs, 1.16 to 1.19 of it from 256 pairs on.  The two forms give the same bits.  The macros
// force one form, for that measurement (experiments/posegraph_marginals_timing.py).
uint32_t pg_marginals_form(size_t pairs, size_t units)
{
#if defined(NDT2D_MARGINALS_ONE_COLUMN)
  return 1;
#elif defined(NDT2D_MARGINALS_LOCKSTEP)
  return 3;
#else
  return 3 * pairs <= units ? 1 : 3;
#endif
}

// What the two marginals kernels are launched with.
struct PgMarginalsLaunch
{
  uint32_t jobs, pairs;          // blocks of the linearize and of the columns kernel
  const uint8_t * d_en;          // the masks of the chunk's jobs, or NULL
  const double * poses;          // the first job's poses
  size_t pose_stride;            // 0: the graph's poses for every job
  double * blocks;               // [jobs][block_doubles]
  size_t block_doubles;
  double * workspace;            // [pairs][(45 or 54) n]
  const uint32_t * nodes;
  uint32_t n_nodes;
  size_t first_pair, first_job;
  double damping, tolerance;
  uint32_t cg_cap;
  double * blocks_out, * columns_out, * records;
  uint32_t columns;              // a workgroup's columns: 3 or 1 (pg_marginals_form)
};

// The marginals kernels of the object's preconditioner and loss.
void pg_marginals(const ndt2d_posegraph * s, hipStream_t stream, const PgGraph & G, const PgMarginalsLaunch & a)
{
  pg_dispatch(s, [&](auto prec, auto loss) {
    constexpr int kPrec = decltype(prec)::value, kLoss = decltype(loss)::value;
    hipLaunchKernelGGL((marginals_linearize_kernel<kPrec, kLoss>), dim3(a.jobs), dim3(kPgThreads), 0, stream, G, a.d_en, a.poses, a.pose_stride,
                       a.blocks, a.block_doubles, a.damping);
    const auto kernel = a.columns == 1 ? marginals_columns_kernel<kPrec, kLoss, 1> : marginals_columns_kernel<kPrec, kLoss, 3>;
    hipLaunchKernelGGL(kernel, dim3(a.columns == 1 ? 3 * a.pairs : a.pairs), dim3(kPgThreads), 0, stream, G, a.d_en, a.blocks, a.block_doubles,
                       a.workspace, a.nodes, a.n_nodes, a.first_pair, a.first_job, a.damping, a.tolerance, a.cg_cap, a.blocks_out, a.columns_out,
                       a.records);
  });
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_marginals_columns(ndt2d_posegraph * s, const uint8_t * enabled, size_t n_jobs, const double * poses, const uint32_t * nodes,
                            size_t n_nodes, double damping, double tolerance, uint32_t max_cg_iterations, double * blocks_out,
                            double * columns_out, double * records_out)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0 || n_nodes == 0) return NDT2D_OK;
  namespace args = ndt2d::pg_args;
  const char * const entry = "ndt2d_marginals_columns";
  const std::string who = std::string(entry) + ": ";
  if (nodes == nullptr || blocks_out == nullptr || records_out == nullptr) return batch_fail(s, NDT2D_ERR_INVALID, who + "null argument");
  int rc = ndt2d::batch_refuse(s, args::damping_refusal(entry, damping));
  if (rc != NDT2D_OK) return rc;
  if (!(tolerance > 0.0) || !std::isfinite(tolerance)) return batch_fail(s, NDT2D_ERR_INVALID, who + "the tolerance is not finite and > 0");
  const size_t Q = n_nodes;
  ndt2d::PgCall call;
  rc = ndt2d::pg_begin_call(s, s, entry, &call, [&] {
    if (Q > 0xFFFFFFFFu) return who + "more than 2^32 - 1 query nodes";
    const std::string named = args::nodes_refusal(entry, "query", nodes, Q, 1, s->n);
    return !named.empty() ? named : args::poses_refusal(entry, poses, n_jobs, s->n);
  });
  if (rc != NDT2D_OK) return rc;
  const hipStream_t stream = call.stream;
  const ndt2d::PgGraph & G = call.G;
  const size_t n = s->n;
  NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_marginal_nodes, &s->marginal_nodes_cap, Q * sizeof(uint32_t)));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_marginal_nodes, nodes, Q * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  ndt2d::PgMarginalsLaunch a{};
  a.nodes = static_cast<const uint32_t *>(s->d_marginal_nodes);
  a.n_nodes = static_cast<uint32_t>(Q);
  a.damping = damping;
  a.tolerance = tolerance;
  a.cg_cap = max_cg_iterations != 0 ? max_cg_iterations : ndt2d::pg_cg_cap(static_cast<uint32_t>(n));
  // a job's block (a solver workspace and the chain's flag), a pair's vectors
  a.block_doubles = ndt2d::pg_job_doubles(s) + 1;
  const size_t pair_doubles = (ndt2d::kPgColumnDoubles + (s->chain ? ndt2d::kPgColumnChainDoubles : 0)) * n;
  if (s->compute_units == 0)
  {
    int units = 0;
    NDT2D_BATCH_HIP(s, hipDeviceGetAttribute(&units, hipDeviceAttributeMultiprocessorCount, s->device));
    s->compute_units = units > 0 ? static_cast<size_t>(units) : 1;
  }
  // the (job, query) pairs, job-major, in chunks of at most max_jobs workgroups
  const size_t total_pairs = n_jobs * Q;
  for (size_t t0 = 0; t0 < total_pairs; t0 += s->max_jobs)
  {
    const size_t t1 = std::min(total_pairs, t0 + s->max_jobs), pc = t1 - t0;
    const size_t k0 = t0 / Q, k1 = (t1 - 1) / Q + 1, kc = k1 - k0;   // the jobs the chunk's pairs belong to
    rc = ndt2d::pg_send_masks(s, stream, enabled, k0, k1, &a.d_en);
    if (rc != NDT2D_OK) return rc;
    rc = ndt2d::pg_chunk_poses(s, stream, &s->marginal_poses, poses, k0, kc, n, G, &a.poses, &a.pose_stride);
    if (rc != NDT2D_OK) return rc;
    a.columns = ndt2d::pg_marginals_form(pc, s->compute_units);
    const size_t groups = a.columns == 1 ? 3 * pc : pc;   // workgroups, each with vectors of its own
    NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_marginals, &s->marginals_cap, (kc * a.block_doubles + groups * pair_doubles) * sizeof(double)));
    a.blocks = static_cast<double *>(s->d_marginals);
    a.workspace = a.blocks + kc * a.block_doubles;
    // what comes back: [blocks pc Q 9 | records pc 9 | columns pc n 9]
    const size_t at_rec = pc * Q * 9, at_col = at_rec + pc * ndt2d::kPgMargDeviceRec;
    const size_t total = at_col + (columns_out != nullptr ? pc * n * 9 : 0);
    NDT2D_BATCH_HIP(s, ndt2d::grow_pair(&s->h_out, &s->d_out, &s->out_cap, total));
    a.jobs = static_cast<uint32_t>(kc);
    a.pairs = static_cast<uint32_t>(pc);
    a.first_pair = t0;
    a.first_job = k0;
    a.blocks_out = s->d_out;
    a.records = s->d_out + at_rec;
    a.columns_out = columns_out != nullptr ? s->d_out + at_col : nullptr;
    rc = ndt2d::batch_round_trip(s, stream, total, [&] {
      ndt2d::pg_marginals(s, stream, G, a);
      return NDT2D_OK;
    });
    if (rc != NDT2D_OK) return rc;
    for (size_t t = t0; t < t1; ++t)
    {
      const size_t k = t / Q, j = t % Q;
      const double * col = s->h_out + (t - t0) * Q * 9;
      for (size_t i = 0; i < Q; ++i) std::memcpy(blocks_out + ((k * Q + i) * Q + j) * 9, col + i * 9, 9 * sizeof(double));
    }
    for (size_t t = t0; t < t1; ++t)
    {
      // the query's record of its three columns': BREAKDOWN before CG_CAP before CONVERGED, the last column's iterations
      const double * dev = s->h_out + at_rec + (t - t0) * ndt2d::kPgMargDeviceRec;
      double * rec = records_out + t * ndt2d::kPgMargRec;
      double worst = dev[0], iterations = dev[3];
      for (int col = 1; col < 3; ++col)
      {
        if (dev[col] == NDT2D_MARGINALS_BREAKDOWN || (dev[col] == NDT2D_MARGINALS_CG_CAP && worst == NDT2D_MARGINALS_CONVERGED)) worst = dev[col];
        iterations = std::max(iterations, dev[3 + col]);
      }
      rec[0] = worst;
      rec[1] = iterations;
      for (int col = 0; col < 3; ++col) rec[2 + col] = dev[6 + col];
    }
    if (columns_out != nullptr) std::memcpy(columns_out + t0 * n * 9, s->h_out + at_col, pc * n * 9 * sizeof(double));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_marginals_relative(const double * pose_a, const double * pose_b, const double * joint, double * transform_out, double * covariance_out)
{
  NDT2D_C_TRY
  if (pose_a == nullptr || pose_b == nullptr || joint == nullptr || transform_out == nullptr || covariance_out == nullptr) return NDT2D_ERR_INVALID;
  for (int i = 0; i < 3; ++i)
  {
    if (!std::isfinite(pose_a[i]) || !std::isfinite(pose_b[i])) return NDT2D_ERR_INVALID;
  }
  for (int i = 0; i < 36; ++i)
  {
    if (!std::isfinite(joint[i])) return NDT2D_ERR_INVALID;
  }
  ndt2d::posegraph::relative(std::cos(pose_a[2]), std::sin(pose_a[2]), pose_a, pose_b, joint, transform_out, covariance_out);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_marginals_distance(const double * transform_pred, const double * covariance_pred, const double * transform_meas,
                             const double * covariance_meas, double * d2_out)
{
  NDT2D_C_TRY
  if (transform_pred == nullptr || covariance_pred == nullptr || transform_meas == nullptr || covariance_meas == nullptr || d2_out == nullptr)
  {
    return NDT2D_ERR_INVALID;
  }
  for (int i = 0; i < 3; ++i)
  {
    if (!std::isfinite(transform_pred[i]) || !std::isfinite(transform_meas[i])) return NDT2D_ERR_INVALID;
  }
  return ndt2d::posegraph::distance(transform_pred, covariance_pred, transform_meas, covariance_meas, d2_out) ? NDT2D_OK : NDT2D_ERR_INVALID;
  NDT2D_C_CATCH(nullptr)
}

}  // extern "C"
