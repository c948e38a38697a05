// The kernels of the direct pose-graph solve (direct/ndt2d_direct.hip; include/ndt2d_hip.h, "Direct
// solve"), all FP64, gfx950 / MI355X: Levenberg-Marquardt whose linear step is exact,
// (H_FF + lambda clamp(diag)) delta = -g by the dense covariance's assembly and blocked Cholesky
// (covariance/ndt2d_covariance_kernel.h, on this unit's layout DirectJob) and the two substitutions
// here.  The cost, the linearisation and the reductions are the CG solver's
// (posegraph/ndt2d_posegraph_kernel.h); the decisions are direct/ndt2d_direct_step.h; what a job holds
// is direct/ndt2d_direct_plan.h.
//
// One LM iteration of a chunk is a fixed list of launches (direct/ndt2d_direct.hip, direct_iteration);
// a job is blockIdx.z of the dense launches and blockIdx.x of the three kernels here.  A job whose
// status has left MAX_ITERATIONS is left alone by the substitution and the step: what the assembly
// and the factor compute for it afterwards is not read.
//
// Determinism.  No atomics.  The sums of the cost and the linearisation are the solver's; an element
// of the substitution's vector has one owner thread per panel, which sums the panel's 48 terms in
// ascending k from zero and subtracts the sum once; inside a panel's triangle the unknowns are
// eliminated in order (forward ascending, backward descending), each by its own lane.
//
// Bounds.  Every loop is bounded by ld, 48, n, m or a node's degree before it starts.
//
// LDS: the substitution 19,200 bytes (a 48 x 49 triangle and 48 values), begin and step 1,280.
// Registers and scratch: DESIGN.md 3.18.5.
// Included by the .hip translation units only.
#ifndef NDT2D_DIRECT_KERNEL_H_
#define NDT2D_DIRECT_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>

#include "covariance/ndt2d_covariance_kernel.h"
#include "covariance/ndt2d_covariance_plan.h"
#include "direct/ndt2d_direct_plan.h"
#include "direct/ndt2d_direct_step.h"
#include "posegraph/ndt2d_posegraph_kernel.h"

namespace ndt2d
{

namespace
{

static_assert(direct::kNodeDoubles == kPgNodeDoubles, "the plan's PgWork");
static_assert(sizeof(direct::State) == 11 * sizeof(double), "the state is doubles only");
constexpr size_t kDirectLm = 13;   // a job's State in the state region, in doubles (11 used)
static_assert(kDirectLm + kCovRec == direct::kStateDoubles, "the plan's state");
constexpr size_t kDirectRec = NDT2D_DIRECT_RECORD_DOUBLES;
constexpr uint32_t kDirectFinishThreads = 256;

// A job's dense part, as the covariance's kernels take a layout: no T.
struct DirectJob
{
  static constexpr bool kInverse = false;
  double * A, * diag, * cs, * act, * rhs;
  __device__ __forceinline__ DirectJob(double * workspace, size_t n, size_t job)
  {
    const size_t ld = cov::padded(3 * n);
    A = workspace + job * direct::dense_doubles(n);
    diag = A + ld * ld;
    cs = diag + ld;
    act = cs + 2 * n;
    rhs = act + n;
  }
};

// A chunk's workspace as the kernels take it.
struct DirectChunk
{
  double * dense;       // [job][dense_doubles(n)]
  double * work;        // [job][work_stride]: (rho' per constraint, m, under a loss |) PgWork
  double * state;       // [job][kDirectLm]
  double * factor;      // [job][kCovRec] the factor kernel's records
  size_t work_stride;
  size_t work_front;    // m under a loss, else 0
  using Job = DirectJob;   // the layout of `dense`
  __device__ __forceinline__ double * work_of(size_t job) const { return work + job * work_stride + work_front; }
  // where the substitution takes g from and leaves delta: the job's PgWork
  __device__ __forceinline__ PgWork vectors_of(size_t job, size_t n) const { return PgWork(work_of(job), n); }
  __device__ __forceinline__ direct::State * state_of(size_t job) const { return reinterpret_cast<direct::State *>(state + job * kDirectLm); }
};

// A job's state, the same bits in every lane, in scalar registers.
__device__ __forceinline__ direct::State direct_load_state(const direct::State * at)
{
  direct::State s;
  s.status = pg_uniform(at->status);
  s.iterations = pg_uniform(at->iterations);
  s.rejected = pg_uniform(at->rejected);
  s.not_positive_definite = pg_uniform(at->not_positive_definite);
  s.initial_cost = pg_uniform(at->initial_cost);
  s.cost = pg_uniform(at->cost);
  s.gradient = pg_uniform(at->gradient);
  s.pivot_ratio = pg_uniform(at->pivot_ratio);
  s.lambda = pg_uniform(at->lambda);
  s.nu = pg_uniform(at->nu);
  s.cost_before = pg_uniform(at->cost_before);
  return s;
}

__device__ __forceinline__ direct::Rules direct_rules(const PgRules & r)
{
  return direct::Rules{r.max_iterations, r.gradient_tolerance, r.function_tolerance, r.parameter_tolerance};
}

//   direct_begin_kernel   grid (job), 1,024 threads: x = the start poses, F (evaluate's bits), g, the
//       diagonal blocks and |g|_inf there, and the job's first state.
template <int kLoss>
__global__ void __launch_bounds__(kPgThreads) direct_begin_kernel(const PgGraph G, const uint8_t * enabled, const DirectChunk chunk,
                                                                   const PgRules rules)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  const size_t job = blockIdx.x, n = G.n;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  const PgWork w(chunk.work_of(job), n);
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
#pragma unroll
    for (int j = 0; j < 3; ++j) w.x[3 * at + j] = G.poses[3 * at + j];
  }
  pg_trig(w.x, w.cs, G.n);
  __syncthreads();
  const double F = pg_cost<kPgJacobi, kLoss>(G, en, w.x, w.cs, sc, parity);
  double gmax = 0.0;
  if (isfinite(F)) gmax = pg_linearize<kPgJacobi, kLoss>(G, en, w, sc, parity);
  direct::State s;
  direct::begin(s, F, gmax, direct_rules(rules));
  if (threadIdx.x == 0) *chunk.state_of(job) = s;
}

//   direct_substitute_kernel   grid (job), 1,024 threads: L y = -g, then L^T delta = y, on the factor
//       the covariance's launches left in A (row-major, ld = padded(3 n), panels of 48).  The vector
//       lies in the job's dense part (global memory: up to 65,520 doubles), the panel's 48 x 48
//       triangle and its 48 solved values in LDS.  Per panel, forward: wave 0 eliminates the
//       triangle's unknowns in ascending order, lane r its own row's value; then thread i takes row
//       i below the panel, rhs[i] -= sum_k L[i, j0 + k] y[k], k ascending from zero.  Backward, from
//       the last panel: wave 0 eliminates in descending order; then thread j takes column j before
//       the panel, rhs[j] -= sum_k L[j0 + k, j] delta[j0 + k], k ascending from zero (the threads
//       of a wave read consecutive columns: coalesced).  delta goes to the solver's PgWork.  A job
//       that is not iterating, or whose factorisation failed, is left alone.  Chunk: the chunk's layout,
//       DirectChunk by default; the sparse solve (sparse/ndt2d_sparse_kernel.h) runs the substitution on
//       the separators' matrix with a layout of its own (n is then the number of separators).
template <class Chunk = DirectChunk>
__global__ void __launch_bounds__(kPgThreads) direct_substitute_kernel(uint32_t n, const Chunk chunk, const PgRules rules)
{
  __shared__ double T[cov::kPanel][kCovLds];
  __shared__ double solved[cov::kPanel];
  const size_t job = blockIdx.x;
  const direct::State s = direct_load_state(chunk.state_of(job));
  if (!direct::iterating(s, direct_rules(rules))) return;
  if (pg_uniform(chunk.factor[job * kCovRec]) != 0.0) return;
  const typename Chunk::Job w(chunk.dense, n, job);
  const auto pw = chunk.vectors_of(job, n);
  const size_t d = 3 * static_cast<size_t>(n), ld = cov::padded(d);
  const uint32_t np = static_cast<uint32_t>(ld / cov::kPanel), lane = threadIdx.x;
  for (size_t i = threadIdx.x; i < ld; i += kPgThreads) w.rhs[i] = i < d ? -pw.g[i] : 0.0;
  __syncthreads();
  for (uint32_t p = 0; p < np; ++p)
  {
    const size_t j0 = static_cast<size_t>(p) * cov::kPanel;
    cov_load_block<false>(w.A, ld, j0, j0, T, kPgThreads);
    __syncthreads();
    if (threadIdx.x < kWave)
    {
      const uint32_t r = lane < cov::kPanel ? lane : cov::kPanel - 1;   // (lanes 48 .. 63 shadow row 47 and store nothing)
      double b = w.rhs[j0 + r];
      for (uint32_t c = 0; c < cov::kPanel; ++c)
      {
        const double y = __shfl(b, static_cast<int>(c)) / T[c][c];
        if (r == c) b = y;
        else if (r > c) b -= T[r][c] * y;
      }
      if (lane < cov::kPanel)
      {
        solved[lane] = b;
        w.rhs[j0 + lane] = b;
      }
    }
    __syncthreads();
    for (size_t i = j0 + cov::kPanel + threadIdx.x; i < ld; i += kPgThreads)
    {
      const double * row = w.A + i * ld + j0;
      double t = 0.0;
#pragma unroll 8
      for (uint32_t k = 0; k < cov::kPanel; ++k) t += row[k] * solved[k];
      w.rhs[i] -= t;
    }
    __syncthreads();
  }
  for (uint32_t q = 0; q < np; ++q)
  {
    const uint32_t p = np - 1 - q;
    const size_t j0 = static_cast<size_t>(p) * cov::kPanel;
    cov_load_block<false>(w.A, ld, j0, j0, T, kPgThreads);
    __syncthreads();
    if (threadIdx.x < kWave)
    {
      const uint32_t r = lane < cov::kPanel ? lane : 0u;   // (lanes 48 .. 63 shadow row 0 and store nothing)
      double b = w.rhs[j0 + r];
      for (uint32_t e = 0; e < cov::kPanel; ++e)
      {
        const uint32_t c = cov::kPanel - 1 - e;
        const double x = __shfl(b, static_cast<int>(c)) / T[c][c];
        if (r == c) b = x;
        else if (r < c) b -= T[c][r] * x;
      }
      if (lane < cov::kPanel)
      {
        solved[lane] = b;
        w.rhs[j0 + lane] = b;
      }
    }
    __syncthreads();
    for (size_t j = threadIdx.x; j < j0; j += kPgThreads)
    {
      const double * column = w.A + j0 * ld + j;
      double t = 0.0;
#pragma unroll 8
      for (uint32_t k = 0; k < cov::kPanel; ++k) t += column[k * ld] * solved[k];
      w.rhs[j] -= t;
    }
    __syncthreads();
  }
  for (size_t i = threadIdx.x; i < d; i += kPgThreads) pw.d[i] = w.rhs[i];
}

//   direct_step_kernel   grid (job), 1,024 threads: the trial point (the solver's d == 0 ? x : x + d),
//       the model's decrease 1/2 (lambda delta^T D delta - g^T delta), the trial's cost, the decision
//       (direct/ndt2d_direct_step.h, by every thread on the same reduced values: uniform control
//       flow) and, on acceptance, x, the linearisation there and the stop rules.  Thread 0 stores
//       the state, with plain stores, behind a barrier.
template <int kLoss>
__global__ void __launch_bounds__(kPgThreads) direct_step_kernel(const PgGraph G, const uint8_t * enabled, const DirectChunk chunk,
                                                                  const PgRules rules)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  const size_t job = blockIdx.x, n = G.n;
  const direct::Rules lm = direct_rules(rules);
  direct::State s = direct_load_state(chunk.state_of(job));
  if (!direct::iterating(s, lm)) return;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  const PgWork w(chunk.work_of(job), n);
  direct::Input in{};
  in.factor_failed = pg_uniform(chunk.factor[job * kCovRec]) != 0.0;
  in.pivot_ratio = pg_uniform(chunk.factor[job * kCovRec + 2]);
  if (!in.factor_failed)
  {
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
    {
      const size_t at = static_cast<size_t>(i);
      const double * S = w.hd + 6 * at;
      const double D[3] = {pg_clamp_diag(S[0]), pg_clamp_diag(S[3]), pg_clamp_diag(S[5])};
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        const double x = w.x[3 * at + j], d = w.d[3 * at + j];
        w.xt[3 * at + j] = d == 0.0 ? x : x + d;   // (a pose that does not move keeps its bits, -0.0 included)
        s4[0] += w.g[3 * at + j] * d;
        s4[1] += s.lambda * D[j] * d * d;
        s4[2] += d * d;
        s4[3] += x * x;
      }
    }
    pg_trig(w.xt, w.cst, G.n);   // (each thread its own nodes: no barrier in between)
    pg_block_sum(s4, sc, parity);
    in.predicted = 0.5 * (s4[1] - s4[0]);
    in.step = sqrt(s4[2]);
    in.x_norm = sqrt(s4[3]);
  }
  if (direct::propose(s, in, lm) == direct::kEvaluate)
  {
    in.trial_cost = pg_cost<kPgJacobi, kLoss>(G, en, w.xt, w.cst, sc, parity);
    if (direct::take(s, in))
    {
      for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
      {
        const size_t at = static_cast<size_t>(i);
#pragma unroll
        for (int j = 0; j < 3; ++j) w.x[3 * at + j] = w.xt[3 * at + j];
        w.cs[2 * at] = w.cst[2 * at];
        w.cs[2 * at + 1] = w.cst[2 * at + 1];
      }
      __syncthreads();
      direct::settle(s, pg_linearize<kPgJacobi, kLoss>(G, en, w, sc, parity), lm);
    }
  }
  __syncthreads();   // (every thread has read the state it started from)
  if (threadIdx.x == 0) *chunk.state_of(job) = s;
}

//   direct_finish_kernel   grid (job), 256 threads: the job's poses and its record.  ([[maybe_unused]]:
//       the sparse covariance's unit takes this header with the sparse solve's kernels and has no poses to return.)
[[maybe_unused]] __global__ void __launch_bounds__(kDirectFinishThreads) direct_finish_kernel(uint32_t n, const DirectChunk chunk, double * poses_out,
                                                                             double * records)
{
  const size_t job = blockIdx.x, d = 3 * static_cast<size_t>(n);
  const PgWork w(chunk.work_of(job), n);
  for (size_t i = threadIdx.x; i < d; i += kDirectFinishThreads) poses_out[job * d + i] = w.x[i];
  if (threadIdx.x < kDirectRec) records[job * kDirectRec + threadIdx.x] = chunk.state[job * kDirectLm + threadIdx.x];
}

//   direct_chi2_kernel   grid (job), 1,024 threads: the evaluate kernel's chi2 of the chunk's jobs at
//       poses (posegraph/ndt2d_posegraph.hip's kernel is that unit's own: the constraint's arithmetic is
//       pg_constraint, one thread a constraint).
[[maybe_unused]] __global__ void __launch_bounds__(kPgThreads) direct_chi2_kernel(const PgGraph G, const double * poses, size_t pose_stride, double * chi2,
                                                                                   size_t chi2_stride)
{
  const size_t job = blockIdx.x;
  const double * xs = poses + job * pose_stride;
  for (uint32_t c = pg_tid(); c < G.m; c += kPgThreads)
  {
    double e[3], r[3];
    chi2[job * chi2_stride + c] = pg_constraint(G, c, xs, nullptr, e, r);
  }
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_DIRECT_KERNEL_H_
