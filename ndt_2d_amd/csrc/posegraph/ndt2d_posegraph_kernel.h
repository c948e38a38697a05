// What every pose-graph kernel is made of (posegraph/ndt2d_posegraph.hip: the solve and evaluate
// kernels; posegraph/ndt2d_posegraph_marginals.hip: the marginals kernels), once: the constants, the
// graph and a job's workspace as a kernel sees them, the block's reductions, a constraint's cost,
// the linearisation, the matrix-vector product and the chain preconditioner (gfx950 / MI355X).  The
// arithmetic of a constraint is posegraph/ndt2d_posegraph_fn.h, the block cyclic reduction
// posegraph/ndt2d_posegraph_chain.h, the losses posegraph/ndt2d_posegraph_loss.h.  Every kernel is a
// workgroup of 1,024 threads in which thread t owns nodes t, t + 1024, ... in every phase and
// constraints t, t + 1024, ... of the cost.
//
// Determinism.  No atomics.  A node's sums (g, its block of H, (H p)_i) are gathers over its incident
// constraints in ascending constraint index (the host's table); a dot product is each thread's
// strided partial in ascending order, the wave by an xor butterfly (every lane ends with the same
// bits), the 16 waves' partials through LDS, summed in wave order by every thread.  A job reads the
// shared graph, its mask and its own workspace only: its result does not depend on the other jobs.
//
// Bounds.  Every loop is bounded before it starts: by n, m, a node's degree, max_iterations or the
// CG cap.  Node and constraint indices are checked by the host at upload (ndt2d_posegraph_set_graph);
// a job's workspace is [job][kPgNodeDoubles * n] doubles, with "chain" kPgChainDoubles * n more and
// under a loss m more in front (pg_job_doubles); the loss's two doubles and m bytes lie behind the
// graph's arrays, which ndt2d_posegraph_set_graph sizes for them.
//
// LDS: 2 x 5 x 16 partials, 1,280 bytes.  Registers and scratch: DESIGN.md 3.18.
// Included by the .hip translation units only.
#ifndef NDT2D_POSEGRAPH_KERNEL_H_
#define NDT2D_POSEGRAPH_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>

#include "ndt2d_device_fn.h"
#include "ndt2d_hip.h"
#include "posegraph/ndt2d_posegraph_fn.h"
#include "posegraph/ndt2d_posegraph_chain.h"
#include "posegraph/ndt2d_posegraph_loss.h"

namespace ndt2d
{

namespace
{

namespace pg = posegraph;

constexpr uint32_t kPgThreads = 1024;
constexpr uint32_t kPgWaves = kPgThreads / kWave;
constexpr int kPgSums = 5;                      // sums one reduction carries at most
constexpr size_t kPgMaxJobs = 65535;            // blocks of a launch
constexpr size_t kPgMaxNodes = size_t(1) << 30;
constexpr size_t kPgMaxConstraints = size_t(1) << 30;   // (2 m table entries, each constraint << 1 | side, in 32 bits)
constexpr size_t kPgRec = NDT2D_POSEGRAPH_RECORD_DOUBLES;
constexpr uint32_t kPgCgCap = 8192;
// per node of a job's workspace: x, trial x, g, p, r, z, Hp, delta (3 each), H's block and the
// preconditioner's inverse (6 each), cos / sin at x and at the trial x (2 each), active (1)
constexpr size_t kPgNodeDoubles = 8 * 3 + 2 * 6 + 2 * 2 + 1;
// the preconditioner, the solve kernel's template argument
constexpr int kPgJacobi = 0, kPgChain = 1;
// what "chain" adds per node: H's block (i, i + 1) (9), the reduction's working diagonal (6) and
// coupling (9), the coupling (9) and the factored pivot (6) kept at the node's elimination, the
// reduced right-hand side (3)
constexpr size_t kPgChainDoubles = 9 + 6 + 9 + 9 + 6 + 3;

// The iterations a CG may take on n poses: the solver's per LM iteration, the marginals' default.
__host__ __device__ inline uint32_t pg_cg_cap(uint32_t n)
{
  return n >= kPgCgCap ? kPgCgCap : min(3u * n + 16u, kPgCgCap);
}

// Levenberg-Marquardt's own constants (free to the implementation: the contract is the minimiser).
constexpr double kPgLambda0 = 1e-4;             // 1 / Ceres's initial trust-region radius
constexpr double kPgLambdaMin = 1e-32, kPgLambdaMax = 1e32;
constexpr double kPgDiagMin = 1e-6, kPgDiagMax = 1e32;   // the clamp of diag(H) in the damping, as Ceres's
constexpr double kPgMinGain = 1e-3;             // a step is accepted above this gain ratio
constexpr double kPgNoise = 256.0 * 2.220446049250313e-16;   // |dF| <= this x F: below the cost's own rounding

struct PgGraph
{
  const double * poses;        // [n][3] the start poses
  const double * transform;    // [m][3]
  const double * W;            // [m][9] row-major: L or L^T of the information
  const uint32_t * begin;      // [m]
  const uint32_t * end;        // [m]
  const uint32_t * node_ptr;   // [n + 1]
  const uint32_t * node_con;   // [2 m]: constraint << 1 | (the node is its end), ascending per node
  uint32_t n, m, fixed;
};

struct PgRules
{
  uint32_t max_iterations;
  double gradient_tolerance, function_tolerance, parameter_tolerance;
};

struct PgScratch
{
  double part[2][kPgSums][kPgWaves];
};

// The loss of a robust instantiation (kLoss: pg::kLossHuber, pg::kLossCauchy): its scale a with
// b = a^2, and which constraints it applies to.  Both lie with the graph -- {a, b} behind W in the
// graph's doubles, the selection's m bytes behind node_con in its index (ndt2d_posegraph_set_graph
// leaves the room, pg_send_loss fills it) -- so that the kernels' arguments are the ones they had
// and the instantiations without a loss are the code they were.  Formed from G where it is used.
template <int kLoss>
struct PgLoss
{
  double a, b;
  const uint8_t * on;   // [m], non-zero: the loss applies
  __device__ __forceinline__ explicit PgLoss(const PgGraph & G)
  {
    const double * scale = G.W + 9 * static_cast<size_t>(G.m);
    a = scale[0];
    b = scale[1];
    on = reinterpret_cast<const uint8_t *>(G.node_con + 2 * static_cast<size_t>(G.m));
  }
  // rho(s) and rho'(s) of constraint c; a constraint the loss is not applied to has rho = s
  __device__ __forceinline__ double rho(uint32_t c, double s) const { return on[c] != 0 ? pg::loss_rho<kLoss>(s, a, b) : s; }
  __device__ __forceinline__ double weight(uint32_t c, double s) const { return on[c] != 0 ? pg::loss_weight<kLoss>(s, a, b) : 1.0; }
};

__device__ __forceinline__ double pg_wave_sum(double v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ double pg_wave_max(double v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// The thread's index, opaque to the optimiser at each use: otherwise it forms the thread's address
// into every array of every phase once, ahead of the iteration, and holds dozens of 64-bit
// pointers in vector registers across it (into scratch, at 128 registers a thread).
__device__ __forceinline__ uint32_t pg_tid()
{
  uint32_t t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// A value every lane holds with the same bits, moved to scalar registers: the solver's scalars and
// its control flow then cost no vector registers.
__device__ __forceinline__ double pg_uniform(double v)
{
  const uint64_t bits = __double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(bits));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(bits >> 32));
  return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(hi) << 32) | lo));
}

// N sums over the block, the same bits in every thread.  The two halves of `part` alternate, so one
// barrier per reduction is enough: a thread writes a half again only behind the barrier of the
// reduction in between, which every thread reaches after it has read that half.  The barrier also
// orders the block's global writes before it against the reads behind it.
template <int N>
__device__ __forceinline__ void pg_block_sum(double (&v)[N], PgScratch & sc, uint32_t & parity)
{
  static_assert(N <= kPgSums, "room in the scratch");
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k)
  {
    const double w = pg_wave_sum(v[k]);
    if (lane == 0) sc.part[parity][k][wave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k)
  {
    double t = sc.part[parity][k][0];
#pragma unroll
    for (uint32_t w = 1; w < kPgWaves; ++w) t += sc.part[parity][k][w];
    v[k] = pg_uniform(t);
  }
  parity ^= 1u;
}

__device__ __forceinline__ double pg_block_max(double v, PgScratch & sc, uint32_t & parity)
{
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const double w = pg_wave_max(v);
  if (lane == 0) sc.part[parity][0][wave] = w;
  __syncthreads();
  double t = sc.part[parity][0][0];
#pragma unroll
  for (uint32_t k = 1; k < kPgWaves; ++k) t = fmax(t, sc.part[parity][0][k]);
  parity ^= 1u;
  return pg_uniform(t);
}

// e, r = W e of constraint c at the poses xs; returns chi2 = |r|^2.  cos / sin of pose a's heading
// are the device library's, here and in the node cache: the same bits for the same heading.
// trig: [node][2] cos, sin of the headings in xs, or NULL to take them here.
__device__ __forceinline__ double pg_constraint(const PgGraph & G, uint32_t c, const double * xs, const double * trig, double * e, double * r)
{
  const size_t a = G.begin[c];
  const double * pa = xs + 3 * a;
  const double * pb = xs + 3 * static_cast<size_t>(G.end[c]);
  double sn, cs;
  if (trig != nullptr)
  {
    cs = trig[2 * a];
    sn = trig[2 * a + 1];
  }
  else
  {
    sincos(pa[2], &sn, &cs);
  }
  const pg::Frame f = pg::frame(cs, sn, pa, pb);
  pg::error(f, pa[2], pb[2], G.transform + 3 * static_cast<size_t>(c), e);
  pg::mul(G.W + 9 * static_cast<size_t>(c), e, r);
  return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
}

// F = 1/2 sum of rho(chi2) over the job's enabled constraints at xs; without a loss rho(s) = s.
// (pg_cost, pg_linearize and pg_matvec carry the solve kernel's template argument kPrec without
// using it: each instantiation of the kernel then has copies of its own, called as often as before
// there were two, and the inliner treats the "jacobi" kernel as it did -- shared between the two it
// left that one with 20 bytes of scratch.  kLoss they use, under `if constexpr`: with kLoss = 0
// nothing of it is compiled.)
template <int kPrec, int kLoss>
__device__ double pg_cost(const PgGraph & G, const uint8_t * en, const double * xs, const double * trig, PgScratch & sc, uint32_t & parity)
{
  double acc[1] = {0.0};
  for (uint32_t c = pg_tid(); c < G.m; c += kPgThreads)
  {
    if (en != nullptr && en[c] == 0) continue;
    double e[3], r[3];
    if constexpr (kLoss == 0) acc[0] += pg_constraint(G, c, xs, trig, e, r);
    else acc[0] += PgLoss<kLoss>(G).rho(c, pg_constraint(G, c, xs, trig, e, r));
  }
  pg_block_sum(acc, sc, parity);
  return 0.5 * acc[0];
}

// A job's workspace.
struct PgWork
{
  double * x, * xt, * g, * p, * r, * z, * hp, * d, * hd, * mi, * cs, * cst, * act;
  __device__ PgWork(double * base, size_t n)
  {
    x = base;
    xt = x + 3 * n;
    g = xt + 3 * n;
    p = g + 3 * n;
    r = p + 3 * n;
    z = r + 3 * n;
    hp = z + 3 * n;
    d = hp + 3 * n;
    hd = d + 3 * n;
    mi = hd + 6 * n;
    cs = mi + 6 * n;
    cst = cs + 2 * n;
    act = cst + 2 * n;
  }
};

// The frame of constraint c at the job's x, from the node cache.
__device__ __forceinline__ pg::Frame pg_frame(const PgWork & w, uint32_t a, uint32_t b)
{
  return pg::frame(w.cs[2 * static_cast<size_t>(a)], w.cs[2 * static_cast<size_t>(a) + 1], w.x + 3 * static_cast<size_t>(a),
                   w.x + 3 * static_cast<size_t>(b));
}

// A robust job's rho' per constraint, m doubles in front of its node arrays.  Written by
// pg_linearize (by the thread that meets the constraint as its begin node: one entry of node_con),
// read behind its closing barrier by pg_matvec and pg_chain_couplings.
__device__ __forceinline__ double * pg_weights(const PgGraph & G, const PgWork & w) { return w.x - G.m; }

// g, the diagonal blocks of H = J^T J and the active flags at x; returns |g|_inf.  Under a loss
// g = sum rho' J^T r and H = sum rho' J^T J: both ends of a constraint take rho' from their own r
// (the same operations on the same values: the same bits), the begin end keeps it.  A node that is
// fixed or has no enabled constraint is not active: its g and block are zero.
template <int kPrec, int kLoss>
__device__ double pg_linearize(const PgGraph & G, const uint8_t * en, const PgWork & w, PgScratch & sc, uint32_t & parity)
{
  double gmax = 0.0;
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    double gi[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t count = 0;
    const uint32_t k1 = G.node_ptr[i + 1];
    for (uint32_t k = G.node_ptr[i]; k < k1; ++k)
    {
      const uint32_t entry = G.node_con[k], c = entry >> 1;
      if (en != nullptr && en[c] == 0) continue;
      ++count;
      const uint32_t a = G.begin[c], b = G.end[c];
      const pg::Frame f = pg_frame(w, a, b);
      const double * W = G.W + 9 * static_cast<size_t>(c);
      double e[3], r[3], v[3], y[3], E[9];
      pg::error(f, w.x[3 * static_cast<size_t>(a) + 2], w.x[3 * static_cast<size_t>(b) + 2], G.transform + 3 * static_cast<size_t>(c), e);
      pg::mul(W, e, r);
      [[maybe_unused]] double rw = 1.0;
      if constexpr (kLoss != 0)
      {
        rw = PgLoss<kLoss>(G).weight(c, (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);   // (chi2 as pg_constraint forms it)
        if ((entry & 1u) == 0u) pg_weights(G, w)[c] = rw;
      }
      pg::mul_t(W, r, v);
      if (entry & 1u)
      {
        pg::apply_bt(f, v, y);
        pg::jacobian_b(f, E);
      }
      else
      {
        pg::apply_at(f, v, y);
        pg::jacobian_a(f, E);
      }
      if constexpr (kLoss == 0)
      {
        gi[0] += y[0];
        gi[1] += y[1];
        gi[2] += y[2];
        pg::add_jtj(W, E, S);
      }
      else
      {
        double T[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        pg::add_jtj(W, E, T);
        gi[0] += rw * y[0];
        gi[1] += rw * y[1];
        gi[2] += rw * y[2];
#pragma unroll
        for (int j = 0; j < 6; ++j) S[j] += rw * T[j];
      }
    }
    const bool active = count != 0u && i != G.fixed;
    const size_t at = static_cast<size_t>(i);
#pragma unroll
    for (int j = 0; j < 3; ++j) w.g[3 * at + j] = active ? gi[j] : 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) w.hd[6 * at + j] = active ? S[j] : 0.0;
    w.act[at] = active ? 1.0 : 0.0;
    if (active) gmax = fmax(gmax, fmax(fabs(gi[0]), fmax(fabs(gi[1]), fabs(gi[2]))));
  }
  return pg_block_max(gmax, sc, parity);
}

__device__ __forceinline__ double pg_clamp_diag(double v) { return fmin(fmax(v, kPgDiagMin), kPgDiagMax); }

// hp_i = ((H + lambda D) p)_i of the thread's nodes; returns the thread's share of p . hp.
template <int kPrec, int kLoss>
__device__ double pg_matvec(const PgGraph & G, const uint8_t * en, const PgWork & w, double lambda)
{
  double php = 0.0;
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
    double acc[3] = {0.0, 0.0, 0.0};
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
        double va[3], vb[3], v[3], u[3], t[3], y[3];
        pg::apply_a(f, w.p + 3 * static_cast<size_t>(a), va);
        pg::apply_b(f, w.p + 3 * static_cast<size_t>(b), vb);
        v[0] = va[0] + vb[0];
        v[1] = va[1] + vb[1];
        v[2] = va[2] + vb[2];
        pg::mul(W, v, u);
        pg::mul_t(W, u, t);
        if (entry & 1u) pg::apply_bt(f, t, y);
        else pg::apply_at(f, t, y);
        if constexpr (kLoss == 0)
        {
          acc[0] += y[0];
          acc[1] += y[1];
          acc[2] += y[2];
        }
        else
        {
          const double rw = pg_weights(G, w)[c];
          acc[0] += rw * y[0];
          acc[1] += rw * y[1];
          acc[2] += rw * y[2];
        }
      }
      const double * S = w.hd + 6 * at;
      const double * pi = w.p + 3 * at;
      acc[0] += lambda * pg_clamp_diag(S[0]) * pi[0];
      acc[1] += lambda * pg_clamp_diag(S[3]) * pi[1];
      acc[2] += lambda * pg_clamp_diag(S[5]) * pi[2];
      php += (pi[0] * acc[0] + pi[1] * acc[1]) + pi[2] * acc[2];
    }
    w.hp[3 * at] = acc[0];
    w.hp[3 * at + 1] = acc[1];
    w.hp[3 * at + 2] = acc[2];
  }
  return php;
}

// cos / sin of the headings of the thread's own nodes of xs into trig.  One body for the start and
// the trial point, in a loop of its own: the library's argument reduction is the largest register
// user of this file, and nothing else is live round it.
__device__ __forceinline__ void pg_trig(const double * xs, double * trig, uint32_t n)
{
  for (uint32_t i = pg_tid(); i < n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
    double sn, cs;
    sincos(xs[3 * at + 2], &sn, &cs);
    trig[2 * at] = cs;
    trig[2 * at + 1] = sn;
  }
}

// ---- the chain preconditioner: z = M^-1 r, M the block-tridiagonal band of H + lambda D over the
// nodes in node order (include/ndt2d_hip.h, "Pose graph"), by the block cyclic reduction of
// posegraph/ndt2d_posegraph_chain.h.  A node that is not active is a segment of its own with the
// identity as its block and zero couplings: its r is 0, so is its z.  At each level the q-th node
// of the level goes to thread q mod 1,024 (not to the node's owner), one barrier between levels. ----

// What "chain" adds to a job's workspace, behind PgWork's arrays.
struct PgChainWork
{
  double * od = nullptr, * b = nullptr;
  pg::chain::System m = {nullptr, nullptr, nullptr, nullptr};
  PgChainWork() = default;   // ("jacobi": an empty shell, nothing of it is used)
  __device__ PgChainWork(double * base, size_t n)
  {
    od = base;
    m.D = od + 9 * n;
    m.U = m.D + 6 * n;
    m.L = m.U + 9 * n;
    m.P = m.L + 9 * n;
    b = m.P + 6 * n;
  }
};

// H's blocks (i, i + 1) at x: each node over its own incident constraints, the enabled ones that
// join it and node i + 1 (either way round, duplicates too) in ascending constraint index, of
// (W E_i)^T (W E_{i+1}), under a loss each weighted by the constraint's rho': the band of the
// reweighted H.  Zero where either node is not active.  Behind pg_linearize (act, rho').
template <int kLoss>
__device__ void pg_chain_couplings(const PgGraph & G, const uint8_t * en, const PgWork & w, const PgChainWork & ch)
{
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (w.act[at] != 0.0 && i + 1u < G.n && i + 1u != G.fixed)
    {
      const uint32_t k1 = G.node_ptr[i + 1];
      for (uint32_t k = G.node_ptr[i]; k < k1; ++k)
      {
        const uint32_t entry = G.node_con[k], c = entry >> 1;
        if (en != nullptr && en[c] == 0) continue;
        const uint32_t a = G.begin[c], b = G.end[c];
        if (((entry & 1u) ? a : b) != i + 1u) continue;
        const pg::Frame f = pg_frame(w, a, b);
        const double * W = G.W + 9 * static_cast<size_t>(c);
        double Ei[9], En[9], Ji[9], Jn[9], X[9];
        if (entry & 1u)
        {
          pg::jacobian_b(f, Ei);
          pg::jacobian_a(f, En);
        }
        else
        {
          pg::jacobian_a(f, Ei);
          pg::jacobian_b(f, En);
        }
        pg::chain::mm(W, Ei, Ji);
        pg::chain::mm(W, En, Jn);
        pg::chain::mtm(Ji, Jn, X);
#pragma unroll
        for (int j = 0; j < 9; ++j)
        {
          if constexpr (kLoss == 0) S[j] += X[j];
          else S[j] += pg_weights(G, w)[c] * X[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) ch.od[9 * at + j] = S[j];
  }
}

// Factors M at lambda: the blocks in (each thread its own nodes), the levels, the root.  Returns
// whether every pivot was positive definite, the same in every thread.
// ([[maybe_unused]], here and on pg_chain_apply: the two that are neither templates nor inline, in a
// header that a unit without a kernel, posegraph/ndt2d_posegraph_robust.hip, takes with the object.)
[[maybe_unused]] __device__ bool pg_chain_factor(const PgGraph & G, const PgWork & w, const PgChainWork & ch, double lambda, PgScratch & sc,
                                                 uint32_t & parity)
{
  const size_t n = G.n;
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
    double S[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (w.act[at] != 0.0)
    {
#pragma unroll
      for (int j = 0; j < 6; ++j) S[j] = w.hd[6 * at + j];
      S[0] += lambda * pg_clamp_diag(S[0]);
      S[3] += lambda * pg_clamp_diag(S[3]);
      S[5] += lambda * pg_clamp_diag(S[5]);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) ch.m.D[6 * at + j] = S[j];
#pragma unroll
    for (int j = 0; j < 9; ++j) ch.m.U[9 * at + j] = ch.od[9 * at + j];
  }
  __syncthreads();
  double bad = 0.0;
  for (size_t s = 1; s < n; s <<= 1)
  {
    const size_t count = pg::chain::stay_count(n, s);
    for (size_t q = pg_tid(); q < count; q += kPgThreads)
    {
      if (!pg::chain::factor_node(ch.m, n, pg::chain::stay_node(s, q), s)) bad = 1.0;
    }
    __syncthreads();
  }
  if (pg_tid() == 0u && !pg::chain::factor_root(ch.m)) bad = 1.0;
  return pg_block_max(bad, sc, parity) == 0.0;   // (its barrier also orders the root's pivot)
}

// z = M^-1 b by the factors; ch.b holds the right-hand side (written by the nodes' owners, no
// barrier behind it yet) and is reduced in place.  Ends behind a barrier: z is whole.
[[maybe_unused]] __device__ void pg_chain_apply(const PgGraph & G, const PgWork & w, const PgChainWork & ch)
{
  const size_t n = G.n;
  __syncthreads();
  for (size_t s = 1; s < n; s <<= 1)
  {
    const size_t count = pg::chain::stay_count(n, s);
    for (size_t q = pg_tid(); q < count; q += kPgThreads) pg::chain::forward_node(ch.m, ch.b, n, pg::chain::stay_node(s, q), s);
    __syncthreads();
  }
  if (pg_tid() == 0u) pg::chain::back_root(ch.m, ch.b, w.z);
  __syncthreads();
  for (size_t s = pg::chain::top_stride(n); s >= 1; s >>= 1)
  {
    const size_t count = pg::chain::gone_count(n, s);
    for (size_t q = pg_tid(); q < count; q += kPgThreads) pg::chain::back_node(ch.m, ch.b, w.z, n, pg::chain::gone_node(s, q), s);
    __syncthreads();
  }
}

// The thread's share of r . z behind pg_chain_apply; kFirst: p = z, the CG's first direction.
template <bool kFirst>
__device__ double pg_chain_rz(const PgGraph & G, const PgWork & w)
{
  double rz = 0.0;
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
    const double * r = w.r + 3 * at, * z = w.z + 3 * at;
    if constexpr (kFirst)
    {
#pragma unroll
      for (int j = 0; j < 3; ++j) w.p[3 * at + j] = z[j];
    }
    rz += (r[0] * z[0] + r[1] * z[1]) + r[2] * z[2];
  }
  return rz;
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_KERNEL_H_
