// Pose-graph optimisation on the device: N poses (x, y, theta), M relative-pose constraints, one
// pose held fixed, and K independent jobs over the one graph, each with its own mask of enabled
// constraints -- Levenberg-Marquardt with a matrix-free, block-Jacobi preconditioned conjugate
// gradient inside, the whole iteration in ONE kernel launch (gfx950 / MI355X).  The residual, the
// weighting, the cost, the stop rules and the records are the contract of include/ndt2d_hip.h
// ("Pose graph"); the arithmetic of a constraint is posegraph/ndt2d_posegraph_fn.h.
//
//   posegraph_solve_kernel     grid (job of the chunk), 1,024 threads: one workgroup per job.  Thread
//       t owns nodes t, t + 1024, ... in every phase and constraints t, t + 1024, ... of the cost.
//       The graph (start poses, constraints with W, the node -> constraint table) lies in HBM and is
//       shared by the jobs; a job's vectors (x, trial x, g, p, r, z, Hp, delta, the diagonal blocks
//       of H, the preconditioner's inverses, cos / sin per node) lie in its own workspace in HBM.
//       The LM loop, the gain ratio, accept / reject and the stop rules are evaluated by every
//       thread on the same reduced values: all control flow is uniform, __syncthreads the only
//       barrier, and the host is not asked between iterations.  A template on the preconditioner:
//       kPgJacobi, each node's 3 x 3 block (the default, the code it was), or kPgChain, the
//       block-tridiagonal band along the node order by block cyclic reduction
//       (posegraph/ndt2d_posegraph_chain.h; pg_chain_* below), chosen per object.  A second template
//       argument is the loss (posegraph/ndt2d_posegraph_loss.h): kLoss = 0, none -- the code as it
//       was, bit for bit -- or Huber or Cauchy on chosen constraints: F sums rho(chi2), and g, the
//       blocks of H, the matrix-vector product and the chain's couplings carry rho' per constraint,
//       taken at the accepted point by pg_linearize and kept in the job's workspace (PgLoss,
//       pg_weights below).
//   posegraph_evaluate_kernel  grid (job), 1,024 threads: e, r = W e and chi2 = |r|^2 of every
//       constraint at the job's poses (thread t: constraints t, t + 1024, ...), F = 1/2 sum chi2
//       over the enabled ones by the same reduction the solver uses -- a solve's initial_cost is
//       evaluate's F bit for bit.  The same template argument kLoss: F then sums rho(chi2).
//
//   marginals_linearize_kernel, marginals_columns_kernel   block columns of the inverse of H at given
//       poses ("Marginal covariances"): a job's linearisation and preconditioner once, then a
//       workgroup per (job, query node) whose three columns run one CG loop in lockstep.  Their
//       heads, behind the evaluate kernel, say the rest.
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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_host.h"
#include "posegraph/ndt2d_posegraph_fn.h"
#include "posegraph/ndt2d_posegraph_chain.h"
#include "posegraph/ndt2d_posegraph_loss.h"
#include "posegraph/ndt2d_posegraph_relative.h"

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
// coupling (9), the coupling (9) and the inverse pivot (6) kept at the node's elimination, the
// reduced right-hand side (3)
constexpr size_t kPgChainDoubles = 9 + 6 + 9 + 9 + 6 + 3;

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
__device__ bool pg_chain_factor(const PgGraph & G, const PgWork & w, const PgChainWork & ch, double lambda, PgScratch & sc, uint32_t & parity)
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
__device__ void pg_chain_apply(const PgGraph & G, const PgWork & w, const PgChainWork & ch)
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

template <int kPrec, int kLoss>
__global__ void __launch_bounds__(kPgThreads) posegraph_solve_kernel(const PgGraph G, const uint8_t * enabled, double * workspace,
                                                                      const PgRules rules, double * poses_out, double * records)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  const uint32_t tid = threadIdx.x;
  const size_t job = blockIdx.x, n = G.n;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  constexpr size_t per_node = kPrec == kPgChain ? kPgNodeDoubles + kPgChainDoubles : kPgNodeDoubles;
  // (a robust job: rho' of its m constraints, then the node arrays)
  double * const base = kLoss == 0 ? workspace + job * per_node * n : workspace + job * (per_node * n + G.m) + G.m;
  const PgWork w(base, n);
  const PgChainWork ch = kPrec == kPgChain ? PgChainWork(base + kPgNodeDoubles * n, n) : PgChainWork();
  bool chain = false;   // whether this LM iteration's CG applies the chain's factors (uniform)

  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
#pragma unroll
    for (int j = 0; j < 3; ++j) w.x[3 * at + j] = G.poses[3 * at + j];
  }
  pg_trig(w.x, w.cs, G.n);
  __syncthreads();

  double F = pg_cost<kPrec, kLoss>(G, en, w.x, w.cs, sc, parity);
  const double F0 = F;
  double gmax = 0.0;
  uint32_t status = NDT2D_POSEGRAPH_MAX_ITERATIONS, iterations = 0, cg_total = 0;
  const uint32_t cg_cap = G.n >= kPgCgCap ? kPgCgCap : min(3u * G.n + 16u, kPgCgCap);
  if (!isfinite(F))
  {
    status = NDT2D_POSEGRAPH_FAILED;
  }
  else
  {
    gmax = pg_linearize<kPrec, kLoss>(G, en, w, sc, parity);
    if constexpr (kPrec == kPgChain) pg_chain_couplings<kLoss>(G, en, w, ch);
    if (gmax <= rules.gradient_tolerance) status = NDT2D_POSEGRAPH_CONVERGED_GRADIENT;
  }
  double lambda = kPgLambda0, nu = 2.0, g_start = -1.0;

  while (status == NDT2D_POSEGRAPH_MAX_ITERATIONS && iterations < rules.max_iterations)
  {
    ++iterations;
    // ---- the step: (H + lambda D) delta = -g by preconditioned conjugate gradients from 0 ----
    // "chain": M is factored anew (lambda changes on accepted and on rejected steps); a pivot that is
    // not positive definite leaves this iteration to the Jacobi blocks below
    if constexpr (kPrec == kPgChain) chain = pg_chain_factor(G, w, ch, lambda, sc, parity);
    double s2[2] = {0.0, 0.0};
    for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
    {
      const size_t at = static_cast<size_t>(i);
      double S[6], M[6], r[3], z[3];
#pragma unroll
      for (int j = 0; j < 6; ++j) S[j] = w.hd[6 * at + j];
      S[0] += lambda * pg_clamp_diag(S[0]);
      S[3] += lambda * pg_clamp_diag(S[3]);
      S[5] += lambda * pg_clamp_diag(S[5]);
      if (w.act[at] == 0.0 || !pg::invert_sym(S, M))
      {
#pragma unroll
        for (int j = 0; j < 6; ++j) M[j] = 0.0;
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) w.mi[6 * at + j] = M[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) r[j] = -w.g[3 * at + j];
      pg::mul_sym(M, r, z);
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        w.r[3 * at + j] = r[j];
        w.z[3 * at + j] = z[j];
        w.p[3 * at + j] = z[j];
        w.d[3 * at + j] = 0.0;
      }
      if constexpr (kPrec == kPgChain)
      {
#pragma unroll
        for (int j = 0; j < 3; ++j) ch.b[3 * at + j] = r[j];
      }
      s2[0] += (r[0] * z[0] + r[1] * z[1]) + r[2] * z[2];
      s2[1] += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    }
    if constexpr (kPrec == kPgChain)
    {
      if (chain)
      {
        pg_chain_apply(G, w, ch);
        s2[0] = pg_chain_rz<true>(G, w);
      }
    }
    pg_block_sum(s2, sc, parity);
    double rz = s2[0];
    const double r_start = sqrt(s2[1]);
    if (g_start < 0.0) g_start = r_start;
    // the forcing term: loose far from the minimiser, tighter with the gradient (superlinear)
    const double target = fmin(0.1, sqrt(r_start / g_start)) * r_start;
    for (uint32_t k = 0; k < cg_cap; ++k)
    {
      double s1[1] = {pg_matvec<kPrec, kLoss>(G, en, w, lambda)};
      pg_block_sum(s1, sc, parity);
      if (!(s1[0] > 0.0) || !(rz > 0.0)) break;   // (p = 0, or a direction rounding made useless)
      const double alpha = rz / s1[0];
      s2[0] = 0.0;
      s2[1] = 0.0;
      for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
      {
        const size_t at = static_cast<size_t>(i);
        double r[3], z[3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
          w.d[3 * at + j] += alpha * w.p[3 * at + j];
          r[j] = w.r[3 * at + j] - alpha * w.hp[3 * at + j];
          w.r[3 * at + j] = r[j];
        }
        if constexpr (kPrec == kPgChain)
        {
          if (chain)   // (z comes from the factors, behind this loop)
          {
#pragma unroll
            for (int j = 0; j < 3; ++j) ch.b[3 * at + j] = r[j];
            s2[1] += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            continue;
          }
        }
        pg::mul_sym(w.mi + 6 * at, r, z);
#pragma unroll
        for (int j = 0; j < 3; ++j) w.z[3 * at + j] = z[j];
        s2[0] += (r[0] * z[0] + r[1] * z[1]) + r[2] * z[2];
        s2[1] += (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
      }
      if constexpr (kPrec == kPgChain)
      {
        if (chain)
        {
          pg_chain_apply(G, w, ch);
          s2[0] = pg_chain_rz<false>(G, w);
        }
      }
      pg_block_sum(s2, sc, parity);
      ++cg_total;
      if (sqrt(s2[1]) <= target) break;
      const double beta = s2[0] / rz;
      rz = s2[0];
      for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
      {
        const size_t at = static_cast<size_t>(i);
#pragma unroll
        for (int j = 0; j < 3; ++j) w.p[3 * at + j] = w.z[3 * at + j] + beta * w.p[3 * at + j];
      }
      __syncthreads();
    }

    // ---- the trial point and what the model says of it ----
    // with rho the CG residual left in r: delta^T H delta = -g.delta - lambda delta^T D delta - delta.r,
    // so the model's decrease -g.delta - 1/2 delta^T H delta = 1/2 (lambda delta^T D delta + delta.r - g.delta)
    double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
    {
      const size_t at = static_cast<size_t>(i);
      const double * S = w.hd + 6 * at;
      const double D[3] = {pg_clamp_diag(S[0]), pg_clamp_diag(S[3]), pg_clamp_diag(S[5])};
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        const double x = w.x[3 * at + j], d = w.d[3 * at + j];
        const double xt = d == 0.0 ? x : x + d;   // (a pose that does not move keeps its bits, -0.0 included)
        w.xt[3 * at + j] = xt;
        s5[0] += w.g[3 * at + j] * d;
        s5[1] += lambda * D[j] * d * d;
        s5[2] += d * w.r[3 * at + j];
        s5[3] += d * d;
        s5[4] += x * x;
      }
    }
    pg_trig(w.xt, w.cst, G.n);   // (each thread its own nodes: no barrier in between)
    pg_block_sum(s5, sc, parity);
    const double predicted = 0.5 * ((s5[1] + s5[2]) - s5[0]);
    const double step = sqrt(s5[3]), x_norm = sqrt(s5[4]);
    if (rules.parameter_tolerance > 0.0 && step <= rules.parameter_tolerance * (x_norm + rules.parameter_tolerance))
    {
      status = NDT2D_POSEGRAPH_CONVERGED_STEP;
      break;
    }
    const double Ft = pg_cost<kPrec, kLoss>(G, en, w.xt, w.cst, sc, parity);
    const double dF = F - Ft;
    // below the rounding of the cost's own sum the gain ratio is noise: the model decides
    const bool noise = fabs(dF) <= kPgNoise * F;
    const double gain = dF / predicted;
    if (isfinite(Ft) && predicted > 0.0 && (noise || gain > kPgMinGain))
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
      gmax = pg_linearize<kPrec, kLoss>(G, en, w, sc, parity);
      if constexpr (kPrec == kPgChain) pg_chain_couplings<kLoss>(G, en, w, ch);
      const double t = 2.0 * gain - 1.0;
      lambda *= noise ? 1.0 / 3.0 : fmax(1.0 / 3.0, 1.0 - t * t * t);
      lambda = fmin(fmax(lambda, kPgLambdaMin), kPgLambdaMax);
      nu = 2.0;
      const double F_before = F;
      F = Ft;
      if (gmax <= rules.gradient_tolerance) status = NDT2D_POSEGRAPH_CONVERGED_GRADIENT;
      else if (rules.function_tolerance > 0.0 && fabs(dF) <= rules.function_tolerance * F_before) status = NDT2D_POSEGRAPH_CONVERGED_COST;
    }
    else
    {
      lambda = fmin(lambda * nu, kPgLambdaMax);
      nu *= 2.0;
    }
  }

  // (FAILED: x still holds the start poses)
  for (uint32_t i = pg_tid(); i < G.n; i += kPgThreads)
  {
    const size_t at = static_cast<size_t>(i);
#pragma unroll
    for (int j = 0; j < 3; ++j) poses_out[(job * n + at) * 3 + j] = w.x[3 * at + j];
  }
  if (tid == 0)
  {
    double * rec = records + job * kPgRec;
    rec[0] = static_cast<double>(status);
    rec[1] = static_cast<double>(iterations);
    rec[2] = static_cast<double>(cg_total);
    rec[3] = F0;
    rec[4] = F;
    rec[5] = gmax;
  }
}

// poses: the job's at poses + job x pose_stride doubles (0: the graph's start poses for every job).
// Under a loss the cost sums rho(chi2); chi2 itself is written as it is.
template <int kLoss>
__global__ void __launch_bounds__(kPgThreads) posegraph_evaluate_kernel(const PgGraph G, const uint8_t * enabled, const double * poses,
                                                                         size_t pose_stride, double * cost, double * chi2, size_t chi2_stride,
                                                                         double * residuals)
{
  __shared__ PgScratch sc;
  uint32_t parity = 0;
  const size_t job = blockIdx.x;
  const uint8_t * en = enabled != nullptr ? enabled + job * G.m : nullptr;
  const double * xs = poses + job * pose_stride;
  double acc[1] = {0.0};
  for (uint32_t c = pg_tid(); c < G.m; c += kPgThreads)
  {
    double e[3], r[3];
    const double q = pg_constraint(G, c, xs, nullptr, e, r);
    if (chi2 != nullptr) chi2[job * chi2_stride + c] = q;
    if (residuals != nullptr)
    {
      double * out = residuals + (job * G.m + c) * 6;
#pragma unroll
      for (int j = 0; j < 3; ++j)
      {
        out[j] = e[j];
        out[3 + j] = r[j];
      }
    }
    if (en == nullptr || en[c] != 0)
    {
      if constexpr (kLoss == 0) acc[0] += q;
      else acc[0] += PgLoss<kLoss>(G).rho(c, q);
    }
  }
  pg_block_sum(acc, sc, parity);
  if (threadIdx.x == 0 && cost != nullptr) cost[job] = 0.5 * acc[0];
}

// ---- marginal covariances (include/ndt2d_hip.h, "Marginal covariances"): block columns of
// (H_FF + damping clamp(diag H_FF))^-1 at given poses, each column one preconditioned CG from 0 on
// the solver's own operator. ----

constexpr size_t kPgMargRec = NDT2D_MARGINALS_RECORD_DOUBLES;
constexpr size_t kPgMargDeviceRec = 9;   // what the columns kernel writes per pair: 3 x {status, iterations, |r|_2}
// pg_linearize's first template argument here: copies of its own, the solver's stay as they were
constexpr int kPgMarginals = 2;
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
  (void)pg_linearize<kPgMarginals + kPrec, kLoss>(G, en, w, sc, parity);
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

// z = M^-1 b of the live columns among three by the job's factors, the levels' barriers shared:
// pg_chain_apply's passes with each node's step taken once per live column -- the same operations per
// column in the same order, so the same bits as three applies.  B, Z: [column][node][3]; B is
// reduced in place.  Ends behind a barrier.  (Used by the measurement build only: see kPgApplyTogether.)
[[maybe_unused]] __device__ __forceinline__ void pg_chain_apply3(const PgGraph & G, const PgChainWork & ch, double * B, double * Z, const bool (&live)[3])
{
  const size_t n = G.n, n3 = 3 * n;
  __syncthreads();
  for (size_t s = 1; s < n; s <<= 1)
  {
    const size_t count = pg::chain::stay_count(n, s);
    for (size_t q = pg_tid(); q < count; q += kPgThreads)
    {
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (live[col]) pg::chain::forward_node(ch.m, B + col * n3, n, pg::chain::stay_node(s, q), s);
      }
    }
    __syncthreads();
  }
  if (pg_tid() == 0u)
  {
#pragma unroll
    for (int col = 0; col < 3; ++col)
    {
      if (live[col]) pg::chain::back_root(ch.m, B + col * n3, Z + col * n3);
    }
  }
  __syncthreads();
  for (size_t s = pg::chain::top_stride(n); s >= 1; s >>= 1)
  {
    const size_t count = pg::chain::gone_count(n, s);
    for (size_t q = pg_tid(); q < count; q += kPgThreads)
    {
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (live[col]) pg::chain::back_node(ch.m, B + col * n3, Z + col * n3, n, pg::chain::gone_node(s, q), s);
      }
    }
    __syncthreads();
  }
}

// Whether the columns kernel applies the chain's factors to its live columns in one pass
// (pg_chain_apply3) or column after column (pg_chain_apply): column after column, which measured
// 2 to 7 % faster where a workgroup has one column and within 2 % either way in lockstep from 256
// pairs on; the macro builds the other for that measurement.  The bits are the same.
#if defined(NDT2D_MARGINALS_APPLY_TOGETHER)
constexpr bool kPgApplyTogether = true;
#else
constexpr bool kPgApplyTogether = false;
#endif

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
      if constexpr (kPgApplyTogether) pg_chain_apply3(G, PgChainWork(base + kPgNodeDoubles * n, n), B, Z, live);
#pragma unroll
      for (int col = 0; col < 3; ++col)
      {
        if (!live[col]) continue;
        PgWork wc = w;
        wc.r = R + col * n3;
        wc.z = Z + col * n3;
        wc.p = P + col * n3;
        if constexpr (!kPgApplyTogether)
        {
          PgChainWork cc(base + kPgNodeDoubles * n, n);
          cc.b = B + col * n3;
          pg_chain_apply(G, wc, cc);
        }
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
        if constexpr (kPgApplyTogether) pg_chain_apply3(G, PgChainWork(base + kPgNodeDoubles * n, n), B, Z, live);
#pragma unroll
        for (int col = 0; col < 3; ++col)
        {
          if (!live[col]) continue;
          PgWork wc = w;
          wc.r = R + col * n3;
          wc.z = Z + col * n3;
          wc.p = P + col * n3;
          if constexpr (!kPgApplyTogether)
          {
            PgChainWork cc(base + kPgNodeDoubles * n, n);
            cc.b = B + col * n3;
            pg_chain_apply(G, wc, cc);
          }
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

}  // namespace

}  // namespace ndt2d

// ---- the object and the C entry points ----

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

PgGraph pg_device_graph(const ndt2d_posegraph * s)
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

// W of every constraint by the weighting in force, behind a change of either.
int pg_send_weights(ndt2d_posegraph * s, hipStream_t stream)
{
  if (s->weights_sent || s->m == 0) return NDT2D_OK;
  s->stage.resize(9 * s->m);
  for (size_t c = 0; c < s->m; ++c)
  {
    const double * L = s->chol.data() + 9 * c;
    double * W = s->stage.data() + 9 * c;
    for (int i = 0; i < 3; ++i)
    {
      for (int j = 0; j < 3; ++j) W[3 * i + j] = s->information_weighting ? L[3 * j + i] : L[3 * i + j];
    }
  }
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(static_cast<double *>(s->d_graph) + 3 * s->n + 3 * s->m, s->stage.data(), 9 * s->m * sizeof(double),
                                    hipMemcpyHostToDevice, stream));
  NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));   // (the stage is reused)
  s->weights_sent = true;
  return NDT2D_OK;
}

// The loss's scale and selection beside the graph (PgLoss), behind a change of either; nothing
// without a loss.
int pg_send_loss(ndt2d_posegraph * s, hipStream_t stream)
{
  if (s->loss == pg::kLossTrivial || s->loss_sent) return NDT2D_OK;
  const double scale[2] = {s->loss_scale, s->loss_scale * s->loss_scale};
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(static_cast<double *>(s->d_graph) + 3 * s->n + 12 * s->m, scale, sizeof(scale), hipMemcpyHostToDevice,
                                    stream));
  const std::vector<uint8_t> every(s->robust.empty() ? s->m : 0, uint8_t(1));
  const std::vector<uint8_t> & on = s->robust.empty() ? every : s->robust;
  if (s->m != 0)
  {
    NDT2D_BATCH_HIP(s, hipMemcpyAsync(static_cast<uint32_t *>(s->d_index) + s->index.size(), on.data(), s->m, hipMemcpyHostToDevice, stream));
  }
  NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));   // (both sources are locals)
  s->loss_sent = true;
  return NDT2D_OK;
}

// A job's workspace in doubles: the node arrays, the chain's where it is selected, rho' per
// constraint under a loss.
size_t pg_job_doubles(const ndt2d_posegraph * s)
{
  return (kPgNodeDoubles + (s->chain ? kPgChainDoubles : 0)) * s->n + (s->loss != pg::kLossTrivial ? s->m : 0);
}

template <int kLoss>
void pg_launch_evaluate(hipStream_t stream, uint32_t jobs, const PgGraph & G, const uint8_t * d_en, const double * poses, size_t pose_stride,
                        double * cost, double * chi2, size_t chi2_stride, double * residuals)
{
  hipLaunchKernelGGL(posegraph_evaluate_kernel<kLoss>, dim3(jobs), dim3(kPgThreads), 0, stream, G, d_en, poses, pose_stride, cost, chi2,
                     chi2_stride, residuals);
}

// The evaluate kernel of the object's loss.
void pg_evaluate(const ndt2d_posegraph * s, hipStream_t stream, uint32_t jobs, const PgGraph & G, const uint8_t * d_en, const double * poses,
                 size_t pose_stride, double * cost, double * chi2, size_t chi2_stride, double * residuals)
{
  if (s->loss == pg::kLossHuber) pg_launch_evaluate<pg::kLossHuber>(stream, jobs, G, d_en, poses, pose_stride, cost, chi2, chi2_stride, residuals);
  else if (s->loss == pg::kLossCauchy) pg_launch_evaluate<pg::kLossCauchy>(stream, jobs, G, d_en, poses, pose_stride, cost, chi2, chi2_stride, residuals);
  else pg_launch_evaluate<pg::kLossTrivial>(stream, jobs, G, d_en, poses, pose_stride, cost, chi2, chi2_stride, residuals);
}

template <int kLoss>
void pg_launch_solve(const ndt2d_posegraph * s, hipStream_t stream, uint32_t jobs, const PgGraph & G, const uint8_t * d_en, const PgRules & rules,
                     double * poses_out, double * records)
{
  double * work = static_cast<double *>(s->d_work);
  if (s->chain)
  {
    hipLaunchKernelGGL((posegraph_solve_kernel<kPgChain, kLoss>), dim3(jobs), dim3(kPgThreads), 0, stream, G, d_en, work, rules, poses_out, records);
  }
  else
  {
    hipLaunchKernelGGL((posegraph_solve_kernel<kPgJacobi, kLoss>), dim3(jobs), dim3(kPgThreads), 0, stream, G, d_en, work, rules, poses_out, records);
  }
}

// The solve kernel of the object's preconditioner and loss.
void pg_solve(const ndt2d_posegraph * s, hipStream_t stream, uint32_t jobs, const PgGraph & G, const uint8_t * d_en, const PgRules & rules,
              double * poses_out, double * records)
{
  if (s->loss == pg::kLossHuber) pg_launch_solve<pg::kLossHuber>(s, stream, jobs, G, d_en, rules, poses_out, records);
  else if (s->loss == pg::kLossCauchy) pg_launch_solve<pg::kLossCauchy>(s, stream, jobs, G, d_en, rules, poses_out, records);
  else pg_launch_solve<pg::kLossTrivial>(s, stream, jobs, G, d_en, rules, poses_out, records);
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

template <int kPrec, int kLoss>
void pg_launch_marginals(hipStream_t stream, const PgGraph & G, const PgMarginalsLaunch & a)
{
  hipLaunchKernelGGL((marginals_linearize_kernel<kPrec, kLoss>), dim3(a.jobs), dim3(kPgThreads), 0, stream, G, a.d_en, a.poses, a.pose_stride,
                     a.blocks, a.block_doubles, a.damping);
  if (a.columns == 1)
  {
    hipLaunchKernelGGL((marginals_columns_kernel<kPrec, kLoss, 1>), dim3(3 * a.pairs), dim3(kPgThreads), 0, stream, G, a.d_en, a.blocks,
                       a.block_doubles, a.workspace, a.nodes, a.n_nodes, a.first_pair, a.first_job, a.damping, a.tolerance, a.cg_cap, a.blocks_out,
                       a.columns_out, a.records);
  }
  else
  {
    hipLaunchKernelGGL((marginals_columns_kernel<kPrec, kLoss, 3>), dim3(a.pairs), dim3(kPgThreads), 0, stream, G, a.d_en, a.blocks,
                       a.block_doubles, a.workspace, a.nodes, a.n_nodes, a.first_pair, a.first_job, a.damping, a.tolerance, a.cg_cap, a.blocks_out,
                       a.columns_out, a.records);
  }
}

template <int kLoss>
void pg_launch_marginals(const ndt2d_posegraph * s, hipStream_t stream, const PgGraph & G, const PgMarginalsLaunch & a)
{
  if (s->chain) pg_launch_marginals<kPgChain, kLoss>(stream, G, a);
  else pg_launch_marginals<kPgJacobi, kLoss>(stream, G, a);
}

// The marginals kernels of the object's preconditioner and loss.
void pg_marginals(const ndt2d_posegraph * s, hipStream_t stream, const PgGraph & G, const PgMarginalsLaunch & a)
{
  if (s->loss == pg::kLossHuber) pg_launch_marginals<pg::kLossHuber>(s, stream, G, a);
  else if (s->loss == pg::kLossCauchy) pg_launch_marginals<pg::kLossCauchy>(s, stream, G, a);
  else pg_launch_marginals<pg::kLossTrivial>(s, stream, G, a);
}

// The masks of jobs [k0, k1) on the device, or NULL for none.
int pg_send_masks(ndt2d_posegraph * s, hipStream_t stream, const uint8_t * enabled, size_t k0, size_t k1, const uint8_t ** out)
{
  *out = nullptr;
  if (enabled == nullptr || s->m == 0) return NDT2D_OK;
  const size_t bytes = (k1 - k0) * s->m;
  NDT2D_BATCH_HIP(s, grow_device(&s->d_enabled, &s->enabled_cap, bytes));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_enabled, enabled + k0 * s->m, bytes, hipMemcpyHostToDevice, stream));
  *out = static_cast<const uint8_t *>(s->d_enabled);
  return NDT2D_OK;
}

constexpr const char * kPgLossNames[3] = {"trivial", "huber", "cauchy"};

// kLoss* of a loss's name, -1 for none.
int pg_loss_kind(const char * kind)
{
  for (int k = 0; k < 3; ++k)
  {
    if (kind != nullptr && std::strcmp(kind, kPgLossNames[k]) == 0) return k;
  }
  return -1;
}

int pg_ready(ndt2d_posegraph * s, const char * who)
{
  if (!s->has_graph) return batch_fail(s, NDT2D_ERR_STATE, std::string(who) + ": no graph (ndt2d_posegraph_set_graph)");
  return NDT2D_OK;
}

}  // namespace

}  // namespace ndt2d

using ndt2d::batch_fail;

extern "C" {

int ndt2d_posegraph_create(ndt2d_handle h, size_t max_nodes, size_t max_constraints, size_t max_jobs, ndt2d_posegraph ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || max_nodes == 0 || max_nodes > ndt2d::kPgMaxNodes || max_constraints > ndt2d::kPgMaxConstraints || max_jobs == 0 ||
      max_jobs > ndt2d::kPgMaxJobs)
  {
    return NDT2D_ERR_INVALID;
  }
  ndt2d_posegraph * s = new ndt2d_posegraph();
  s->h = h;
  s->device = ndt2d_device_id(h);
  s->max_nodes = max_nodes;
  s->max_constraints = max_constraints;
  s->max_jobs = max_jobs;
  *out = s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_posegraph_destroy(ndt2d_posegraph * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  ndt2d::batch_drain(s);
  ndt2d::batch_release(s);
  for (void * p : {s->d_graph, s->d_index, s->d_enabled, s->d_work, s->d_marginals, s->d_marginal_poses, s->d_marginal_nodes})
  {
    if (p != nullptr) (void)hipFree(p);
  }
  delete s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_posegraph_last_error(ndt2d_posegraph * s)
{
  return s != nullptr ? s->err.c_str() : "null posegraph";
}

int ndt2d_posegraph_set_timing(ndt2d_posegraph * s, int enabled)
{
  NDT2D_C_TRY
  return ndt2d::batch_set_timing(s, enabled);
  NDT2D_C_CATCH(s)
}

int ndt2d_posegraph_last_ms(ndt2d_posegraph * s, float * kernel_ms, float * fetch_ms)
{
  NDT2D_C_TRY
  return ndt2d::batch_last_ms(s, "posegraph", kernel_ms, fetch_ms);
  NDT2D_C_CATCH(s)
}

int ndt2d_posegraph_set_weighting(ndt2d_posegraph * s, const char * weighting)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const std::string name = weighting != nullptr ? weighting : "";
  if (name != "reference" && name != "information")
  {
    return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_posegraph_set_weighting: \"" + name + "\" (\"reference\" or \"information\")");
  }
  const bool information = name == "information";
  if (information != s->information_weighting) s->weights_sent = false;
  s->information_weighting = information;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

const char * ndt2d_posegraph_weighting(ndt2d_posegraph * s)
{
  return s == nullptr ? "" : s->information_weighting ? "information" : "reference";
}

int ndt2d_pose_graph_set_preconditioner(ndt2d_posegraph * s, const char * preconditioner)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const std::string name = preconditioner != nullptr ? preconditioner : "";
  if (name != "jacobi" && name != "chain")
  {
    return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_pose_graph_set_preconditioner: \"" + name + "\" (\"jacobi\" or \"chain\")");
  }
  s->chain = name == "chain";
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

const char * ndt2d_pose_graph_preconditioner(ndt2d_posegraph * s)
{
  return s == nullptr ? "" : s->chain ? "chain" : "jacobi";
}

// ---- robust losses (include/ndt2d_hip.h, "Robust losses") ----

int ndt2d_robust_rho(const char * kind, double scale, double s, double * rho3_out)
{
  NDT2D_C_TRY
  const int loss = ndt2d::pg_loss_kind(kind);
  if (rho3_out == nullptr || loss < 0 || !(scale > 0.0) || !std::isfinite(scale) || !(s >= 0.0) || !std::isfinite(s)) return NDT2D_ERR_INVALID;
  return ndt2d::posegraph::loss_evaluate(loss, scale, s, rho3_out) ? NDT2D_OK : NDT2D_ERR_INVALID;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_robust_set_loss(ndt2d_posegraph * s, const char * kind, double scale)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const int loss = ndt2d::pg_loss_kind(kind);
  if (loss < 0)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, std::string("ndt2d_robust_set_loss: \"") + (kind != nullptr ? kind : "") +
                                              "\" (\"trivial\", \"huber\" or \"cauchy\")");
  }
  if (loss != ndt2d::posegraph::kLossTrivial)
  {
    if (!(scale > 0.0) || !std::isfinite(scale)) return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_robust_set_loss: the scale is not finite and > 0");
    if (scale != s->loss_scale) s->loss_sent = false;
    s->loss_scale = scale;
  }
  s->loss = loss;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

const char * ndt2d_robust_loss(ndt2d_posegraph * s, double * scale_out)
{
  if (s != nullptr && scale_out != nullptr) *scale_out = s->loss_scale;
  return s == nullptr ? "" : ndt2d::kPgLossNames[s->loss];
}

int ndt2d_robust_select(ndt2d_posegraph * s, const uint8_t * robust, size_t m)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const int rc = ndt2d::pg_ready(s, "ndt2d_robust_select");
  if (rc != NDT2D_OK) return rc;
  if (robust == nullptr)
  {
    s->robust.clear();
  }
  else
  {
    if (m != s->m)
    {
      return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_robust_select: " + std::to_string(m) + " bytes, the graph has " + std::to_string(s->m) +
                                                " constraints");
    }
    s->robust.assign(robust, robust + m);
    if (m == 0) s->robust.clear();
  }
  s->loss_sent = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_posegraph_set_graph(ndt2d_posegraph * s, const double * poses_xyt, size_t n, const uint32_t * begin, const uint32_t * end,
                              const double * transform, const double * information, size_t m, size_t fixed)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const std::string who = "ndt2d_posegraph_set_graph: ";
  if (n == 0) return batch_fail(s, NDT2D_ERR_INVALID, who + "no poses");
  if (poses_xyt == nullptr || (m != 0 && (begin == nullptr || end == nullptr || transform == nullptr || information == nullptr)))
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + "null argument");
  }
  if (n > s->max_nodes)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + std::to_string(n) + " poses, the capacity is " + std::to_string(s->max_nodes));
  }
  if (m > s->max_constraints)
  {
    return batch_fail(s, NDT2D_ERR_INVALID, who + std::to_string(m) + " constraints, the capacity is " + std::to_string(s->max_constraints));
  }
  if (fixed >= n) return batch_fail(s, NDT2D_ERR_INVALID, who + "fixed pose " + std::to_string(fixed) + " of " + std::to_string(n));
  for (size_t i = 0; i < 3 * n; ++i)
  {
    if (!std::isfinite(poses_xyt[i])) return batch_fail(s, NDT2D_ERR_INVALID, who + "pose " + std::to_string(i / 3) + " is not finite");
  }
  // every constraint is checked before the object changes: a refused graph leaves the old one in place
  std::vector<double> chol(9 * m);
  for (size_t c = 0; c < m; ++c)
  {
    const std::string name = "constraint " + std::to_string(c);
    if (begin[c] >= n || end[c] >= n)
    {
      return batch_fail(s, NDT2D_ERR_INVALID, who + name + " names pose " + std::to_string(begin[c] >= n ? begin[c] : end[c]) + " of " +
                                                std::to_string(n));
    }
    if (begin[c] == end[c]) return batch_fail(s, NDT2D_ERR_INVALID, who + name + " begins and ends at pose " + std::to_string(begin[c]));
    for (int j = 0; j < 3; ++j)
    {
      if (!std::isfinite(transform[3 * c + j])) return batch_fail(s, NDT2D_ERR_INVALID, who + name + ": its transform is not finite");
    }
    for (int j = 0; j < 9; ++j)
    {
      if (!std::isfinite(information[9 * c + j])) return batch_fail(s, NDT2D_ERR_INVALID, who + name + ": its information is not finite");
    }
    if (!ndt2d::posegraph::cholesky_lower(information + 9 * c, chol.data() + 9 * c))
    {
      return batch_fail(s, NDT2D_ERR_INVALID, who + name + ": its information is not symmetric positive definite");
    }
  }
  NDT2D_BATCH_HIP(s, hipSetDevice(s->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));
  s->has_graph = false;
  // the node -> constraint table: a node's constraints in ascending constraint index
  s->index.assign(2 * m + n + 1 + 2 * m, 0u);
  uint32_t * u_begin = s->index.data(), * u_end = u_begin + m, * ptr = u_end + m, * con = ptr + n + 1;
  for (size_t c = 0; c < m; ++c)
  {
    u_begin[c] = begin[c];
    u_end[c] = end[c];
    ++ptr[begin[c] + 1];
    ++ptr[end[c] + 1];
  }
  for (size_t i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
  {
    std::vector<uint32_t> fill(ptr, ptr + n);
    for (size_t c = 0; c < m; ++c)
    {
      con[fill[begin[c]]++] = static_cast<uint32_t>(c << 1);
      con[fill[end[c]]++] = static_cast<uint32_t>(c << 1) | 1u;
    }
  }
  s->stage.resize(3 * n + 3 * m);
  std::memcpy(s->stage.data(), poses_xyt, 3 * n * sizeof(double));
  if (m != 0) std::memcpy(s->stage.data() + 3 * n, transform, 3 * m * sizeof(double));
  // (with room for a loss's scale and selection: PgLoss)
  NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_graph, &s->graph_cap, (3 * n + 12 * m + 2) * sizeof(double)));
  NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_index, &s->index_cap, s->index.size() * sizeof(uint32_t) + m));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_graph, s->stage.data(), s->stage.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_index, s->index.data(), s->index.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
  s->chol.swap(chol);
  s->n = n;
  s->m = m;
  s->fixed = fixed;
  s->weights_sent = false;
  s->robust.clear();
  s->loss_sent = false;
  s->has_graph = true;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_posegraph_evaluate(ndt2d_posegraph * s, const uint8_t * enabled, size_t n_jobs, double * cost_out, double * chi2_out,
                             double * residuals_out)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  if (cost_out == nullptr) return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_posegraph_evaluate: null argument");
  int rc = ndt2d::pg_ready(s, "ndt2d_posegraph_evaluate");
  if (rc != NDT2D_OK) return rc;
  NDT2D_BATCH_HIP(s, hipSetDevice(s->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));
  rc = ndt2d::pg_send_weights(s, stream);
  if (rc != NDT2D_OK) return rc;
  rc = ndt2d::pg_send_loss(s, stream);
  if (rc != NDT2D_OK) return rc;
  const ndt2d::PgGraph G = ndt2d::pg_device_graph(s);
  const size_t m = s->m;
  for (size_t k0 = 0; k0 < n_jobs; k0 += s->max_jobs)
  {
    const size_t k1 = std::min(n_jobs, k0 + s->max_jobs), kc = k1 - k0;
    const uint8_t * d_en = nullptr;
    rc = ndt2d::pg_send_masks(s, stream, enabled, k0, k1, &d_en);
    if (rc != NDT2D_OK) return rc;
    // what comes back: [cost kc | chi2 kc m | residuals kc m 6]
    const size_t at_chi2 = kc, at_res = at_chi2 + (chi2_out != nullptr ? kc * m : 0);
    const size_t total = at_res + (residuals_out != nullptr ? kc * m * 6 : 0);
    NDT2D_BATCH_HIP(s, ndt2d::grow_pair(&s->h_out, &s->d_out, &s->out_cap, total));
    s->timed = false;
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[0], stream));
    ndt2d::pg_evaluate(s, stream, static_cast<uint32_t>(kc), G, d_en, G.poses, size_t(0), s->d_out,
                       chi2_out != nullptr ? s->d_out + at_chi2 : nullptr, m, residuals_out != nullptr ? s->d_out + at_res : nullptr);
    NDT2D_BATCH_HIP(s, hipGetLastError());
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[1], stream));
    NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, total * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[2], stream));
    NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
    s->timed = s->timing;
    std::memcpy(cost_out + k0, s->h_out, kc * sizeof(double));
    if (chi2_out != nullptr && m != 0) std::memcpy(chi2_out + k0 * m, s->h_out + at_chi2, kc * m * sizeof(double));
    if (residuals_out != nullptr && m != 0) std::memcpy(residuals_out + k0 * m * 6, s->h_out + at_res, kc * m * 6 * sizeof(double));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_posegraph_solve(ndt2d_posegraph * s, const uint8_t * enabled, size_t n_jobs, uint32_t max_iterations, double gradient_tolerance,
                          double function_tolerance, double parameter_tolerance, double * poses_out, double * records_out,
                          double * chi2_out)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0) return NDT2D_OK;
  if (poses_out == nullptr || records_out == nullptr) return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_posegraph_solve: null argument");
  if (!(gradient_tolerance >= 0.0) || !(function_tolerance >= 0.0) || !(parameter_tolerance >= 0.0) || !std::isfinite(gradient_tolerance) ||
      !std::isfinite(function_tolerance) || !std::isfinite(parameter_tolerance))
  {
    return batch_fail(s, NDT2D_ERR_INVALID, "ndt2d_posegraph_solve: a tolerance is negative or not finite");
  }
  int rc = ndt2d::pg_ready(s, "ndt2d_posegraph_solve");
  if (rc != NDT2D_OK) return rc;
  NDT2D_BATCH_HIP(s, hipSetDevice(s->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));
  rc = ndt2d::pg_send_weights(s, stream);
  if (rc != NDT2D_OK) return rc;
  rc = ndt2d::pg_send_loss(s, stream);
  if (rc != NDT2D_OK) return rc;
  const ndt2d::PgGraph G = ndt2d::pg_device_graph(s);
  const ndt2d::PgRules rules{max_iterations, gradient_tolerance, function_tolerance, parameter_tolerance};
  const size_t n = s->n, m = s->m;
  for (size_t k0 = 0; k0 < n_jobs; k0 += s->max_jobs)
  {
    const size_t k1 = std::min(n_jobs, k0 + s->max_jobs), kc = k1 - k0;
    const uint8_t * d_en = nullptr;
    rc = ndt2d::pg_send_masks(s, stream, enabled, k0, k1, &d_en);
    if (rc != NDT2D_OK) return rc;
    // (the chain's arrays and a loss's weights are paid for only where they are selected)
    NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_work, &s->work_cap, kc * ndt2d::pg_job_doubles(s) * sizeof(double)));
    // what comes back: [poses kc n 3 | records kc 6 | chi2 kc 2 m (start, end)]
    const size_t at_rec = kc * n * 3, at_chi2 = at_rec + kc * ndt2d::kPgRec;
    const size_t total = at_chi2 + (chi2_out != nullptr ? kc * 2 * m : 0);
    NDT2D_BATCH_HIP(s, ndt2d::grow_pair(&s->h_out, &s->d_out, &s->out_cap, total));
    s->timed = false;
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[0], stream));
    const uint32_t blocks = static_cast<uint32_t>(kc);
    if (chi2_out != nullptr)
    {
      ndt2d::pg_evaluate(s, stream, blocks, G, d_en, G.poses, size_t(0), nullptr, s->d_out + at_chi2, 2 * m, nullptr);
      NDT2D_BATCH_HIP(s, hipGetLastError());
    }
    ndt2d::pg_solve(s, stream, blocks, G, d_en, rules, s->d_out, s->d_out + at_rec);
    NDT2D_BATCH_HIP(s, hipGetLastError());
    if (chi2_out != nullptr)
    {
      ndt2d::pg_evaluate(s, stream, blocks, G, d_en, s->d_out, 3 * n, nullptr, s->d_out + at_chi2 + m, 2 * m, nullptr);
      NDT2D_BATCH_HIP(s, hipGetLastError());
    }
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[1], stream));
    NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, total * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[2], stream));
    NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
    s->timed = s->timing;
    std::memcpy(poses_out + k0 * n * 3, s->h_out, kc * n * 3 * sizeof(double));
    std::memcpy(records_out + k0 * ndt2d::kPgRec, s->h_out + at_rec, kc * ndt2d::kPgRec * sizeof(double));
    if (chi2_out != nullptr && m != 0) std::memcpy(chi2_out + k0 * 2 * m, s->h_out + at_chi2, kc * 2 * m * sizeof(double));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

// ---- marginal covariances (include/ndt2d_hip.h, "Marginal covariances") ----

int ndt2d_marginals_columns(ndt2d_posegraph * s, const uint8_t * enabled, size_t n_jobs, const double * poses, const uint32_t * nodes,
                            size_t n_nodes, double damping, double tolerance, uint32_t max_cg_iterations, double * blocks_out,
                            double * columns_out, double * records_out)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_jobs == 0 || n_nodes == 0) return NDT2D_OK;
  const std::string who = "ndt2d_marginals_columns: ";
  if (nodes == nullptr || blocks_out == nullptr || records_out == nullptr) return batch_fail(s, NDT2D_ERR_INVALID, who + "null argument");
  if (!(damping >= 0.0) || !std::isfinite(damping)) return batch_fail(s, NDT2D_ERR_INVALID, who + "the damping is negative or not finite");
  if (!(tolerance > 0.0) || !std::isfinite(tolerance)) return batch_fail(s, NDT2D_ERR_INVALID, who + "the tolerance is not finite and > 0");
  int rc = ndt2d::pg_ready(s, "ndt2d_marginals_columns");
  if (rc != NDT2D_OK) return rc;
  const size_t n = s->n, Q = n_nodes;
  if (Q > 0xFFFFFFFFu) return batch_fail(s, NDT2D_ERR_INVALID, who + "more than 2^32 - 1 query nodes");
  for (size_t q = 0; q < Q; ++q)
  {
    if (nodes[q] >= n) return batch_fail(s, NDT2D_ERR_INVALID, who + "query " + std::to_string(q) + " names node " + std::to_string(nodes[q]) +
                                                                 " of " + std::to_string(n));
  }
  if (poses != nullptr)
  {
    for (size_t i = 0; i < n_jobs * n * 3; ++i)
    {
      if (!std::isfinite(poses[i]))
      {
        return batch_fail(s, NDT2D_ERR_INVALID, who + "job " + std::to_string(i / (3 * n)) + " pose " + std::to_string(i / 3 % n) + " is not finite");
      }
    }
  }
  NDT2D_BATCH_HIP(s, hipSetDevice(s->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));
  rc = ndt2d::pg_send_weights(s, stream);
  if (rc != NDT2D_OK) return rc;
  rc = ndt2d::pg_send_loss(s, stream);
  if (rc != NDT2D_OK) return rc;
  const ndt2d::PgGraph G = ndt2d::pg_device_graph(s);
  NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_marginal_nodes, &s->marginal_nodes_cap, Q * sizeof(uint32_t)));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_marginal_nodes, nodes, Q * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  ndt2d::PgMarginalsLaunch a{};
  a.nodes = static_cast<const uint32_t *>(s->d_marginal_nodes);
  a.n_nodes = static_cast<uint32_t>(Q);
  a.damping = damping;
  a.tolerance = tolerance;
  a.cg_cap = max_cg_iterations != 0 ? max_cg_iterations
                                    : n >= ndt2d::kPgCgCap ? ndt2d::kPgCgCap : std::min(3u * static_cast<uint32_t>(n) + 16u, ndt2d::kPgCgCap);
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
    if (poses != nullptr)
    {
      NDT2D_BATCH_HIP(s, ndt2d::grow_device(&s->d_marginal_poses, &s->marginal_poses_cap, kc * n * 3 * sizeof(double)));
      NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->d_marginal_poses, poses + k0 * n * 3, kc * n * 3 * sizeof(double), hipMemcpyHostToDevice, stream));
      a.poses = static_cast<const double *>(s->d_marginal_poses);
      a.pose_stride = 3 * n;
    }
    else
    {
      a.poses = G.poses;
      a.pose_stride = 0;
    }
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
    s->timed = false;
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[0], stream));
    ndt2d::pg_marginals(s, stream, G, a);
    NDT2D_BATCH_HIP(s, hipGetLastError());
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[1], stream));
    NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, total * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[2], stream));
    NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
    s->timed = s->timing;
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
