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
//       (posegraph/ndt2d_posegraph_chain.h; pg_chain_* of the kernel header), chosen per object.  A
//       second template argument is the loss (posegraph/ndt2d_posegraph_loss.h): kLoss = 0, none --
//       the code as it was, bit for bit -- or Huber or Cauchy on chosen constraints: F sums
//       rho(chi2), and g, the blocks of H, the matrix-vector product and the chain's couplings carry
//       rho' per constraint, taken at the accepted point by pg_linearize and kept in the job's
//       workspace (PgLoss, pg_weights).
//   posegraph_evaluate_kernel  grid (job), 1,024 threads: e, r = W e and chi2 = |r|^2 of every
//       constraint at the job's poses (thread t: constraints t, t + 1024, ...), F = 1/2 sum chi2
//       over the enabled ones by the same reduction the solver uses -- a solve's initial_cost is
//       evaluate's F bit for bit.  The same template argument kLoss: F then sums rho(chi2).
//
// What the kernels are made of -- the graph and a job's workspace as they see them, the reductions,
// the linearisation, the matrix-vector product, the chain's passes -- is
// posegraph/ndt2d_posegraph_kernel.h, with the contract of determinism, bounds and LDS that holds for
// every kernel built from it; the object and the host helpers shared with the units beside this one
// (posegraph/ndt2d_posegraph_robust.hip: the losses' entry points; posegraph/ndt2d_posegraph_marginals.hip:
// the marginal covariances) are posegraph/ndt2d_posegraph_state.h, with the prelude a call begins
// with (pg_begin_call); what the calls refuse about their arguments is
// posegraph/ndt2d_posegraph_args.h.  Here: the two kernels, the object's life, the graph's upload,
// evaluate and solve.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "batch/ndt2d_batch_state.h"
#include "posegraph/ndt2d_posegraph_args.h"
#include "posegraph/ndt2d_posegraph_fn.h"
#include "posegraph/ndt2d_posegraph_loss.h"
#include "posegraph/ndt2d_posegraph_kernel.h"
#include "posegraph/ndt2d_posegraph_state.h"

namespace ndt2d
{

namespace
{

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
  const uint32_t cg_cap = pg_cg_cap(G.n);
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

}  // namespace

// ---- the host helpers the three units share (declared in posegraph/ndt2d_posegraph_state.h) ----

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

size_t pg_job_doubles(const ndt2d_posegraph * s)
{
  return (kPgNodeDoubles + (s->chain ? kPgChainDoubles : 0)) * s->n + (s->loss != pg::kLossTrivial ? s->m : 0);
}

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

namespace
{

// The evaluate kernel of the object's loss.
void pg_evaluate(const ndt2d_posegraph * s, hipStream_t stream, uint32_t jobs, const PgGraph & G, const uint8_t * d_en, const double * poses,
                 size_t pose_stride, double * cost, double * chi2, size_t chi2_stride, double * residuals)
{
  pg_dispatch(s, [&](auto, auto loss) {
    hipLaunchKernelGGL(posegraph_evaluate_kernel<decltype(loss)::value>, dim3(jobs), dim3(kPgThreads), 0, stream, G, d_en, poses, pose_stride,
                       cost, chi2, chi2_stride, residuals);
  });
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
  for (void * p : {s->d_graph, s->d_index, s->d_enabled, s->d_work, s->d_marginals, s->marginal_poses.d, s->d_marginal_nodes})
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
  ndt2d::PgCall call;
  int rc = ndt2d::pg_begin_call(s, s, "ndt2d_posegraph_evaluate", &call);
  if (rc != NDT2D_OK) return rc;
  const hipStream_t stream = call.stream;
  const ndt2d::PgGraph & G = call.G;
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
    rc = ndt2d::batch_round_trip(s, stream, total, [&] {
      ndt2d::pg_evaluate(s, stream, static_cast<uint32_t>(kc), G, d_en, G.poses, size_t(0), s->d_out,
                         chi2_out != nullptr ? s->d_out + at_chi2 : nullptr, m, residuals_out != nullptr ? s->d_out + at_res : nullptr);
      return NDT2D_OK;
    });
    if (rc != NDT2D_OK) return rc;
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
  int rc = ndt2d::batch_refuse(s, ndt2d::pg_args::tolerances_refusal("ndt2d_posegraph_solve", gradient_tolerance, function_tolerance,
                                                                       parameter_tolerance));
  if (rc != NDT2D_OK) return rc;
  ndt2d::PgCall call;
  rc = ndt2d::pg_begin_call(s, s, "ndt2d_posegraph_solve", &call);
  if (rc != NDT2D_OK) return rc;
  const hipStream_t stream = call.stream;
  const ndt2d::PgGraph & G = call.G;
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
    rc = ndt2d::batch_round_trip(s, stream, total, [&] {
      const uint32_t blocks = static_cast<uint32_t>(kc);
      if (chi2_out != nullptr)
      {
        ndt2d::pg_evaluate(s, stream, blocks, G, d_en, G.poses, size_t(0), nullptr, s->d_out + at_chi2, 2 * m, nullptr);
        NDT2D_BATCH_HIP(s, hipGetLastError());
      }
      // the solve kernel of the object's preconditioner and loss
      ndt2d::pg_dispatch(s, [&](auto prec, auto loss) {
        hipLaunchKernelGGL((ndt2d::posegraph_solve_kernel<decltype(prec)::value, decltype(loss)::value>), dim3(blocks), dim3(ndt2d::kPgThreads),
                           0, stream, G, d_en, static_cast<double *>(s->d_work), rules, s->d_out, s->d_out + at_rec);
      });
      if (chi2_out != nullptr)
      {
        NDT2D_BATCH_HIP(s, hipGetLastError());
        ndt2d::pg_evaluate(s, stream, blocks, G, d_en, s->d_out, 3 * n, nullptr, s->d_out + at_chi2 + m, 2 * m, nullptr);
      }
      return NDT2D_OK;
    });
    if (rc != NDT2D_OK) return rc;
    std::memcpy(poses_out + k0 * n * 3, s->h_out, kc * n * 3 * sizeof(double));
    std::memcpy(records_out + k0 * ndt2d::kPgRec, s->h_out + at_rec, kc * ndt2d::kPgRec * sizeof(double));
    if (chi2_out != nullptr && m != 0) std::memcpy(chi2_out + k0 * 2 * m, s->h_out + at_chi2, kc * 2 * m * sizeof(double));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
