// The one launch path of the dense assemble-and-factor sequence: the nodes, the fill, the assembly
// under the graph's loss, then the plan's launches -- the factorisation A = L L^T and, where the
// layout has a T, the inversion T = L^-1 behind it.  The dense covariance (covariance/ndt2d_covariance.hip,
// CovJob, with the inversion) and the direct solve (direct/ndt2d_direct.hip, DirectJob, without) are
// this function on their own layouts; what follows it -- the blocks, or the substitutions and the
// step -- is theirs.  Its two parts, the fill and the plan's launches, are functions of their own for a
// unit that assembles a matrix itself (sparse/ndt2d_sparse.hip: the separators' Schur complement).
// The kernels are covariance/ndt2d_covariance_kernel.h, the list covariance/ndt2d_covariance_plan.h.
// Included by the .hip translation units only.
#ifndef NDT2D_COVARIANCE_LAUNCH_H_
#define NDT2D_COVARIANCE_LAUNCH_H_

#include <hip/hip_runtime.h>

#include <vector>

#include "covariance/ndt2d_covariance_kernel.h"
#include "covariance/ndt2d_covariance_plan.h"
#include "posegraph/ndt2d_posegraph_state.h"

namespace ndt2d
{

namespace
{

// The plan's launches for d unknowns in `list`: all of them, or (inverse false) the factor's part,
// those in front of the first of the inversion.
inline void cov_launch_list(size_t d, bool inverse, std::vector<cov::Launch> * list)
{
  list->resize(cov::launch_list(d, nullptr));
  (void)cov::launch_list(d, list->data());
  if (inverse) return;
  size_t factor = 0;
  while (factor < list->size() && (*list)[factor].kind <= cov::kUpdate) ++factor;
  list->resize(factor);
}

// What the sequence takes: the chunk's jobs on the layout `Job`, each at its poses.
struct CovFactorLaunch
{
  uint32_t jobs;
  const uint8_t * d_en;            // the masks of the chunk's jobs, or NULL
  const double * poses;            // the first job's poses
  size_t pose_stride;              // 0: the graph's poses for every job
  double damping;                  // of every job, where job_damping is NULL
  const double * job_damping;      // a job's own at job_damping[job x damping_stride], or NULL
  size_t damping_stride;
  double * workspace;              // [jobs] of Job's layout
  double * records;                // what the factor kernel writes per job
};

// The fill of the chunk's matrices of dimension 3 n on the layout `Job`: zero, the padding's unit
// diagonal (and T the identity where the layout has one).
template <class Job>
void cov_enqueue_fill(hipStream_t stream, uint32_t n, uint32_t jobs, double * workspace)
{
  const uint32_t ld = static_cast<uint32_t>(cov::padded(3 * static_cast<size_t>(n)));
  hipLaunchKernelGGL(covariance_fill_kernel<Job>, dim3((ld + kCovFillThreads - 1) / kCovFillThreads, ld, jobs), dim3(kCovFillThreads), 0, stream, n,
                     workspace);
}

// `launches` (cov_launch_list's, with the inversion's where kInverse) on matrices of dimension 3 n
// that are assembled already -- by cov_enqueue_factor below, or by a unit that assembles a matrix of
// its own (the sparse solve's separators: n is then their number).
template <class Job, bool kInverse>
void cov_enqueue_launches(hipStream_t stream, uint32_t n, uint32_t jobs, double * workspace, double * records,
                          const std::vector<cov::Launch> & launches)
{
  for (const cov::Launch & l : launches)
  {
    const dim3 grid(l.groups, 1, jobs);
    switch (l.kind)
    {
      case cov::kFactor:
        hipLaunchKernelGGL(covariance_factor_kernel<Job>, grid, dim3(kCovFactorThreads), 0, stream, n, l.panel, workspace, records);
        break;
      case cov::kSolveBelow:
        hipLaunchKernelGGL((covariance_solve_kernel<false, Job>), grid, dim3(kWave), 0, stream, n, l.panel, workspace);
        break;
      case cov::kUpdate:
        hipLaunchKernelGGL((covariance_update_kernel<false, Job>), grid, dim3(kCovUpdateThreads), 0, stream, n, l.panel, workspace);
        break;
      default:   // (the inversion's: in no list without it)
        if constexpr (kInverse)
        {
          if (l.kind == cov::kSolveRow) hipLaunchKernelGGL((covariance_solve_kernel<true, Job>), grid, dim3(kWave), 0, stream, n, l.panel, workspace);
          else hipLaunchKernelGGL((covariance_update_kernel<true, Job>), grid, dim3(kCovUpdateThreads), 0, stream, n, l.panel, workspace);
        }
        break;
    }
  }
}

// In stream order: nodes, fill, assemble, `launches` (cov_launch_list's, with the inversion's where
// kInverse).  graph: the object whose loss the assembly is compiled for.
template <class Job, bool kInverse>
void cov_enqueue_factor(const ndt2d_posegraph * graph, hipStream_t stream, const PgGraph & G, const CovFactorLaunch & a,
                        const std::vector<cov::Launch> & launches)
{
  const uint32_t n = G.n;
  const dim3 per_node((n + kCovNodeThreads - 1) / kCovNodeThreads, 1, a.jobs);
  hipLaunchKernelGGL(covariance_nodes_kernel<Job>, per_node, dim3(kCovNodeThreads), 0, stream, G, a.d_en, a.poses, a.pose_stride, a.workspace);
  cov_enqueue_fill<Job>(stream, n, a.jobs, a.workspace);
  pg_dispatch(graph, [&](auto, auto loss) {
    hipLaunchKernelGGL((covariance_assemble_kernel<decltype(loss)::value, Job>), per_node, dim3(kCovNodeThreads), 0, stream, G, a.d_en, a.poses,
                       a.pose_stride, a.damping, a.job_damping, a.damping_stride, a.workspace);
  });
  cov_enqueue_launches<Job, kInverse>(stream, n, a.jobs, a.workspace, a.records, launches);
}

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_COVARIANCE_LAUNCH_H_
