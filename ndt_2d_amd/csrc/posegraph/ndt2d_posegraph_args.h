// What the pose-graph calls refuse about their arguments, on the host: the solver, the marginal
// covariances, the dense covariance and the direct solve share it -- one text per refusal, so that
// the entry points cannot drift apart in what they refuse.  As batch/ndt2d_refine_jobs.h: each
// function returns the refusal's text, prefixed with `entry`, or an empty string, and goes through
// batch_refuse.  The dense limits are arguments (the dense plan's kMaxDim and chunk_jobs): the plan
// is not named under posegraph/.  Plain C++: no HIP; a stand-alone host program checks every text
// (tests/cpp/posegraph_args_check.cpp).
#ifndef NDT2D_POSEGRAPH_ARGS_H_
#define NDT2D_POSEGRAPH_ARGS_H_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace ndt2d
{

namespace pg_args
{

// The caller's poses of n_jobs jobs of n nodes, [job][node][3]: the first value that is not finite,
// by its job and pose.  NULL: the graph's own poses, nothing to refuse.
inline std::string poses_refusal(const char * entry, const double * poses, size_t n_jobs, size_t n)
{
  if (poses == nullptr) return std::string();
  for (size_t i = 0; i < n_jobs * n * 3; ++i)
  {
    if (!std::isfinite(poses[i]))
    {
      return std::string(entry) + ": job " + std::to_string(i / (3 * n)) + " pose " + std::to_string(i / 3 % n) + " is not finite";
    }
  }
  return std::string();
}

inline std::string damping_refusal(const char * entry, double damping)
{
  if (!(damping >= 0.0) || !std::isfinite(damping)) return std::string(entry) + ": the damping is negative or not finite";
  return std::string();
}

// The three tolerances of a solve (0 disables a rule).
inline std::string tolerances_refusal(const char * entry, double gradient_tolerance, double function_tolerance, double parameter_tolerance)
{
  if (!(gradient_tolerance >= 0.0) || !(function_tolerance >= 0.0) || !(parameter_tolerance >= 0.0) || !std::isfinite(gradient_tolerance) ||
      !std::isfinite(function_tolerance) || !std::isfinite(parameter_tolerance))
  {
    return std::string(entry) + ": a tolerance is negative or not finite";
  }
  return std::string();
}

// `count` items of `per_item` node ids each ("query": 1, "pair": 2) against the graph's n nodes: the
// first id that names no node, by its item.
inline std::string nodes_refusal(const char * entry, const char * noun, const uint32_t * ids, size_t count, size_t per_item, size_t n)
{
  for (size_t q = 0; q < count * per_item; ++q)
  {
    if (ids[q] >= n)
    {
      return std::string(entry) + ": " + noun + " " + std::to_string(q / per_item) + " names node " + std::to_string(ids[q]) + " of " +
             std::to_string(n);
    }
  }
  return std::string();
}

// The dense limits: a matrix of 3 n unknowns against max_dim, then the jobs the workspace's budget
// holds (chunk, what the plan's chunk_jobs gives for job_bytes a job: 0 where not even one fits).
inline std::string dense_refusal(const char * entry, size_t n, size_t max_dim, size_t chunk, size_t job_bytes, size_t workspace_bytes)
{
  if (3 * n > max_dim) return std::string(entry) + ": " + std::to_string(n) + " poses, a dense matrix holds " + std::to_string(max_dim / 3);
  if (chunk == 0)
  {
    return std::string(entry) + ": a job of " + std::to_string(n) + " poses needs " + std::to_string(job_bytes) + " bytes, the workspace is " +
           std::to_string(workspace_bytes);
  }
  return std::string();
}

}  // namespace pg_args

}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_ARGS_H_
