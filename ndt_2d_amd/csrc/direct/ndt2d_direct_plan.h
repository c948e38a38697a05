// The plan of the direct pose-graph solve (direct/ndt2d_direct.hip): what a job holds on the device,
// in doubles, and how many jobs a byte budget holds.  Plain C++ without HIP types, host and device.
// The panels, the padding and the factor's launches are the dense covariance's
// (covariance/ndt2d_covariance_plan.h).
//
// A chunk's workspace is three regions, each [job][...]:
//   dense   the matrix A (then its factor L), padded(d)^2; A's diagonal as assembled, padded(d); cos,
//           sin and the free flag of each node, 3 n; the substitution's vector (-g, then y, then
//           delta), padded(d)                                             -- dense_doubles(n)
//   work    the solver's PgWork (posegraph/ndt2d_posegraph_kernel.h), kNodeDoubles a node, with m
//           doubles in front under a loss (rho' per constraint)           -- work_doubles(n, m, loss)
//   state   the LM state (direct/ndt2d_direct_step.h's State) and the factor kernel's record
//                                                                         -- kStateDoubles
#ifndef NDT2D_DIRECT_PLAN_H_
#define NDT2D_DIRECT_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include "covariance/ndt2d_covariance_plan.h"

namespace ndt2d
{
namespace direct
{

constexpr size_t kNodeDoubles = 41;    // kPgNodeDoubles (the kernel header holds them equal)
constexpr size_t kStateDoubles = 16;   // State's 11 doubles, the factor's record of 3 behind them at kFactorRecord
constexpr size_t kFactorRecord = 12;

NDT2D_COV_HD inline size_t dense_doubles(size_t n)
{
  const size_t ld = covariance::padded(3 * n);
  return ld * ld + 2 * ld + 3 * n;
}

NDT2D_COV_HD inline size_t work_doubles(size_t n, size_t m, bool loss) { return kNodeDoubles * n + (loss ? m : 0); }

NDT2D_COV_HD inline size_t job_doubles(size_t n, size_t m, bool loss) { return dense_doubles(n) + work_doubles(n, m, loss) + kStateDoubles; }

}  // namespace direct
}  // namespace ndt2d

#endif  // NDT2D_DIRECT_PLAN_H_
