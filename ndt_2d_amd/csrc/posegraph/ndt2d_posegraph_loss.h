// The robust losses of the pose graph (posegraph/ndt2d_posegraph_kernel.h): rho(s), rho'(s) and rho''(s)
// of s = |r|^2 >= 0 at a scale a > 0, b = a^2 -- the contract of include/ndt2d_hip.h ("Pose graph",
// robust losses).  Plain C++ without HIP types, host and device, as posegraph/ndt2d_posegraph_fn.h:
// the kernels' threads run it, ndt2d_robust_rho hands it out on the host, and a stand-alone host
// program checks it (tests/cpp/posegraph_loss_check.cpp).
//
//   trivial   rho = s                          rho' = 1                     rho'' = 0
//   huber     s <= b: as trivial; otherwise, q = sqrt(s):
//             rho = 2 a q - b                  rho' = max(DBL_MIN, a / q)   rho'' = -rho' / (2 s)
//   cauchy    u = 1 + s / b:
//             rho = b log(u)                   rho' = max(DBL_MIN, 1 / u)   rho'' = -rho'^2 / b
//
// Ceres's HuberLoss and CauchyLoss.  Both have rho'' <= 0 and rho' > 0 everywhere: the solver
// reweights (g = sum rho' J^T r, H = sum rho' J^T J) and applies no second-order correction.
// Cauchy's log(u) is taken as log1p(s / b): the same function, and rho keeps its leading digits
// where s / b is below the rounding of 1 (1 + s / b, formed first, would give rho = 0 there).
#ifndef NDT2D_POSEGRAPH_LOSS_H_
#define NDT2D_POSEGRAPH_LOSS_H_

#include <math.h>

#include "ndt2d_posegraph_fn.h"

namespace ndt2d
{
namespace posegraph
{

constexpr int kLossTrivial = 0, kLossHuber = 1, kLossCauchy = 2;
constexpr double kLossWeightMin = 2.2250738585072014e-308;   // DBL_MIN: rho' stays positive

// rho(s), what the cost sums.
template <int kLoss>
NDT2D_PG_HD inline double loss_rho(double s, double a, double b)
{
  if (kLoss == kLossHuber) return s <= b ? s : 2.0 * a * sqrt(s) - b;
  if (kLoss == kLossCauchy) return b * log1p(s / b);
  return s;
}

// rho'(s), the weight of the constraint in g and H.
template <int kLoss>
NDT2D_PG_HD inline double loss_weight(double s, double a, double b)
{
  if (kLoss == kLossHuber) return s <= b ? 1.0 : fmax(kLossWeightMin, a / sqrt(s));
  if (kLoss == kLossCauchy) return fmax(kLossWeightMin, 1.0 / (1.0 + s / b));
  return 1.0;
}

// rho''(s) from rho'(s) = w.
template <int kLoss>
NDT2D_PG_HD inline double loss_curvature(double s, double w, double b)
{
  if (kLoss == kLossHuber) return s <= b ? 0.0 : -w / (2.0 * s);
  if (kLoss == kLossCauchy) return -(w * w) / b;
  return 0.0;
}

// out3 = {rho, rho', rho''} of the loss `kind` (kLoss*); false for a kind there is none of.
NDT2D_PG_HD inline bool loss_evaluate(int kind, double a, double s, double * out3)
{
  const double b = a * a;
  if (kind == kLossTrivial)
  {
    out3[0] = loss_rho<kLossTrivial>(s, a, b);
    out3[1] = loss_weight<kLossTrivial>(s, a, b);
    out3[2] = loss_curvature<kLossTrivial>(s, out3[1], b);
    return true;
  }
  if (kind == kLossHuber)
  {
    out3[0] = loss_rho<kLossHuber>(s, a, b);
    out3[1] = loss_weight<kLossHuber>(s, a, b);
    out3[2] = loss_curvature<kLossHuber>(s, out3[1], b);
    return true;
  }
  if (kind == kLossCauchy)
  {
    out3[0] = loss_rho<kLossCauchy>(s, a, b);
    out3[1] = loss_weight<kLossCauchy>(s, a, b);
    out3[2] = loss_curvature<kLossCauchy>(s, out3[1], b);
    return true;
  }
  return false;
}

}  // namespace posegraph
}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_LOSS_H_
