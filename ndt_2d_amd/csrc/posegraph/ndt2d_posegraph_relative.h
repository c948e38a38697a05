// What a consumer does with marginal covariances of the pose graph (include/ndt2d_hip.h, "Marginal
// covariances"): the relative pose of two nodes with its covariance from their joint marginal, and
// the squared Mahalanobis distance of a measured relative pose from a predicted one.  Plain C++
// without HIP types, host and plugin, as posegraph/ndt2d_posegraph_fn.h: IEEE + - x / sqrt and
// floor only (cos and sin of pose a's heading are the caller's), every operation written out in the
// order a restatement has to follow; a stand-alone host program checks it
// (tests/cpp/posegraph_relative_check.cpp).  Verdicts, no policy.
#ifndef NDT2D_POSEGRAPH_RELATIVE_H_
#define NDT2D_POSEGRAPH_RELATIVE_H_

#include "ndt2d_posegraph_fn.h"

namespace ndt2d
{
namespace posegraph
{

// The transform of pose b in pose a's frame, t = (R_a^T (p_b - p_a), theta_b - theta_a) (the heading
// difference is not wrapped, as makeConstraint's is not), and its covariance
//     [A B] sym(joint) [A B]^T
// with A = dt / d(pose a) and B = dt / d(pose b) of jacobian_a / jacobian_b and sym(J) = (J + J^T) / 2
// of the 6 x 6 joint = [aa ab; ba bb], given as four row-major 3 x 3 blocks [2][2][9].  A zero aa
// block (with ab and ba) means pose a is held.  c, s: cos and sin of pa[2].  The sums run over the six
// columns in ascending order from 0.0.
NDT2D_PG_HD inline void relative(double c, double s, const double * pa, const double * pb, const double * joint, double * t, double * cov)
{
  const Frame f = frame(c, s, pa, pb);
  t[0] = f.ex;
  t[1] = f.ey;
  t[2] = pb[2] - pa[2];
  double A[9], B[9], T[18], S[36], X[18];
  jacobian_a(f, A);
  jacobian_b(f, B);
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j)
    {
      T[6 * i + j] = A[3 * i + j];
      T[6 * i + 3 + j] = B[3 * i + j];
    }
  }
  // the joint as a 6 x 6, symmetrised
  for (int i = 0; i < 6; ++i)
  {
    for (int j = 0; j < 6; ++j)
    {
      const double ij = joint[9 * (2 * (i / 3) + j / 3) + 3 * (i % 3) + j % 3];
      const double ji = joint[9 * (2 * (j / 3) + i / 3) + 3 * (j % 3) + i % 3];
      S[6 * i + j] = 0.5 * (ij + ji);
    }
  }
  for (int i = 0; i < 3; ++i)
  {
    for (int k = 0; k < 6; ++k)
    {
      double v = 0.0;
      for (int l = 0; l < 6; ++l) v += T[6 * i + l] * S[6 * l + k];
      X[6 * i + k] = v;
    }
  }
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j)
    {
      double v = 0.0;
      for (int k = 0; k < 6; ++k) v += X[6 * i + k] * T[6 * j + k];
      cov[3 * i + j] = v;
    }
  }
}

// d^2 = e^T S^-1 e with e = meas - pred, its heading through normalize, and S = cov_pred + cov_meas
// (row-major 3 x 3, the lower triangle is read): S = L L^T by cholesky_lower, L y = e, d^2 = |y|^2.
// false (d2 untouched) when S is not positive definite as far as that factorisation can tell.
NDT2D_PG_HD inline bool distance(const double * t_pred, const double * cov_pred, const double * t_meas, const double * cov_meas, double * d2)
{
  double S[9], L[9], e[3], y[3];
  for (int i = 0; i < 9; ++i) S[i] = cov_pred[i] + cov_meas[i];
  if (!cholesky_lower(S, L)) return false;
  e[0] = t_meas[0] - t_pred[0];
  e[1] = t_meas[1] - t_pred[1];
  e[2] = normalize(t_meas[2] - t_pred[2]);
  y[0] = e[0] / L[0];
  y[1] = (e[1] - L[3] * y[0]) / L[4];
  y[2] = ((e[2] - L[6] * y[0]) - L[7] * y[1]) / L[8];
  *d2 = (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
  return true;
}

}  // namespace posegraph
}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_RELATIVE_H_
