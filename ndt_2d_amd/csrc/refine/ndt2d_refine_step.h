// The step of the Newton NDT registration (refine/ndt2d_refine_kernel.h): what ONE thread does between
// two evaluations of (f, g, H) -- the 3 x 3 Cholesky solve of the damped system, the lambda rule
// and the stop rules of include/ndt2d_hip.h ("Newton NDT registration").  Plain C++ without HIP
// types, host and device: the kernel's thread 0 runs it, and a stand-alone host program checks it
// (tests/cpp/refine_step_check.cpp).  Every operation is written out in the order a restatement
// has to follow; the translation units are compiled with -ffp-contract=off.
#ifndef NDT2D_REFINE_STEP_H_
#define NDT2D_REFINE_STEP_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_REFINE_HD __host__ __device__
#else
#define NDT2D_REFINE_HD
#endif

namespace ndt2d
{
namespace refine
{

// NDT2D_REFINE_CONVERGED ... NDT2D_REFINE_NOT_FINITE of the public header
constexpr int kConverged = 0, kMaxEvals = 1, kStalled = 2, kNoOverlap = 3, kNotFinite = 4;

constexpr double kLambdaFirst = 1.0e-3;    // the first damping after a failure
constexpr double kLambdaGrow = 10.0;
constexpr double kLambdaOff = 1.0e-9;      // at or below: no damping
constexpr double kLambdaStall = 1.0e12;    // above: the job has stalled
constexpr double kScaleFloor = 1.0e-12;    // D_j = max(|H_jj|, this)

// f and its derivatives at one pose; H as xx, xy, xt, yy, yt, tt.
struct Eval
{
  double f;
  double g[3];
  double H[6];
};

struct Rules
{
  uint32_t max_evals;
  double tol_lin, tol_ang;
};

// A job between two evaluations.  pose / at: the accepted pose and its (f, g, H); trial: the pose
// the next evaluation is wanted at (while the step functions return true).
struct State
{
  double pose[3];
  Eval at;
  double f_start;
  double lambda;
  uint32_t evals, steps;
  int status;
  double trial[3];
};

NDT2D_REFINE_HD inline double magnitude(double v) { return v < 0.0 ? -v : v; }
NDT2D_REFINE_HD inline bool finite_value(double v) { return (v - v) == 0.0; }

// (H + lambda diag D) delta = -g, D_j = max(|H_jj|, kScaleFloor), by Cholesky.  false: a pivot
// is not > 0 (which a NaN is not either); delta is then not written.
NDT2D_REFINE_HD inline bool damped_solve(const double (&H)[6], const double (&g)[3], double lambda, double (&delta)[3])
{
  const double d0 = magnitude(H[0]) > kScaleFloor ? magnitude(H[0]) : kScaleFloor;
  const double d1 = magnitude(H[3]) > kScaleFloor ? magnitude(H[3]) : kScaleFloor;
  const double d2 = magnitude(H[5]) > kScaleFloor ? magnitude(H[5]) : kScaleFloor;
  const double a00 = H[0] + lambda * d0, a01 = H[1], a02 = H[2];
  const double a11 = H[3] + lambda * d1, a12 = H[4];
  const double a22 = H[5] + lambda * d2;
  if (!(a00 > 0.0)) return false;
  const double l00 = sqrt(a00);
  const double l10 = a01 / l00;
  const double l20 = a02 / l00;
  const double p1 = a11 - l10 * l10;
  if (!(p1 > 0.0)) return false;
  const double l11 = sqrt(p1);
  const double l21 = (a12 - l20 * l10) / l11;
  const double p2 = (a22 - l20 * l20) - l21 * l21;
  if (!(p2 > 0.0)) return false;
  const double l22 = sqrt(p2);
  // L y = -g
  const double y0 = -g[0] / l00;
  const double y1 = (-g[1] - l10 * y0) / l11;
  const double y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22;
  // L^T delta = y
  const double t2 = y2 / l22;
  const double t1 = (y1 - l21 * t2) / l11;
  const double t0 = ((y0 - l10 * t1) - l20 * t2) / l00;
  delta[0] = t0;
  delta[1] = t1;
  delta[2] = t2;
  return true;
}

// cov = H^-1, row-major 3 x 3, by the same Cholesky with lambda = 0 and no D scaling: H = L L^T,
// M = L^-1, cov = M^T M.  false: an entry of H is not finite, a pivot is not > 0, or an entry of
// the inverse is not finite; cov is then not written.  The mirrored entries are copies: cov is
// symmetric bit for bit.
NDT2D_REFINE_HD inline bool covariance(const double (&H)[6], double (&cov)[9])
{
  for (int k = 0; k < 6; ++k)
  {
    if (!finite_value(H[k])) return false;
  }
  const double a00 = H[0], a01 = H[1], a02 = H[2], a11 = H[3], a12 = H[4], a22 = H[5];
  if (!(a00 > 0.0)) return false;
  const double l00 = sqrt(a00);
  const double l10 = a01 / l00;
  const double l20 = a02 / l00;
  const double p1 = a11 - l10 * l10;
  if (!(p1 > 0.0)) return false;
  const double l11 = sqrt(p1);
  const double l21 = (a12 - l20 * l10) / l11;
  const double p2 = (a22 - l20 * l20) - l21 * l21;
  if (!(p2 > 0.0)) return false;
  const double l22 = sqrt(p2);
  // M = L^-1 (lower triangular)
  const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
  const double m10 = -(l10 * m00) / l11;
  const double m21 = -(l21 * m11) / l22;
  const double m20 = -(l20 * m00 + l21 * m10) / l22;
  const double c00 = (m00 * m00 + m10 * m10) + m20 * m20;
  const double c01 = m10 * m11 + m20 * m21;
  const double c02 = m20 * m22;
  const double c11 = m11 * m11 + m21 * m21;
  const double c12 = m21 * m22;
  const double c22 = m22 * m22;
  if (!finite_value(c00) || !finite_value(c01) || !finite_value(c02) || !finite_value(c11) || !finite_value(c12) ||
      !finite_value(c22))
  {
    return false;
  }
  cov[0] = c00;
  cov[1] = cov[3] = c01;
  cov[2] = cov[6] = c02;
  cov[4] = c11;
  cov[5] = cov[7] = c12;
  cov[8] = c22;
  return true;
}

// lambda after a failure (a pivot, or a trial that did not lower f); false: stalled.
NDT2D_REFINE_HD inline bool raise_lambda(State & s)
{
  const double grown = kLambdaGrow * s.lambda;
  s.lambda = grown > kLambdaFirst ? grown : kLambdaFirst;
  if (s.lambda > kLambdaStall)
  {
    s.status = kStalled;
    return false;
  }
  return true;
}

// The next trial pose from the accepted one; false: the job has stopped (s.status says why).
NDT2D_REFINE_HD inline bool propose(State & s, const Rules & rules)
{
  if (s.evals >= rules.max_evals)
  {
    s.status = kMaxEvals;
    return false;
  }
  double delta[3];
  while (!damped_solve(s.at.H, s.at.g, s.lambda, delta))
  {
    if (!raise_lambda(s)) return false;
  }
  if (magnitude(delta[0]) < rules.tol_lin && magnitude(delta[1]) < rules.tol_lin && magnitude(delta[2]) < rules.tol_ang)
  {
    s.status = kConverged;
    return false;
  }
  s.trial[0] = s.pose[0] + delta[0];
  s.trial[1] = s.pose[1] + delta[1];
  s.trial[2] = s.pose[2] + delta[2];   // (not normalised: the reference adds raw corrections too)
  return true;
}

// The evaluation at the start pose.  true: s.trial wants an evaluation.
NDT2D_REFINE_HD inline bool begin(State & s, const double (&start)[3], const Eval & e, const Rules & rules)
{
  s.pose[0] = s.trial[0] = start[0];
  s.pose[1] = s.trial[1] = start[1];
  s.pose[2] = s.trial[2] = start[2];
  s.at = e;
  s.f_start = e.f;
  s.lambda = 0.0;
  s.evals = 1;
  s.steps = 0;
  s.status = kMaxEvals;
  if (e.f == 0.0)   // (-0.0 too: no beam scores)
  {
    s.status = kNoOverlap;
    return false;
  }
  if (!finite_value(e.f))
  {
    s.status = kNotFinite;
    return false;
  }
  return propose(s, rules);
}

// The evaluation at s.trial.  true: s.trial wants another.
NDT2D_REFINE_HD inline bool take(State & s, const Eval & e, const Rules & rules)
{
  s.evals += 1;
  if (e.f < s.at.f)   // (a NaN does not pass)
  {
    s.pose[0] = s.trial[0];
    s.pose[1] = s.trial[1];
    s.pose[2] = s.trial[2];
    s.at = e;
    s.steps += 1;
    s.lambda = s.lambda / kLambdaGrow;
    if (s.lambda <= kLambdaOff) s.lambda = 0.0;
  }
  else if (!raise_lambda(s))
  {
    return false;
  }
  return propose(s, rules);
}

}  // namespace refine
}  // namespace ndt2d

#endif  // NDT2D_REFINE_STEP_H_
