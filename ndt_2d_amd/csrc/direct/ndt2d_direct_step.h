// The Levenberg-Marquardt decisions of the direct pose-graph solve (direct/ndt2d_direct_kernel.h;
// include/ndt2d_hip.h, "Direct solve"): what ONE thread decides in one iteration from the reduced
// values every thread holds -- whether the step is taken, the new lambda and nu, and the four stop
// rules.  The rules are the CG solver's (posegraph/ndt2d_posegraph.hip, posegraph_solve_kernel) with
// the two differences of an exact linear step: the model's decrease has no residual term, and a
// factorisation that fails is a rejected step without a trial point.  Plain C++ without HIP types,
// host and device: the step kernel runs it, and a stand-alone host program checks every branch
// (tests/cpp/direct_step_check.cpp).  The translation units are compiled with -ffp-contract=off.
//
// An iteration in the order its values become known:
//   propose(s, in, rules)   the factor's verdict and the step's norms: kRejected (the factorisation
//                           failed), kStopped (the step rule) or kEvaluate (the trial's cost is wanted)
//   take(s, in)             the trial's cost and the model's decrease: accepted or rejected
//   settle(s, gmax, rules)  behind an accepted step's linearisation: the gradient and the cost rule
#ifndef NDT2D_DIRECT_STEP_H_
#define NDT2D_DIRECT_STEP_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_DIRECT_HD __host__ __device__
#else
#define NDT2D_DIRECT_HD
#endif

namespace ndt2d
{
namespace direct
{

// NDT2D_POSEGRAPH_CONVERGED_GRADIENT ... NDT2D_POSEGRAPH_FAILED of the public header
constexpr int kConvergedGradient = 0, kConvergedCost = 1, kConvergedStep = 2, kMaxIterations = 3, kFailed = 4;

constexpr double kLambda0 = 1e-4;
constexpr double kLambdaMin = 1e-32, kLambdaMax = 1e32;
constexpr double kMinGain = 1e-3;                         // a step is accepted above this gain ratio
constexpr double kNoise = 256.0 * 2.220446049250313e-16;  // |dF| <= this x F: below the cost's own rounding

// what propose() says
constexpr int kRejected = 0, kStopped = 1, kEvaluate = 2;

struct Rules
{
  uint32_t max_iterations;
  double gradient_tolerance, function_tolerance, parameter_tolerance;
};

// A job between two iterations: the first eight are its record (NDT2D_DIRECT_RECORD_DOUBLES).
struct State
{
  double status, iterations, rejected, not_positive_definite, initial_cost, cost, gradient, pivot_ratio;
  double lambda, nu;
  double cost_before;   // F before the last accepted step (settle's cost rule)
};

// The inputs of one iteration.
struct Input
{
  bool factor_failed;        // the factor kernel's record: a pivot <= 0 or not finite
  double pivot_ratio;        // the factorisation's smallest pivot / diagonal, where it succeeded
  double step, x_norm;       // |delta|_2, |x|_2
  double trial_cost;         // F at x + delta
  double predicted;          // 1/2 (lambda delta^T D delta - g^T delta)
};

NDT2D_DIRECT_HD inline bool finite_value(double v) { return (v - v) == 0.0; }
NDT2D_DIRECT_HD inline double magnitude(double v) { return v < 0.0 ? -v : v; }

// The start: F and |g|_inf at the start poses.  A cost that is not finite fails the job (gmax is
// then not looked at); a gradient within the tolerance ends it before the first iteration.
NDT2D_DIRECT_HD inline void begin(State & s, double cost, double gmax, const Rules & rules)
{
  s.status = kMaxIterations;
  s.iterations = s.rejected = s.not_positive_definite = 0.0;
  s.initial_cost = s.cost = s.cost_before = cost;
  s.gradient = 0.0;
  s.pivot_ratio = 1.0;
  s.lambda = kLambda0;
  s.nu = 2.0;
  if (!finite_value(cost))
  {
    s.status = kFailed;
    return;
  }
  s.gradient = gmax;
  if (gmax <= rules.gradient_tolerance) s.status = kConvergedGradient;
}

// Whether the job takes another iteration.
NDT2D_DIRECT_HD inline bool iterating(const State & s, const Rules & rules)
{
  return s.status == kMaxIterations && s.iterations < static_cast<double>(rules.max_iterations);
}

// lambda and nu after a step that is not taken.
NDT2D_DIRECT_HD inline void reject(State & s)
{
  const double grown = s.lambda * s.nu;
  s.lambda = grown < kLambdaMax ? grown : kLambdaMax;
  s.nu = s.nu * 2.0;
  s.rejected += 1.0;
}

NDT2D_DIRECT_HD inline int propose(State & s, const Input & in, const Rules & rules)
{
  s.iterations += 1.0;
  if (in.factor_failed)
  {
    s.not_positive_definite += 1.0;
    reject(s);
    return kRejected;
  }
  s.pivot_ratio = in.pivot_ratio;
  if (rules.parameter_tolerance > 0.0 && in.step <= rules.parameter_tolerance * (in.x_norm + rules.parameter_tolerance))
  {
    s.status = kConvergedStep;
    return kStopped;
  }
  return kEvaluate;
}

// true: the trial point becomes x (and settle follows its linearisation).
NDT2D_DIRECT_HD inline bool take(State & s, const Input & in)
{
  const double dF = s.cost - in.trial_cost;
  // below the rounding of the cost's own sum the gain ratio is noise: the model decides
  const bool noise = magnitude(dF) <= kNoise * s.cost;
  const double gain = dF / in.predicted;
  if (finite_value(in.trial_cost) && in.predicted > 0.0 && (noise || gain > kMinGain))
  {
    const double t = 2.0 * gain - 1.0;
    const double cube = 1.0 - t * t * t;
    double factor = cube > 1.0 / 3.0 ? cube : 1.0 / 3.0;   // (a NaN gives 1 / 3)
    if (noise) factor = 1.0 / 3.0;
    double lambda = s.lambda * factor;
    lambda = lambda > kLambdaMin ? lambda : kLambdaMin;
    s.lambda = lambda < kLambdaMax ? lambda : kLambdaMax;
    s.nu = 2.0;
    s.cost_before = s.cost;
    s.cost = in.trial_cost;
    return true;
  }
  reject(s);
  return false;
}

NDT2D_DIRECT_HD inline void settle(State & s, double gmax, const Rules & rules)
{
  s.gradient = gmax;
  if (gmax <= rules.gradient_tolerance)
  {
    s.status = kConvergedGradient;
  }
  else if (rules.function_tolerance > 0.0 && magnitude(s.cost_before - s.cost) <= rules.function_tolerance * s.cost_before)
  {
    s.status = kConvergedCost;
  }
}

}  // namespace direct
}  // namespace ndt2d

#endif  // NDT2D_DIRECT_STEP_H_
