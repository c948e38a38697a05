// Host-only check of the step of the Newton NDT registration
// (ndt_2d_amd/csrc/refine/ndt2d_refine_step.h): the damped 3 x 3 Cholesky solve on positive-
// definite, indefinite and singular systems, NaN and zero-gradient inputs, the lambda ladder up to
// STALLED, both tolerance stops and the count stop.  Every positive-definite solve is printed in
// hexadecimal ("solve H.. g.. lambda -> delta.."): tests/test_refine_host.py compares those bits
// with the restatement's Cholesky, which keeps the same operation order.  A program of its own,
// built with the host compiler and the sanitizers.
#include <cmath>
#include <cstdio>
#include <limits>

#include "ndt2d_refine_step.h"

using namespace ndt2d::refine;

static int bad = 0;

static void expect(bool ok, const char * what)
{
  if (!ok)
  {
    std::printf("FAILED: %s\n", what);
    ++bad;
  }
}

static Eval eval_of(double f, double g0, double g1, double g2, double xx, double xy, double xt, double yy, double yt, double tt)
{
  return Eval{f, {g0, g1, g2}, {xx, xy, xt, yy, yt, tt}};
}

static void print_solve(const Eval & e, double lambda)
{
  double d[3] = {0.0, 0.0, 0.0};
  const bool ok = damped_solve(e.H, e.g, lambda, d);
  expect(ok, "a positive-definite system is solved");
  std::printf("solve %a %a %a %a %a %a | %a %a %a | %a -> %a %a %a\n", e.H[0], e.H[1], e.H[2], e.H[3], e.H[4], e.H[5], e.g[0],
              e.g[1], e.g[2], lambda, d[0], d[1], d[2]);
  // the residual of (H + lambda D) delta + g, against the size of its terms
  const double D[3] = {std::fabs(e.H[0]), std::fabs(e.H[3]), std::fabs(e.H[5])};
  const double A[3][3] = {{e.H[0] + lambda * D[0], e.H[1], e.H[2]}, {e.H[1], e.H[3] + lambda * D[1], e.H[4]}, {e.H[2], e.H[4], e.H[5] + lambda * D[2]}};
  for (int r = 0; r < 3; ++r)
  {
    double res = e.g[r], size = std::fabs(e.g[r]);
    for (int c = 0; c < 3; ++c)
    {
      res += A[r][c] * d[c];
      size += std::fabs(A[r][c] * d[c]);
    }
    expect(std::fabs(res) <= 1e-12 * size, "the solution satisfies the system");
  }
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const Rules rules{32, 1e-6, 1e-6};
  const double start[3] = {1.0, -2.0, 0.5};

  // positive definite: the bits go to the test
  const Eval pd[] = {eval_of(-10.0, 1.0, -2.0, 0.5, 4.0, 1.0, 0.5, 3.0, 0.2, 2.0),
                     eval_of(-45.1, 682.4571, 169.43, -35.3353, 91234.5 / 3.0, -1234.25 / 7.0, 17.0 / 3.0, 60321.0 / 7.0, 4000.0 / 9.0, 1.0e6 / 3.0),
                     eval_of(-0.8, -8.6191, -4.7616, -30.4763, 1.0 / 3.0, 1.0 / 7.0, -1.0 / 9.0, 2.0 / 3.0, 1.0 / 11.0, 5.0 / 7.0),
                     eval_of(-1.0, 1e-7, -3e-7, 2e-9, 1e-3, 2e-4, -1e-4, 3e-3, 1e-5, 7e-2)};
  for (const Eval & e : pd)
  {
    print_solve(e, 0.0);
    print_solve(e, 1.0e-3);
    print_solve(e, 10.0);
  }

  // indefinite: no solve without damping; the ladder stops at the first lambda that makes it definite
  {
    const Eval e = eval_of(-1.0, 1.0, 1.0, 1.0, -1.0, 0.0, 0.0, 2.0, 0.0, 3.0);
    double d[3] = {7.0, 7.0, 7.0};
    expect(!damped_solve(e.H, e.g, 0.0, d) && d[0] == 7.0, "an indefinite system is refused and delta is not written");
    State s;
    expect(begin(s, start, e, rules), "indefinite: a trial is proposed");
    double lambda = 0.0;
    do
    {
      lambda = 10.0 * lambda > 1.0e-3 ? 10.0 * lambda : 1.0e-3;
    } while (!(-1.0 + lambda * 1.0 > 0.0));
    expect(s.lambda == lambda && lambda > 1.0 && lambda < 11.0, "indefinite: lambda is the ladder's first rung above 1");
    expect(s.evals == 1 && s.steps == 0 && s.f_start == -1.0, "indefinite: counters");
    // H + lambda |diag| = diag(-1 + lambda, 2 + 2 lambda, 3 + 3 lambda)
    expect(std::fabs((s.trial[0] - start[0]) - (-1.0 / (lambda - 1.0))) < 1e-15, "indefinite: the damped step along x");
  }

  // singular: a zero pivot is refused as a negative one is
  {
    const Eval e = eval_of(-1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0);
    double d[3];
    expect(!damped_solve(e.H, e.g, 0.0, d), "a singular system is refused");
    State s;
    expect(begin(s, start, e, rules) && s.lambda == 1.0e-3, "singular: the first rung solves it");
    const Eval zero = eval_of(-1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
    expect(!damped_solve(zero.H, zero.g, 0.0, d), "the zero matrix is refused");
    expect(damped_solve(zero.H, zero.g, 1.0e-3, d) && std::fabs(d[0] * (1.0e-3 * 1.0e-12) + 1.0) < 1e-12 && d[0] == d[1] && d[1] == d[2],
           "the zero matrix: D_j = 1e-12 scales the damping");
  }

  // NaN: in H no rung solves -> STALLED without an evaluation; in f at the start -> NOT_FINITE
  {
    State s;
    expect(!begin(s, start, eval_of(-1.0, 1.0, 1.0, 1.0, nan, 0.0, 0.0, 1.0, 0.0, 1.0), rules) && s.status == kStalled && s.evals == 1 &&
             s.lambda > kLambdaStall,
           "a NaN Hessian stalls");
    expect(s.pose[0] == start[0] && s.pose[1] == start[1] && s.pose[2] == start[2], "... at the start pose");
    expect(!begin(s, start, eval_of(nan, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), rules) && s.status == kNotFinite, "f = NaN: NOT_FINITE");
    expect(!begin(s, start, eval_of(-HUGE_VAL, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), rules) && s.status == kNotFinite, "f = -inf: NOT_FINITE");
    expect(!begin(s, start, eval_of(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), rules) && s.status == kNoOverlap, "f = 0: NO_OVERLAP");
    expect(!begin(s, start, eval_of(-0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), rules) && s.status == kNoOverlap && s.evals == 1 &&
             s.pose[2] == start[2],
           "f = -0: NO_OVERLAP");
    // a trial whose f is NaN is not accepted
    const Eval e = eval_of(-1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0);
    expect(begin(s, start, e, rules) && s.lambda == 0.0 && s.trial[0] == start[0] - 1.0, "a Newton step is proposed");
    expect(take(s, eval_of(nan, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), rules) && s.steps == 0 && s.evals == 2 && s.lambda == 1.0e-3 &&
             s.pose[0] == start[0] && s.at.f == -1.0,
           "f' = NaN: rejected, lambda raised, the pose stays");
    // a NaN gradient: the step is NaN, no tolerance test passes, the trial is NaN
    expect(begin(s, start, eval_of(-1.0, nan, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), rules) && s.trial[0] != s.trial[0], "a NaN gradient proposes a NaN trial");
  }

  // zero gradient: the step is zero, CONVERGED on the first evaluation
  {
    State s;
    expect(!begin(s, start, eval_of(-3.0, 0.0, 0.0, 0.0, 2.0, 0.1, 0.0, 2.0, 0.0, 1.0), rules) && s.status == kConverged && s.evals == 1 &&
             s.steps == 0 && s.lambda == 0.0 && s.at.f == -3.0,
           "zero gradient: CONVERGED");
  }

  // the ladder up to STALLED: every trial is refused
  {
    const Rules many{1000, 0.0, 0.0};
    const Eval e = eval_of(-1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0);
    State s;
    expect(begin(s, start, e, many), "ladder: a first trial");
    unsigned rungs = 0;
    double lambda = 0.0;
    bool more = true;
    while (more)
    {
      more = take(s, eval_of(-1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), many);   // f' == f is no decrease
      lambda = 10.0 * lambda > 1.0e-3 ? 10.0 * lambda : 1.0e-3;
      ++rungs;
      expect(s.lambda == lambda, "ladder: lambda = max(10 lambda, 1e-3)");
      if (rungs > 100) break;
    }
    expect(s.status == kStalled && lambda > 1.0e12 && lambda < 1.1e13 && s.evals == 1 + rungs && s.steps == 0, "ladder: STALLED past 1e12");
    expect(rungs == 16 || rungs == 17, "ladder: sixteen or seventeen rungs");
    expect(s.pose[0] == start[0] && s.at.f == -1.0, "ladder: the accepted pose and f stay");
    std::printf("ladder: %u rungs, lambda %a\n", rungs, lambda);
  }

  // acceptance: the pose moves, lambda falls by 10 and is 0 once <= 1e-9
  {
    const Eval e = eval_of(-1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0);
    State s;
    expect(begin(s, start, e, rules), "accept: a first trial");
    const Eval lower = eval_of(-2.0, 0.5, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0);
    s.lambda = 1.0e-3;
    const double trial0 = s.trial[0];
    expect(take(s, lower, rules) && s.steps == 1 && s.evals == 2 && s.pose[0] == trial0 && s.at.f == -2.0 && s.at.g[0] == 0.5 &&
             s.lambda == 1.0e-3 / 10.0,
           "accept: pose, f, g, H taken; lambda / 10");
    s.lambda = 5.0e-9;
    expect(take(s, eval_of(-3.0, 0.25, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), rules) && s.lambda == 0.0 && s.steps == 2 && s.f_start == -1.0,
           "accept: lambda is 0 once <= 1e-9");
  }

  // the tolerance stops and the count stop
  {
    State s;
    const Eval lin_small = eval_of(-1.0, 5.0e-7, -5.0e-7, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0);
    expect(!begin(s, start, lin_small, rules) && s.status == kConverged, "|dx|, |dy| < tol_lin: CONVERGED");
    const Rules tight_lin{32, 1.0e-7, 1.0e-6};
    expect(begin(s, start, lin_small, tight_lin), "|dx| >= tol_lin: goes on");
    const Eval ang_small = eval_of(-1.0, 0.0, 0.0, 5.0e-7, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0);
    expect(!begin(s, start, ang_small, rules) && s.status == kConverged, "|dtheta| < tol_ang: CONVERGED");
    const Rules tight_ang{32, 1.0e-6, 1.0e-7};
    expect(begin(s, start, ang_small, tight_ang) && s.trial[2] == start[2] - 5.0e-7, "|dtheta| >= tol_ang: goes on");
    expect(begin(s, start, ang_small, Rules{32, 0.0, 0.0}), "tolerances of 0 never stop a non-zero step");
    expect(begin(s, start, eval_of(-3.0, 0.0, 0.0, 0.0, 2.0, 0.1, 0.0, 2.0, 0.0, 1.0), Rules{32, 0.0, 0.0}) && s.trial[0] == start[0],
           "tolerances of 0: not even a zero step is < 0");
    const Eval big = eval_of(-1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0);
    expect(!begin(s, start, big, Rules{1, 1e-6, 1e-6}) && s.status == kMaxEvals && s.evals == 1, "max_evals = 1: the evaluation alone");
    expect(begin(s, start, big, Rules{2, 1e-6, 1e-6}), "max_evals = 2: one trial");
    expect(!take(s, eval_of(-2.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0), Rules{2, 1e-6, 1e-6}) && s.status == kMaxEvals && s.evals == 2 &&
             s.steps == 1,
           "max_evals = 2: MAX_EVALS after the accepted trial");
  }

  std::printf(bad == 0 ? "OK\n" : "FAILED\n");
  return bad == 0 ? 0 : 1;
}
