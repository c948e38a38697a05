// Host-only check of the decisions of the direct pose-graph solve
// (ndt_2d_amd/csrc/direct/ndt2d_direct_step.h): every branch of an iteration -- accept by gain, accept
// by noise, reject by gain, a trial cost that is not finite, a model that predicts no decrease, a
// failed factorisation without a trial, each of the four stop rules, a start that is not finite,
// and lambda's clamps at both ends.  The expectations are written out from the rules of
// include/ndt2d_hip.h ("Direct solve").  A program of its own, built with the host compiler, plainly
// and with the sanitizers.
#include <cmath>
#include <cstdio>
#include <limits>

#include "ndt2d_direct_step.h"

using namespace ndt2d::direct;

static int bad = 0;

static void expect(bool ok, const char * what)
{
  if (!ok)
  {
    std::printf("FAILED: %s\n", what);
    ++bad;
  }
}

// A job at cost F with gradient 1 and the rules' tolerances all off but those given.
static State started(double F, const Rules & rules)
{
  State s;
  begin(s, F, 1.0, rules);
  return s;
}

static Input trial(double Ft, double predicted)
{
  Input in{};
  in.factor_failed = false;
  in.pivot_ratio = 0.5;
  in.step = 1.0;
  in.x_norm = 10.0;
  in.trial_cost = Ft;
  in.predicted = predicted;
  return in;
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double eps = 2.220446049250313e-16;
  const Rules off{100, 0.0, 0.0, 0.0};

  // ---- the start ----
  {
    State s = started(8.0, off);
    expect(s.status == kMaxIterations && s.iterations == 0.0 && s.rejected == 0.0 && s.not_positive_definite == 0.0, "a fresh job iterates");
    expect(s.initial_cost == 8.0 && s.cost == 8.0 && s.gradient == 1.0 && s.lambda == 1e-4 && s.nu == 2.0 && s.pivot_ratio == 1.0, "its first state");
    expect(iterating(s, off), "it takes an iteration");
    const Rules none{0, 0.0, 0.0, 0.0};
    expect(!iterating(s, none), "max_iterations = 0: none");
    State t;
    begin(t, 8.0, 1e-3, Rules{100, 1e-3, 0.0, 0.0});
    expect(t.status == kConvergedGradient && t.gradient == 1e-3 && !iterating(t, off), "a start gradient at the tolerance ends the job");
    begin(t, 0.0, 0.0, off);
    expect(t.status == kConvergedGradient, "no constraint, or one pose: the gradient is 0, converged");
    begin(t, nan, 1.0, off);
    expect(t.status == kFailed && t.gradient == 0.0 && !iterating(t, off), "a start cost that is NaN fails the job");
    begin(t, inf, 1.0, off);
    expect(t.status == kFailed, "a start cost that is infinite fails the job");
  }

  // ---- accept by gain: F 8 -> 6 where the model said 2: gain 1, lambda x max(1/3, 1 - 1) ----
  {
    State s = started(8.0, off);
    Input in = trial(6.0, 2.0);
    expect(propose(s, in, off) == kEvaluate && s.iterations == 1.0 && s.pivot_ratio == 0.5, "a factorisation that succeeded asks for the trial's cost");
    expect(take(s, in), "gain 1 is accepted");
    expect(s.cost == 6.0 && s.cost_before == 8.0 && s.lambda == 1e-4 * (1.0 / 3.0) && s.nu == 2.0 && s.rejected == 0.0, "lambda falls to a third");
    settle(s, 0.25, off);
    expect(s.status == kMaxIterations && s.gradient == 0.25, "no rule stops it");
    // gain 1/2: 1 - 0^3 = 1, lambda stays
    State h = started(8.0, off);
    in = trial(7.0, 2.0);
    expect(propose(h, in, off) == kEvaluate && take(h, in) && h.lambda == 1e-4, "gain 1/2 keeps lambda");
    // gain 1/4: 1 - (-1/2)^3 = 1.125
    State q = started(8.0, off);
    in = trial(7.5, 2.0);
    expect(propose(q, in, off) == kEvaluate && take(q, in) && q.lambda == 1e-4 * 1.125, "gain 1/4 raises lambda by an eighth");
    // nu returns to 2 behind a rejection
    State r = started(8.0, off);
    in = trial(9.0, 2.0);
    expect(propose(r, in, off) == kEvaluate && !take(r, in) && r.nu == 4.0, "a rejection doubles nu");
    in = trial(6.0, 2.0);
    expect(propose(r, in, off) == kEvaluate && take(r, in) && r.nu == 2.0 && r.iterations == 2.0 && r.rejected == 1.0, "an acceptance resets nu");
  }

  // ---- reject by gain ----
  {
    State s = started(8.0, off);
    Input in = trial(8.0 - 1e-3, 2.0);   // gain 5e-4 < 1e-3
    expect(propose(s, in, off) == kEvaluate && !take(s, in), "a gain of 5e-4 is rejected");
    expect(s.cost == 8.0 && s.lambda == 2e-4 && s.nu == 4.0 && s.rejected == 1.0 && s.not_positive_definite == 0.0, "lambda x nu, nu x 2");
    in = trial(9.0, 2.0);                // the cost rose
    expect(propose(s, in, off) == kEvaluate && !take(s, in) && s.lambda == 8e-4 && s.nu == 8.0 && s.rejected == 2.0, "again: lambda x 4, nu x 2");
    expect(s.iterations == 2.0 && s.status == kMaxIterations, "rejected iterations are counted");
  }

  // ---- accept by noise: |dF| <= 256 eps F, the model decides, lambda x 1/3 whatever the gain ----
  {
    State s = started(8.0, off);
    Input in = trial(8.0 + 8.0 * 100.0 * eps, 1e-20);   // the cost "rose" by 100 eps F: noise
    expect(propose(s, in, off) == kEvaluate && take(s, in), "a change below the cost's rounding is accepted where the model predicts a decrease");
    expect(s.lambda == 1e-4 * (1.0 / 3.0) && s.cost == 8.0 + 8.0 * 100.0 * eps, "lambda falls to a third under the noise rule");
    State t = started(8.0, off);
    in = trial(8.0 + 8.0 * 300.0 * eps, 1e-20);         // 300 eps F: not noise, and a rise
    expect(propose(t, in, off) == kEvaluate && !take(t, in), "a rise above the noise level is rejected");
    State z = started(0.0, Rules{100, 0.0, 0.0, 0.0});
    in = trial(0.0, 1e-30);                             // F = 0: dF = 0 <= 0
    expect(propose(z, in, off) == kEvaluate && take(z, in), "at F = 0 a step that keeps it is noise");
  }

  // ---- a trial cost that is not finite, a model that predicts no decrease ----
  {
    State s = started(8.0, off);
    Input in = trial(nan, 2.0);
    expect(propose(s, in, off) == kEvaluate && !take(s, in) && s.cost == 8.0 && s.rejected == 1.0, "a NaN trial cost is rejected");
    in = trial(inf, 2.0);
    expect(propose(s, in, off) == kEvaluate && !take(s, in), "an infinite trial cost is rejected");
    in = trial(-inf, 2.0);
    expect(propose(s, in, off) == kEvaluate && !take(s, in), "minus infinity too");
    in = trial(6.0, 0.0);
    expect(propose(s, in, off) == kEvaluate && !take(s, in), "predicted = 0 is rejected");
    in = trial(6.0, -2.0);
    expect(propose(s, in, off) == kEvaluate && !take(s, in), "predicted < 0 is rejected");
    in = trial(6.0, nan);
    expect(propose(s, in, off) == kEvaluate && !take(s, in), "predicted NaN is rejected");
    in = trial(8.0, 0.0);
    expect(propose(s, in, off) == kEvaluate && !take(s, in), "noise does not pass a model without a decrease");
    expect(s.rejected == 7.0 && s.iterations == 7.0 && s.cost == 8.0, "seven rejections");
  }

  // ---- a failed factorisation: a rejection without a trial ----
  {
    State s = started(8.0, off);
    Input in{};
    in.factor_failed = true;
    in.pivot_ratio = -3.0;
    in.step = nan;
    in.x_norm = nan;
    expect(propose(s, in, Rules{100, 0.0, 0.0, 1.0}) == kRejected, "no trial point (and the step rule is not asked)");
    expect(s.iterations == 1.0 && s.rejected == 1.0 && s.not_positive_definite == 1.0 && s.lambda == 2e-4 && s.nu == 4.0, "lambda and nu as on a rejection");
    expect(s.pivot_ratio == 1.0 && s.status == kMaxIterations && s.cost == 8.0, "the pivot ratio is the last successful factorisation's");
  }

  // ---- the stop rules ----
  {
    const Rules gradient{100, 1e-6, 0.0, 0.0}, cost{100, 0.0, 0x1p-20, 0.0}, step{100, 0.0, 0.0, 1e-8}, count{2, 0.0, 0.0, 0.0};
    State s = started(8.0, gradient);
    Input in = trial(6.0, 2.0);
    expect(propose(s, in, gradient) == kEvaluate && take(s, in), "accepted");
    settle(s, 1e-6, gradient);
    expect(s.status == kConvergedGradient && s.gradient == 1e-6, "|g| at the tolerance: CONVERGED_GRADIENT");
    State c = started(8.0, cost);
    in = trial(8.0 - 0x1p-17, 0x1p-17);   // (exact in doubles: dF = 2^-17 = 2^-20 x 8)
    expect(propose(c, in, cost) == kEvaluate && take(c, in), "accepted");
    settle(c, 1.0, cost);
    expect(c.status == kConvergedCost, "|dF| = tolerance x F: CONVERGED_COST");
    State c2 = started(8.0, cost);
    in = trial(8.0 - 0x1p-16, 0x1p-16);
    expect(propose(c2, in, cost) == kEvaluate && take(c2, in), "accepted");
    settle(c2, 1.0, cost);
    expect(c2.status == kMaxIterations, "a larger decrease goes on");
    State both = started(8.0, Rules{100, 1e-6, 0x1p-20, 0.0});
    in = trial(8.0 - 0x1p-17, 0x1p-17);
    expect(propose(both, in, off) == kEvaluate && take(both, in), "accepted");
    settle(both, 1e-7, Rules{100, 1e-6, 0x1p-20, 0.0});
    expect(both.status == kConvergedGradient, "the gradient rule comes first");
    State p = started(8.0, step);
    in = trial(6.0, 2.0);
    in.step = 1e-8 * (10.0 + 1e-8);
    expect(propose(p, in, step) == kStopped && p.status == kConvergedStep && p.iterations == 1.0 && p.cost == 8.0, "a step at the tolerance: CONVERGED_STEP before the trial");
    State p2 = started(8.0, step);
    in.step = 2e-7;
    expect(propose(p2, in, step) == kEvaluate, "a longer step goes on");
    State m = started(8.0, count);
    in = trial(9.0, 2.0);
    expect(propose(m, in, count) == kEvaluate && !take(m, in) && iterating(m, count), "one of two");
    expect(propose(m, in, count) == kEvaluate && !take(m, in) && !iterating(m, count) && m.status == kMaxIterations, "two of two: MAX_ITERATIONS");
  }

  // ---- lambda's clamps ----
  {
    State s = started(8.0, off);
    Input in = trial(9.0, 2.0);
    for (int k = 0; k < 40; ++k) (void)(propose(s, in, off) == kEvaluate && take(s, in));
    expect(s.lambda == 1e32 && s.rejected == 40.0, "rejections stop at lambda = 1e32");
    s.lambda = 2e-32;
    in = trial(6.0, 2.0);
    expect(propose(s, in, off) == kEvaluate && take(s, in) && s.lambda == 1e-32, "acceptances stop at lambda = 1e-32");
    s.lambda = 1e32;
    in = trial(s.cost - 0.5, 2.0);   // gain 1/4: x 1.125, clamped
    expect(propose(s, in, off) == kEvaluate && take(s, in) && s.lambda == 1e32, "an acceptance that raises lambda stops at 1e32 too");
  }

  std::printf("%s\n", bad == 0 ? "ok" : "failed");
  return bad == 0 ? 0 : 1;
}
