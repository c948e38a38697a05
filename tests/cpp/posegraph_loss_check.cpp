// Stand-alone check of ndt_2d_amd/csrc/posegraph/ndt2d_posegraph_loss.h: rho' against central
// differences of rho and rho'' against central differences of rho', rho'' <= 0 and rho' > 0, rho
// rising and rho' falling with s, the trivial loss, Huber's two branches meeting at s = b, and the
// refusal of a kind there is none of.  Built with the host compiler (once more with
// -fsanitize=address,undefined) and run directly; no device, no library.  Prints one line per
// loss and scale ("L <kind> <scale> <worst relative difference of rho'> <of rho''>"); exits
// non-zero when a check fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "ndt2d_posegraph_loss.h"

namespace P = ndt2d::posegraph;

namespace
{

int failures = 0;

void check(bool ok, const char * what, int kind, double a, double s)
{
  if (!ok)
  {
    std::fprintf(stderr, "FAILED: %s (kind %d, scale %g, s %.17g)\n", what, kind, a, s);
    ++failures;
  }
}

}  // namespace

int main()
{
  const double scales[] = {0.05, 1.0, 1.345, 30.0};
  for (int kind : {P::kLossTrivial, P::kLossHuber, P::kLossCauchy})
  {
    for (double a : scales)
    {
      const double b = a * a;
      double worst1 = 0.0, worst2 = 0.0, last[3] = {-1.0, 2.0, 0.0};
      // s over twelve decades round b, 40 points a decade
      for (int k = -240; k <= 240; ++k)
      {
        const double s = b * std::pow(10.0, k / 40.0);
        double at[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0}, lo[3] = {0.0, 0.0, 0.0};
        check(P::loss_evaluate(kind, a, s, at), "evaluate", kind, a, s);
        check(std::isfinite(at[0]) && at[0] >= 0.0, "rho is finite and >= 0", kind, a, s);
        check(at[1] > 0.0 && at[1] <= 1.0, "0 < rho' <= 1", kind, a, s);
        check(at[2] <= 0.0, "rho'' <= 0", kind, a, s);
        check(at[0] <= s * (1.0 + 4.0 * 2.220446049250313e-16), "rho <= s", kind, a, s);
        check(at[0] > last[0], "rho rises with s", kind, a, s);
        check(at[1] <= last[1], "rho' falls with s", kind, a, s);
        last[0] = at[0];
        last[1] = at[1];
        // central differences with h = 1e-4 s: their own error is 1e-8 relative, rounding 1e-12;
        // not across Huber's kink at s = b
        const double h = 1e-4 * s;
        if (kind == P::kLossHuber && s - h <= b && s + h >= b) continue;
        P::loss_evaluate(kind, a, s + h, hi);
        P::loss_evaluate(kind, a, s - h, lo);
        const double d1 = (hi[0] - lo[0]) / ((s + h) - (s - h)), d2 = (hi[1] - lo[1]) / ((s + h) - (s - h));
        const double e1 = std::fabs(d1 - at[1]) / at[1];
        const double e2 = std::fabs(d2 - at[2]) / std::fmax(std::fabs(at[2]), 1e-3 * at[1] / s);   // (where rho'' is far below rho' / s the difference's rounding is what is left)
        worst1 = std::fmax(worst1, e1);
        worst2 = std::fmax(worst2, e2);
        check(e1 <= 1e-6, "rho' is the derivative of rho", kind, a, s);
        check(e2 <= 1e-6, "rho'' is the derivative of rho'", kind, a, s);
      }
      std::printf("L %d %g %.3e %.3e\n", kind, a, worst1, worst2);
      double out[3] = {0.0, 0.0, 0.0};
      P::loss_evaluate(kind, a, 0.0, out);
      check(out[0] == 0.0 && out[1] == 1.0, "rho(0) = 0, rho'(0) = 1", kind, a, 0.0);
      if (kind == P::kLossTrivial)
      {
        P::loss_evaluate(kind, a, 7.5, out);
        check(out[0] == 7.5 && out[1] == 1.0 && out[2] == 0.0, "trivial: rho = s", kind, a, 7.5);
      }
      if (kind == P::kLossHuber)
      {
        double up[3] = {0.0, 0.0, 0.0};
        P::loss_evaluate(kind, a, b, out);
        P::loss_evaluate(kind, a, std::nextafter(b, INFINITY), up);
        check(out[0] == b && out[1] == 1.0 && out[2] == 0.0, "huber: s = b is the quadratic branch", kind, a, b);
        check(std::fabs(up[0] - b) <= 4.0 * 2.220446049250313e-16 * b && up[1] <= 1.0 && up[1] >= 1.0 - 4.0 * 2.220446049250313e-16,
              "huber: the branches meet at b", kind, a, b);
      }
      // far out (s / b still a finite number) rho is finite, and rho' stays positive wherever s is
      P::loss_evaluate(kind, a, 1e300, out);
      check(out[1] > 0.0 && std::isfinite(out[0]) && out[2] <= 0.0, "rho finite and rho' > 0 at s = 1e300", kind, a, 1e300);
      P::loss_evaluate(kind, a, 1.7e308, out);
      check(out[1] > 0.0 && out[2] <= 0.0, "rho' > 0 at the largest s", kind, a, 1.7e308);
    }
  }
  double out[3] = {0.0, 0.0, 0.0};
  if (P::loss_evaluate(3, 1.0, 1.0, out) || P::loss_evaluate(-1, 1.0, 1.0, out))
  {
    std::fprintf(stderr, "FAILED: a kind there is none of is refused\n");
    ++failures;
  }
  if (failures != 0) return EXIT_FAILURE;
  std::printf("ok\n");
  return EXIT_SUCCESS;
}
