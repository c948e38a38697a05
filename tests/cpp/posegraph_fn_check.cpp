// Stand-alone check of ndt_2d_amd/csrc/posegraph/ndt2d_posegraph_fn.h: Normalize on and round its
// edges, the analytic Jacobians and the products the solver makes of them against central
// differences, the symmetric inverse, and the host's Cholesky with its refusals.  Built with the
// host compiler (once more with -fsanitize=address,undefined) and run directly; no device, no
// library.  Prints one line per Normalize case ("N <v hex> <result hex>") for
// tests/test_posegraph_host.py to compare with the restatement bit for bit; exits non-zero on the
// first check that fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "ndt2d_posegraph_fn.h"

namespace P = ndt2d::posegraph;

namespace
{

int failures = 0;

void check(bool ok, const char * what)
{
  if (!ok)
  {
    std::fprintf(stderr, "FAILED: %s\n", what);
    ++failures;
  }
}

// e of the constraint with transform t between the poses pa and pb.
void residual(const double * pa, const double * pb, const double * t, double * e)
{
  const P::Frame f = P::frame(std::cos(pa[2]), std::sin(pa[2]), pa, pb);
  P::error(f, pa[2], pb[2], t, e);
}

}  // namespace

int main()
{
  // ---- Normalize ----
  const double pi = P::kPi;
  const double cases[] = {-pi, pi, std::nextafter(pi, 0.0), 3.0 * pi, -3.0 * pi, 1e6, 0.0, -0.0, 0.3, -2.9, 6.5, std::nextafter(-pi, 0.0),
                          std::nextafter(-pi, -4.0), 2.0 * pi, -1e6};
  for (double v : cases)
  {
    const double r = P::normalize(v);
    std::printf("N %a %a\n", v, r);
    // the range is [-pi, pi) up to the formula's own rounding
    check(r >= -pi - 4e-16 && r < pi, "normalize: range");
    check(std::fabs(std::remainder(r - v, 2.0 * pi)) <= 1e-9 * std::fmax(1.0, std::fabs(v)), "normalize: a multiple of 2 pi away");
  }
  check(P::normalize(-pi) == -pi, "normalize(-pi) == -pi");
  check(P::normalize(pi) == -pi, "normalize(pi) == -pi");
  check(P::normalize(0.0) == 0.0, "normalize(0) == 0");

  // ---- the Jacobians against central differences, h = 1e-6: tolerance 1e-7 relative ----
  const double poses[][6] = {{0.3, -0.2, 0.4, 1.3, 0.2, 0.1}, {-4.0, 2.5, 2.9, -3.1, 2.0, -2.7}, {10.0, 10.0, 7.5, 9.0, 12.0, 8.0},
                             {0.0, 0.0, 0.0, 1.0, 0.0, 0.0}};
  const double t[3] = {1.0, 0.5, 0.3};
  for (const auto & pp : poses)
  {
    const double * pa = pp, * pb = pp + 3;
    const P::Frame f = P::frame(std::cos(pa[2]), std::sin(pa[2]), pa, pb);
    double A[9], B[9];
    P::jacobian_a(f, A);
    P::jacobian_b(f, B);
    const double h = 1e-6;
    for (int j = 0; j < 6; ++j)
    {
      double hi[6], lo[6], eh[3], el[3];
      for (int k = 0; k < 6; ++k) hi[k] = lo[k] = pp[k];
      hi[j] += h;
      lo[j] -= h;
      residual(hi, hi + 3, t, eh);
      residual(lo, lo + 3, t, el);
      for (int i = 0; i < 3; ++i)
      {
        const double numeric = (eh[i] - el[i]) / (2.0 * h);
        const double analytic = j < 3 ? A[3 * i + j] : B[3 * i + (j - 3)];
        check(std::fabs(numeric - analytic) <= 1e-7 * std::fmax(1.0, std::fabs(analytic)), "jacobian against central differences");
      }
    }
    // the products without the blocks
    const double v[3] = {0.7, -1.1, 0.45};
    double y[3], z[3];
    P::apply_a(f, v, y);
    P::mul(A, v, z);
    for (int i = 0; i < 3; ++i) check(std::fabs(y[i] - z[i]) <= 1e-14 * (1.0 + std::fabs(z[i])), "apply_a == A v");
    P::apply_b(f, v, y);
    P::mul(B, v, z);
    for (int i = 0; i < 3; ++i) check(std::fabs(y[i] - z[i]) <= 1e-14 * (1.0 + std::fabs(z[i])), "apply_b == B v");
    P::apply_at(f, v, y);
    P::mul_t(A, v, z);
    for (int i = 0; i < 3; ++i) check(std::fabs(y[i] - z[i]) <= 1e-14 * (1.0 + std::fabs(z[i])), "apply_at == A^T v");
    P::apply_bt(f, v, y);
    P::mul_t(B, v, z);
    for (int i = 0; i < 3; ++i) check(std::fabs(y[i] - z[i]) <= 1e-14 * (1.0 + std::fabs(z[i])), "apply_bt == B^T v");
    // J^T J of the weighted block, and its inverse
    const double W[9] = {10.0, 0.0, 0.0, 1.0, 8.9, 0.0, 0.5, -0.95, 19.97};
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, inv[6], unit[3];
    P::add_jtj(W, A, S);
    double J[9];
    for (int i = 0; i < 3; ++i)
    {
      for (int j = 0; j < 3; ++j) J[3 * i + j] = W[3 * i] * A[j] + W[3 * i + 1] * A[3 + j] + W[3 * i + 2] * A[6 + j];
    }
    double Jv[3], JtJv[3], Sv[3];
    P::mul(J, v, Jv);
    P::mul_t(J, Jv, JtJv);
    P::mul_sym(S, v, Sv);
    for (int i = 0; i < 3; ++i) check(std::fabs(Sv[i] - JtJv[i]) <= 1e-12 * (1.0 + std::fabs(JtJv[i])), "add_jtj == J^T J");
    check(P::invert_sym(S, inv), "invert_sym of a definite block");
    P::mul_sym(inv, Sv, unit);
    for (int i = 0; i < 3; ++i) check(std::fabs(unit[i] - v[i]) <= 1e-9, "invert_sym inverts");
  }
  const double singular[6] = {1.0, 1.0, 0.0, 1.0, 0.0, 0.0};
  double out[6];
  check(!P::invert_sym(singular, out) && out[0] == 0.0 && out[5] == 0.0, "invert_sym refuses a singular block");

  // ---- the Cholesky and its refusals ----
  const double info[9] = {100.0, 10.0, 5.0, 10.0, 80.0, -8.0, 5.0, -8.0, 400.0};
  double L[9];
  check(P::cholesky_lower(info, L), "cholesky of a definite matrix");
  check(L[1] == 0.0 && L[2] == 0.0 && L[5] == 0.0, "cholesky: lower");
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j)
    {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += L[3 * i + k] * L[3 * j + k];
      check(std::fabs(s - info[3 * i + j]) <= 1e-12 * 400.0, "L L^T == information");
    }
  }
  const double zeros[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double indefinite[9] = {1.0, 2.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  const double negative[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0};
  const double semi[9] = {1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  const double nan_pivot[9] = {1.0, 0.0, 0.0, 0.0, NAN, 0.0, 0.0, 0.0, 1.0};
  const double huge[9] = {INFINITY, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  check(!P::cholesky_lower(zeros, L), "cholesky refuses zeros");
  check(!P::cholesky_lower(indefinite, L), "cholesky refuses an indefinite matrix");
  check(!P::cholesky_lower(negative, L), "cholesky refuses a negative pivot");
  check(!P::cholesky_lower(semi, L), "cholesky refuses a semi-definite matrix");
  check(!P::cholesky_lower(nan_pivot, L), "cholesky refuses a NaN pivot");
  check(!P::cholesky_lower(huge, L), "cholesky refuses an infinite pivot");

  if (failures != 0)
  {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
