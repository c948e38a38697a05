// Host-only check of the covariance of the Newton NDT registration
// (ndt_2d_amd/csrc/refine/ndt2d_refine_step.h, covariance()): H^-1 by the 3 x 3 Cholesky on
// diagonal, well and badly conditioned positive-definite matrices, and the refusals -- indefinite,
// singular, zero, NaN and infinite entries, an inverse that overflows -- which must leave the
// output untouched.  Every accepted inverse is printed in hexadecimal ("cov H.. -> c.."):
// tests/test_refine_neighbours_host.py compares those bits with the restatement's.  A program of
// its own, built with the host compiler and the sanitizers.
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

static void check_inverse(const double (&H)[6])
{
  double c[9];
  for (double & v : c) v = -7.0;
  expect(covariance(H, c), "a positive-definite matrix is inverted");
  std::printf("cov %a %a %a %a %a %a -> %a %a %a %a %a %a %a %a %a\n", H[0], H[1], H[2], H[3], H[4], H[5], c[0], c[1], c[2], c[3],
              c[4], c[5], c[6], c[7], c[8]);
  expect(c[1] == c[3] && c[2] == c[6] && c[5] == c[7], "the inverse is symmetric bit for bit");
  // H cov = 1, against the size of the products (the residual grows with the condition number:
  // 1e6 x 2^-53 = 1e-10 for the last matrix below)
  const double A[3][3] = {{H[0], H[1], H[2]}, {H[1], H[3], H[4]}, {H[2], H[4], H[5]}};
  for (int r = 0; r < 3; ++r)
  {
    for (int k = 0; k < 3; ++k)
    {
      double sum = 0.0, size = 0.0;
      for (int j = 0; j < 3; ++j)
      {
        sum += A[r][j] * c[3 * j + k];
        size += std::fabs(A[r][j] * c[3 * j + k]);
      }
      expect(std::fabs(sum - (r == k ? 1.0 : 0.0)) <= 1e-9 * size, "H times its inverse is the unit matrix");
    }
  }
}

static void check_refused(const double (&H)[6], const char * what)
{
  double c[9];
  for (int k = 0; k < 9; ++k) c[k] = 3.0 + k;
  bool untouched = !covariance(H, c);
  for (int k = 0; k < 9; ++k) untouched = untouched && c[k] == 3.0 + k;
  expect(untouched, what);
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double inf = std::numeric_limits<double>::infinity();

  // diagonal, pivots with exact square roots: exact reciprocals
  {
    const double H[6] = {4.0, 0.0, 0.0, 16.0, 0.0, 0.25};
    double c[9];
    expect(covariance(H, c) && c[0] == 0.25 && c[4] == 0.0625 && c[8] == 4.0, "diagonal: exact reciprocals");
    expect(c[1] == 0.0 && c[2] == 0.0 && c[5] == 0.0 && c[3] == 0.0 && c[6] == 0.0 && c[7] == 0.0, "diagonal: no off-diagonal entry");
  }

  // positive definite: the sizes a 100-beam and a 720-beam scan give, and a badly conditioned one
  const double pd[][6] = {{4.0, 1.0, 0.5, 3.0, 0.2, 2.0},
                          {91234.5 / 3.0, -1234.25 / 7.0, 17.0 / 3.0, 60321.0 / 7.0, 4000.0 / 9.0, 1.0e6 / 3.0},
                          {1.0 / 3.0, 1.0 / 7.0, -1.0 / 9.0, 2.0 / 3.0, 1.0 / 11.0, 5.0 / 7.0},
                          {1e-3, 2e-4, -1e-4, 3e-3, 1e-5, 7e-2},
                          {1.0e4, 99.0, 10.0, 1.0, 0.0, 1.0}};
  for (const auto & H : pd) check_inverse(H);

  // the refusals
  check_refused({-1.0, 0.0, 0.0, 2.0, 0.0, 3.0}, "a negative first pivot is refused");
  check_refused({1.0, 2.0, 0.0, 1.0, 0.0, 1.0}, "an indefinite matrix is refused");
  check_refused({1.0, 0.0, 0.0, 1.0, 2.0, 1.0}, "a negative last pivot is refused");
  check_refused({1.0, 1.0, 0.0, 1.0, 0.0, 1.0}, "a singular matrix is refused");
  check_refused({0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, "the zero matrix is refused");
  check_refused({nan, 0.0, 0.0, 1.0, 0.0, 1.0}, "a NaN on the diagonal is refused");
  check_refused({1.0, 0.0, nan, 1.0, 0.0, 1.0}, "a NaN off the diagonal is refused");
  check_refused({1.0, 0.0, 0.0, 1.0, 0.0, nan}, "a NaN in the last entry is refused");
  check_refused({inf, 0.0, 0.0, 1.0, 0.0, 1.0}, "an infinite entry is refused");
  check_refused({1.0, 0.0, 0.0, 1.0, -inf, 1.0}, "a negative infinite entry is refused");
  check_refused({1e-320, 0.0, 0.0, 1.0, 0.0, 1.0}, "an inverse that overflows is refused");

  std::printf(bad == 0 ? "OK\n" : "FAILED\n");
  return bad == 0 ? 0 : 1;
}
