// Stand-alone check of ndt_2d_amd/csrc/posegraph/ndt2d_posegraph_relative.h: `relative` and
// `distance` on inputs made here from a small generator, printed with their results as hexadecimal
// doubles, one line per call:
//     R <c> <s> <pa 3> <pb 3> <joint 36> <t 3> <cov 9>
//     D <t_pred 3> <cov_pred 9> <t_meas 3> <cov_meas 9> <d2, or "refused">
// tests/test_posegraph_marginals_host.py recomputes every line with the numpy restatement and
// compares bit for bit.  Its own checks: the covariance is symmetric to rounding and positive
// semidefinite on its diagonal, a held pose a (zero aa, ab, ba) gives B bb B^T, a sum that is not
// positive definite is refused and d2 is left alone, d2 >= 0, d2 = 0 for meas = pred.  Built with
// the host compiler (once more with -fsanitize=address,undefined) and run directly; no device, no
// library.  Exits non-zero when a check fails.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "ndt2d_posegraph_relative.h"

namespace P = ndt2d::posegraph;

namespace
{

int failures = 0;
std::uint64_t state = 0x9E3779B97F4A7C15ull;

// a double in [-1, 1) with 20 bits: every product of a few of them is exact enough to print
double next()
{
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<double>(static_cast<std::int64_t>(state >> 44) - (1 << 19)) / static_cast<double>(1 << 19);
}

void check(bool ok, const char * what, int k)
{
  if (!ok)
  {
    std::fprintf(stderr, "FAILED: %s (case %d)\n", what, k);
    ++failures;
  }
}

void print(const double * v, int n)
{
  for (int i = 0; i < n; ++i) std::printf(" %a", v[i]);
}

// a symmetric positive definite n x n (row-major) = G G^T + shift I
void spd(double * out, int n, double scale, double shift)
{
  double G[36];
  for (int i = 0; i < n * n; ++i) G[i] = scale * next();
  for (int i = 0; i < n; ++i)
  {
    for (int j = 0; j < n; ++j)
    {
      double v = i == j ? shift : 0.0;
      for (int k = 0; k < n; ++k) v += G[n * i + k] * G[n * j + k];
      out[n * i + j] = v;
    }
  }
}

}  // namespace

int main()
{
  const double cs[][2] = {{1.0, 0.0}, {0.6, 0.8}, {-0.8, 0.6}, {0.0, -1.0}, {0.28, -0.96}};
  for (int k = 0; k < 20; ++k)
  {
    const double c = cs[k % 5][0], s = cs[k % 5][1];
    double pa[3], pb[3], six[36], joint[36], t[3], cov[9];
    for (int i = 0; i < 3; ++i)
    {
      pa[i] = 4.0 * next();
      pb[i] = 4.0 * next();
    }
    spd(six, 6, 0.1, 0.001);
    // as four 3 x 3 blocks aa ab ba bb; not quite symmetric, as computed columns are not
    for (int i = 0; i < 6; ++i)
    {
      for (int j = 0; j < 6; ++j) joint[9 * (2 * (i / 3) + j / 3) + 3 * (i % 3) + j % 3] = six[6 * i + j] + (i < j ? 1e-9 * next() : 0.0);
    }
    const bool held = k % 4 == 3;
    if (held)
    {
      for (int i = 0; i < 27; ++i) joint[i] = 0.0;
    }
    P::relative(c, s, pa, pb, joint, t, cov);
    std::printf("R %a %a", c, s);
    print(pa, 3);
    print(pb, 3);
    print(joint, 36);
    print(t, 3);
    print(cov, 9);
    std::printf("\n");
    check(t[2] == pb[2] - pa[2], "the heading difference is not wrapped", k);
    for (int i = 0; i < 3; ++i)
    {
      check(cov[4 * i] >= 0.0, "a variance is >= 0", k);
      for (int j = 0; j < i; ++j) check(std::fabs(cov[3 * i + j] - cov[3 * j + i]) <= 1e-14 * (cov[4 * i] + cov[4 * j]), "the covariance is symmetric", k);
    }
    if (held)
    {
      // B bb B^T: the translation block is bb's rotated into a's frame, the heading's variance bb's own
      const double * bb = joint + 27;
      check(std::fabs(cov[8] - bb[8]) <= 1e-15 * std::fabs(bb[8]), "a held: the heading variance is b's", k);
      check(std::fabs((cov[0] + cov[4]) - (bb[0] + bb[4])) <= 1e-14 * (bb[0] + bb[4]), "a held: the trace of the translation block is b's", k);
    }
  }
  for (int k = 0; k < 20; ++k)
  {
    double tp[3], tm[3], cp[9], cm[9], d2 = -7.0;
    for (int i = 0; i < 3; ++i)
    {
      tp[i] = 3.0 * next();
      tm[i] = k == 5 ? tp[i] : tp[i] + (i == 2 && k % 3 == 0 ? 6.0 : 0.2) * next();   // (some heading differences beyond pi)
    }
    spd(cp, 3, 0.2, 0.001);
    spd(cm, 3, 0.1, 0.0005);
    const bool indefinite = k == 11 || k == 17;
    if (indefinite) cm[k == 11 ? 0 : 8] = -1.0;
    const bool ok = P::distance(tp, cp, tm, cm, &d2);
    std::printf("D");
    print(tp, 3);
    print(cp, 9);
    print(tm, 3);
    print(cm, 9);
    if (ok) std::printf(" %a\n", d2);
    else std::printf(" refused\n");
    check(ok != indefinite, "a sum that is not positive definite is refused, any other is not", k);
    check(ok ? d2 >= 0.0 : d2 == -7.0, "d2 >= 0, and left alone by a refusal", k);
    if (k == 5) check(d2 == 0.0, "meas = pred: d2 = 0", k);
  }
  if (failures != 0) return EXIT_FAILURE;
  std::printf("ok\n");
  return EXIT_SUCCESS;
}
