// Stand-alone check of ndt_2d_amd/csrc/posegraph/ndt2d_posegraph_fn.h: Normalize on and round its
// edges, the analytic Jacobians and the products the solver makes of them against central
// differences, the symmetric inverse, and the host's Cholesky with its refusals.  Built with the
// host compiler (once more with -fsanitize=address,undefined) and run directly; no device, no
// library.  The 3 x 3 inverses of the preconditioners (invert_sym, and the chain's invert_spd) at
// their limit: blocks Q diag(1, sqrt(kappa), kappa) Q^T for kappa = 1e3 ... 1e15 and the diagonal
// blocks of H of the graphs of tests/posegraph_hard_cases.py (posegraph_hard_blocks.h) against a
// long double Cholesky inverse; prints the kappa at which each first breaks down, and that of the cofactor
// form invert_sym was before, of which a copy is kept here for that ("K ...").
// Prints one line per Normalize case ("N <v hex> <result hex>") for
// tests/test_posegraph_host.py to compare with the restatement bit for bit; exits non-zero on the
// first check that fails.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "ndt2d_posegraph_chain.h"
#include "ndt2d_posegraph_fn.h"
#include "posegraph_hard_blocks.h"

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

// The inverse of the symmetric 3 x 3 S (00, 01, 02, 11, 12, 22) by a Cholesky factorisation in long double,
// same storage; false where a pivot is not positive.
bool reference_inverse(const double * S, long double * out)
{
  const long double a[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
  long double L[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, T[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int j = 0; j < 3; ++j)
  {
    long double d = a[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0L)) return false;
    L[j][j] = sqrtl(d);
    for (int i = j + 1; i < 3; ++i)
    {
      long double v = a[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int c = 0; c < 3; ++c)   // T = L^-1, column by column
  {
    T[c][c] = 1.0L / L[c][c];
    for (int r = c + 1; r < 3; ++r)
    {
      long double v = 0.0L;
      for (int k = c; k < r; ++k) v -= L[r][k] * T[k][c];
      T[r][c] = v / L[r][r];
    }
  }
  const int at[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
  for (int e = 0; e < 6; ++e)
  {
    long double v = 0.0L;
    for (int k = 0; k < 3; ++k) v += T[k][at[e][0]] * T[k][at[e][1]];
    out[e] = v;
  }
  return true;
}

// Positive definite as its own Cholesky tells (the symmetric storage).
bool definite(const double * S)
{
  const double full[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]};
  double L[9];
  return P::cholesky_lower(full, L);
}

// The cofactor inverse invert_sym was until DESIGN.md 3.18.8, kept here so that its recorded break-down stays
// reproducible: out = adj(S) / det, refused (zeroed) where det is not a positive finite number.
bool cofactor_inverse(const double * S, double * out)
{
  const double c00 = S[3] * S[5] - S[4] * S[4];
  const double c01 = S[2] * S[4] - S[1] * S[5];
  const double c02 = S[1] * S[4] - S[2] * S[3];
  const double det = S[0] * c00 + S[1] * c01 + S[2] * c02;
  if (!(det > 0.0) || !(det <= 1.7976931348623157e308))
  {
    for (int i = 0; i < 6; ++i) out[i] = 0.0;
    return false;
  }
  const double inv = 1.0 / det;
  out[0] = c00 * inv;
  out[1] = c01 * inv;
  out[2] = c02 * inv;
  out[3] = (S[0] * S[5] - S[2] * S[2]) * inv;
  out[4] = (S[1] * S[2] - S[0] * S[4]) * inv;
  out[5] = (S[0] * S[3] - S[1] * S[1]) * inv;
  return true;
}

enum Verdict { kGood, kRefused, kIndefinite };
enum Form { kSym, kSpd, kCofactor };

// One of the two inverses on a definite block: what it returned, and the error of a returned inverse
// relative to the largest entry of the reference.
Verdict run(int form, const double * S, double * relative_error)
{
  double out[6];
  long double ref[6];
  *relative_error = 0.0;
  if (!reference_inverse(S, ref)) return kRefused;   // (not reached: the callers pass definite blocks)
  const bool ok = form == kSpd ? ndt2d::posegraph::chain::invert_spd(S, out) : (form == kSym ? P::invert_sym(S, out) : cofactor_inverse(S, out));
  if (!ok)
  {
    for (int i = 0; i < 6; ++i) check(out[i] == 0.0, "a refused block is zeroed");
    return kRefused;
  }
  long double worst = 0.0L, scale = 0.0L;
  for (int i = 0; i < 6; ++i)
  {
    worst = fmaxl(worst, fabsl((long double)out[i] - ref[i]));
    scale = fmaxl(scale, fabsl(ref[i]));
  }
  *relative_error = (double)(worst / scale);
  return definite(out) ? kGood : kIndefinite;
}

// Q diag(1, sqrt(kappa), kappa) Q^T, Q a turn by a about z behind a turn by b about x, formed in long
// double and rounded once: symmetric storage.
void designed_block(double kappa, double a, double b, double * S)
{
  const long double ca = cosl(a), sa = sinl(a), cb = cosl(b), sb = sinl(b);
  const long double Q[3][3] = {{ca, -sa * cb, sa * sb}, {sa, ca * cb, -ca * sb}, {0.0L, sb, cb}};
  const long double d[3] = {1.0L, sqrtl((long double)kappa), (long double)kappa};
  const int at[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
  for (int e = 0; e < 6; ++e)
  {
    long double v = 0.0L;
    for (int k = 0; k < 3; ++k) v += Q[at[e][0]][k] * d[k] * Q[at[e][1]][k];
    S[e] = (double)v;
  }
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

  // ---- the two 3 x 3 inverses at their limit ----
  // A returned inverse must be positive definite and within 100 kappa 2^-53 of the long double one, and a
  // definite block must not be refused: asserted up to kappa = 1e12 (where the long double reference still
  // has three digits to spare) and for every block of a hard case.  The kappa of the first miss of the
  // bound, of the first indefinite inverse and of the first refusal are printed, and the first of them must
  // lie beyond what the hard cases' blocks reach.  (The cofactor form this inverse replaced summed the
  // determinant, kappa^1.5, from products of size kappa^3: it missed the bound from kappa = 1e8, refused
  // definite blocks from 1e12 and returned indefinite inverses from 1e14.)
  const double turns[][2] = {{0.0, 0.0}, {0.37, 0.2}, {1.1, -0.7}, {2.6, 1.3}};
  const double eps53 = 1.1102230246251565e-16;
  const char * names[3] = {"invert_sym", "invert_spd", "the cofactor form (no longer in the product)"};
  double broke[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};   // [form][bound, indefinite, refused]
  int swept = 0, not_definite = 0;
  for (int decade = 3; decade <= 15; ++decade)
  {
    const double kappa = std::pow(10.0, decade);
    for (const auto & turn : turns)
    {
      double S[6], err;
      designed_block(kappa, turn[0], turn[1], S);
      ++swept;
      if (!definite(S))   // (rounded to doubles, the block itself is no longer definite)
      {
        ++not_definite;
        continue;
      }
      for (int form = 0; form < 3; ++form)
      {
        const Verdict v = run(form, S, &err);
        const bool within = v == kRefused || err <= 100.0 * kappa * eps53;
        if (!within && broke[form][0] == 0.0) broke[form][0] = kappa;
        if (v == kIndefinite && broke[form][1] == 0.0) broke[form][1] = kappa;
        if (v == kRefused && broke[form][2] == 0.0) broke[form][2] = kappa;
        if (form != kCofactor && decade <= 12) check(v == kGood && within, form == kSpd ? "invert_spd up to kappa 1e12" : "invert_sym up to kappa 1e12");
      }
    }
  }
  std::printf("K %d designed blocks, %d of them skipped: not definite once rounded to doubles\n", swept, not_definite);
  check(not_definite == 0, "every designed block is definite in doubles");
  double first[3];
  for (int form = 0; form < 3; ++form)
  {
    first[form] = 0.0;
    for (double k : broke[form])
    {
      if (k != 0.0 && (first[form] == 0.0 || k < first[form])) first[form] = k;
    }
    std::printf("K %s: beyond 100 kappa 2^-53 first at kappa %g, an indefinite inverse first at %g, a definite block refused first at %g (0: not up to 1e15)\n",
                names[form], broke[form][0], broke[form][1], broke[form][2]);
  }
  // the cofactor form's record: what the replacement is measured against
  check(broke[kCofactor][0] == 1e8 && broke[kCofactor][2] == 1e12 && broke[kCofactor][1] == 1e14, "the cofactor form breaks down where it is recorded to");
  double hard_kappa = 0.0;
  for (const HardBlock & b : kHardBlocks)
  {
    check(definite(b.S), "a hard case's block is definite");
    long double ref[6];
    reference_inverse(b.S, ref);
    // kappa from below: |S|_max |S^-1|_max
    long double smax = 0.0L, imax = 0.0L;
    for (int i = 0; i < 6; ++i)
    {
      smax = fmaxl(smax, fabsl((long double)b.S[i]));
      imax = fmaxl(imax, fabsl(ref[i]));
    }
    const double kappa = (double)(smax * imax);
    hard_kappa = std::fmax(hard_kappa, kappa);
    for (int chain = 0; chain < 2; ++chain)
    {
      double err;
      const Verdict v = run(chain, b.S, &err);
      if (v != kGood || err > 100.0 * kappa * eps53)
      {
        std::fprintf(stderr, "%s node %d lambda %g: verdict %d, error %.3e at kappa %.3e\n", b.graph, b.node, b.lambda, (int)v, err, kappa);
      }
      check(v != kRefused, "a hard case's definite block is not refused");
      check(v != kIndefinite, "a hard case's block: the returned inverse is positive definite");
      check(err <= 100.0 * kappa * eps53, "a hard case's block: within 100 kappa 2^-53 of the long double inverse");
    }
  }
  std::printf("K the hard cases' blocks reach kappa %.1e\n", hard_kappa);
  check(first[0] == 0.0 || first[0] > hard_kappa, "invert_sym breaks down beyond the hard cases' blocks");
  check(first[1] == 0.0 || first[1] > hard_kappa, "invert_spd breaks down beyond the hard cases' blocks");

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
