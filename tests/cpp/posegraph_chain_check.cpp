// Stand-alone check of ndt_2d_amd/csrc/posegraph/ndt2d_posegraph_chain.h: the header's sequential
// drivers (the per-node steps the kernel runs, level by level) on random symmetric positive definite
// block-tridiagonal systems against a Cholesky written here.  Built with the host compiler (once
// more with -fsanitize=address,undefined) and run directly; no device, no library.  Prints one line
// per system ("S <n> <cuts> <relative residual> <difference to the Cholesky>") and "ok"; exits
// non-zero when a check fails.
//
// The systems.  M = sum over the edges (i, i + 1) of [A_i B_i]^T [A_i B_i] + I with A_i, B_i random in
// [-1, 1]^(3 x 3): J^T J of a chain plus the identity, as the solver's band is.  Its eigenvalues lie in
// [1, 1 + 4 x 9], so the condition number is below 40 and both the reduction and the Cholesky carry a
// relative error of a few dozen eps: the bounds are |M z - r|_2 <= 1e-12 |r|_2 (what the solver needs of
// a preconditioner, with three orders to spare over 64 eps x 40) and |z - z_chol|_inf <= 1e-10 |z_chol|_inf.
// Edges are cut (A_i = B_i = 0) at chosen places, which leaves decoupled segments, of one node too.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ndt2d_posegraph_chain.h"

namespace P = ndt2d::posegraph;
namespace CH = ndt2d::posegraph::chain;

namespace
{

int failures = 0;

void check(bool ok, const char * what, size_t n)
{
  if (!ok)
  {
    std::fprintf(stderr, "FAILED: %s (n = %zu)\n", what, n);
    ++failures;
  }
}

// (a small generator of its own: the same systems everywhere)
uint64_t state = 0x9e3779b97f4a7c15ull;

double uniform()
{
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<double>(state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

struct Blocks
{
  size_t n;
  std::vector<double> D;   // [n][6]
  std::vector<double> U;   // [n][9] the block (i, i + 1); the last is zero
};

// S += the upper triangle of the row-major X.
void add_sym(const double * X, double * S)
{
  S[0] += X[0]; S[1] += X[1]; S[2] += X[2];
  S[3] += X[4]; S[4] += X[5]; S[5] += X[8];
}

// cut: 0 none, 1 every third edge, 2 edges 0 and 1 and the last (segments of one node at both ends),
// 3 every edge (n segments of one node)
Blocks make(size_t n, int cut)
{
  Blocks m{n, std::vector<double>(6 * n, 0.0), std::vector<double>(9 * n, 0.0)};
  for (size_t i = 0; i < n; ++i) m.D[6 * i] = m.D[6 * i + 3] = m.D[6 * i + 5] = 1.0;
  for (size_t i = 0; i + 1 < n; ++i)
  {
    double A[9], B[9], X[9];
    for (int k = 0; k < 9; ++k) A[k] = uniform();
    for (int k = 0; k < 9; ++k) B[k] = uniform();
    const bool gone = cut == 3 || (cut == 1 && i % 3 == 1) || (cut == 2 && (i <= 1 || i + 2 == n));
    if (gone) continue;
    CH::mtm(A, A, X);
    add_sym(X, m.D.data() + 6 * i);
    CH::mtm(B, B, X);
    add_sym(X, m.D.data() + 6 * (i + 1));
    CH::mtm(A, B, m.U.data() + 9 * i);
  }
  return m;
}

// y = M v of the blocks.
void product(const Blocks & m, const std::vector<double> & v, std::vector<double> & y)
{
  y.assign(3 * m.n, 0.0);
  for (size_t i = 0; i < m.n; ++i)
  {
    double t[3];
    P::mul_sym(m.D.data() + 6 * i, v.data() + 3 * i, t);
    for (int k = 0; k < 3; ++k) y[3 * i + k] += t[k];
    if (i + 1 < m.n)
    {
      P::mul(m.U.data() + 9 * i, v.data() + 3 * (i + 1), t);
      for (int k = 0; k < 3; ++k) y[3 * i + k] += t[k];
      P::mul_t(m.U.data() + 9 * i, v.data() + 3 * i, t);
      for (int k = 0; k < 3; ++k) y[3 * (i + 1) + k] += t[k];
    }
  }
}

// The lower triangle of M in rows of w + 1 entries: a[r][k] = M[r][r - k].  w = 3 n - 1 is the whole
// triangle (a dense Cholesky), w = 5 the band of a block-tridiagonal matrix.
struct Lower
{
  size_t rows, w;
  std::vector<double> a;
  double & at(size_t r, size_t c) { return a[r * (w + 1) + (r - c)]; }
};

Lower lower_of(const Blocks & m, size_t w)
{
  Lower l{3 * m.n, w, std::vector<double>(3 * m.n * (w + 1), 0.0)};
  static const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  for (size_t i = 0; i < m.n; ++i)
  {
    for (int r = 0; r < 3; ++r)
    {
      for (int c = 0; c <= r; ++c) l.at(3 * i + r, 3 * i + c) = m.D[6 * i + sym[r][c]];
      if (i + 1 < m.n)
      {
        for (int c = 0; c < 3; ++c) l.at(3 * (i + 1) + r, 3 * i + c) = m.U[9 * i + 3 * c + r];   // (the block (i + 1, i) = U^T)
      }
    }
  }
  return l;
}

// Cholesky in place and the solve; false at a pivot that is not positive.
bool cholesky_solve(Lower & l, std::vector<double> & v)
{
  const size_t n = l.rows, w = l.w;
  for (size_t j = 0; j < n; ++j)
  {
    const size_t k0 = j > w ? j - w : 0;
    double d = l.at(j, j);
    for (size_t k = k0; k < j; ++k) d -= l.at(j, k) * l.at(j, k);
    if (!(d > 0.0)) return false;
    const double root = std::sqrt(d);
    l.at(j, j) = root;
    for (size_t i = j + 1; i < n && i <= j + w; ++i)
    {
      const size_t i0 = i > w ? i - w : 0;
      double s = l.at(i, j);
      for (size_t k = i0 > k0 ? i0 : k0; k < j; ++k) s -= l.at(i, k) * l.at(j, k);
      l.at(i, j) = s / root;
    }
  }
  for (size_t i = 0; i < n; ++i)
  {
    double s = v[i];
    for (size_t k = i > w ? i - w : 0; k < i; ++k) s -= l.at(i, k) * v[k];
    v[i] = s / l.at(i, i);
  }
  for (size_t i = n; i-- > 0;)
  {
    double s = v[i];
    for (size_t k = i + 1; k < n && k <= i + w; ++k) s -= l.at(k, i) * v[k];
    v[i] = s / l.at(i, i);
  }
  return true;
}

double norm2(const std::vector<double> & v)
{
  double s = 0.0;
  for (double x : v) s += x * x;
  return std::sqrt(s);
}

// The header's driver on a copy of the blocks; false: a pivot was reported.
bool reduce_solve(const Blocks & m, const std::vector<double> & r, std::vector<double> & z, std::vector<double> * pivots = nullptr)
{
  const size_t n = m.n;
  std::vector<double> D = m.D, U = m.U, L(9 * n, 0.0), Pi(6 * n, 0.0), b = r;
  const CH::System sys{D.data(), U.data(), L.data(), Pi.data()};
  z.assign(3 * n, 0.0);
  const bool ok = CH::factor(sys, n);
  CH::solve(sys, n, b.data(), z.data());
  if (pivots != nullptr) *pivots = Pi;
  return ok;
}

void run(size_t n, int cut)
{
  const Blocks m = make(n, cut);
  std::vector<double> r(3 * n), z, y, zc;
  for (double & v : r) v = uniform();
  check(reduce_solve(m, r, z), "the reduction reported a pivot of a positive definite system", n);
  product(m, z, y);
  for (size_t i = 0; i < 3 * n; ++i) y[i] -= r[i];
  const double residual = norm2(y) / norm2(r);
  // the Cholesky: the whole triangle where that is small, the band beyond (and both at 33: they agree)
  zc = r;
  Lower l = lower_of(m, n <= 33 ? 3 * n - 1 : 5);
  check(cholesky_solve(l, zc), "the Cholesky met a pivot <= 0", n);
  if (n == 33)
  {
    std::vector<double> zb = r;
    Lower band = lower_of(m, 5);
    check(cholesky_solve(band, zb), "the band Cholesky met a pivot <= 0", n);
    for (size_t i = 0; i < 3 * n; ++i) check(std::fabs(zb[i] - zc[i]) <= 1e-13 * (1.0 + std::fabs(zc[i])), "band and dense Cholesky differ", n);
  }
  double diff = 0.0, scale = 0.0;
  for (size_t i = 0; i < 3 * n; ++i)
  {
    diff = std::fmax(diff, std::fabs(z[i] - zc[i]));
    scale = std::fmax(scale, std::fabs(zc[i]));
  }
  std::printf("S %zu %d %.3e %.3e\n", n, cut, residual, diff / scale);
  check(residual <= 1e-12, "|M z - r| <= 1e-12 |r|", n);
  check(diff <= 1e-10 * scale, "|z - z_chol| <= 1e-10 |z_chol|", n);
}

}  // namespace

int main()
{
  // ---- the levels: every node but the root is eliminated at exactly one stride ----
  const size_t sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025, 2049};
  for (size_t n : sizes)
  {
    std::vector<int> seen(n, 0);
    size_t levels = 0;
    for (size_t s = 1; s < n; s *= 2, ++levels)
    {
      for (size_t q = 0; q < CH::gone_count(n, s); ++q)
      {
        const size_t i = CH::gone_node(s, q);
        check(i < n && i % (2 * s) == s, "gone_node", n);
        if (i < n) ++seen[i];
      }
      const size_t stay = CH::stay_count(n, s);
      check(CH::stay_node(s, stay - 1) < n && CH::stay_node(s, stay) >= n, "stay_count", n);
      check(s <= CH::top_stride(n), "top_stride", n);
    }
    size_t log2 = 0;
    while ((size_t(1) << log2) < n) ++log2;
    check(levels == log2, "ceil(log2 n) levels", n);
    check(seen[0] == 0, "the root is eliminated", n);
    for (size_t i = 1; i < n; ++i) check(seen[i] == 1, "a node is not eliminated exactly once", n);
  }
  check(CH::top_stride(1) == 0 && CH::top_stride(2) == 1 && CH::top_stride(1024) == 512 && CH::top_stride(1025) == 1024, "top_stride values", 0);

  // ---- the systems ----
  for (size_t n : sizes)
  {
    for (int cut = 0; cut < 4; ++cut) run(n, cut);
  }

  // ---- a block that is not positive definite is reported, not inverted ----
  for (size_t bad : {size_t(0), size_t(5), size_t(8)})
  {
    Blocks m = make(9, 0);
    m.D[6 * bad + 3] = -m.D[6 * bad + 3];       // a negative diagonal entry: indefinite
    std::vector<double> r(27, 1.0), z, pivots;
    check(!reduce_solve(m, r, z, &pivots), "an indefinite block was not reported", bad);
    if (bad != 0 && bad != 8)
    {
      // (node 5 is eliminated at the first stride: its own block is the pivot)
      for (int k = 0; k < 6; ++k) check(pivots[6 * bad + k] == 0.0, "an indefinite block was inverted", bad);
    }
  }
  {
    Blocks m = make(4, 0);
    m.D[6 * 1] = std::nan("");
    std::vector<double> r(12, 1.0), z;
    check(!reduce_solve(m, r, z), "a block that is not finite was not reported", 4);
    double S[6] = {1.0, 2.0, 0.0, 1.0, 0.0, 1.0}, out[6];   // positive diagonal and determinant -3: the second minor tells
    check(!CH::invert_spd(S, out) && out[0] == 0.0 && out[5] == 0.0, "invert_spd: indefinite", 0);
    double T[6] = {1.0, 0.0, 0.0, -1.0, 0.0, -1.0};          // determinant +1, not definite
    check(!CH::invert_spd(T, out), "invert_spd: two negative eigenvalues", 0);
  }

  if (failures != 0) return 1;
  std::printf("ok\n");
  return 0;
}
