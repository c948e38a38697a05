// csrc/sparse/ndt2d_sparse_schur.h in a program of its own: random SPD systems of the sparse solve's
// structure -- a chain with lambda D, closures, disabled chain edges, a floating component held by
// lambda D alone, a fixed node inside a segment or on a separator -- each solved two ways: by the
// header's sequential driver (the steps the kernels run) and by a plain dense Cholesky written here,
// which is the yardstick.  Compared are the residuals |A delta + g|_inf of the two, evaluated in long
// double on the dense matrix: the sparse one may be kBound times the dense one, floored at 4 ulps of
// |A|_inf |delta|_inf.  kBound is 4 x the worst ratio measured over these systems (the program
// prints it): the margin is for chain's explicitly inverted 3 x 3 pivots.
// Prints "ok" and returns 0, or says what failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sparse/ndt2d_sparse_plan.h"
#include "sparse/ndt2d_sparse_schur.h"

namespace sp = ndt2d::sparse;
namespace cov = ndt2d::covariance;

namespace
{

constexpr double kBound = 4.0 * 4.70;   // 4 x the worst ratio measured over the systems below, 4.70 (printed at the end)
constexpr double kEps = 2.220446049250313e-16;

struct Rng
{
  uint64_t s;
  uint64_t next()
  {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  }
  double unit() { return static_cast<double>(next() >> 11) / 9007199254740992.0; }   // [0, 1)
  double sym() { return 2.0 * unit() - 1.0; }
  size_t below(size_t n) { return static_cast<size_t>(next() % n); }
};

struct Edge
{
  uint32_t a, b;
  bool on;
};

int failures = 0;

void fail(const char * what, size_t trial)
{
  std::printf("FAILED: %s (system %zu)\n", what, trial);
  ++failures;
}

// One system.  Returns the ratio sparse residual / max(dense residual, floor), or -1 where it was
// not solvable as expected.
double one_system(Rng & rng, size_t trial, size_t n, size_t want_sep, double p_off, bool floating, bool * floored)
{
  // the graph: the chain, closures among want_sep chosen nodes
  std::vector<Edge> edges;
  for (uint32_t i = 0; i + 1 < n; ++i) edges.push_back(Edge{i, i + 1, rng.unit() >= p_off});
  if (floating && n >= 6) edges[n / 2].on = false;   // what lies behind n / 2 hangs on lambda D and the closures that stay
  std::vector<uint32_t> chosen;
  for (size_t k = 0; k < want_sep && n >= 3; ++k) chosen.push_back(static_cast<uint32_t>(rng.below(n)));
  for (size_t k = 0; k + 1 < chosen.size(); k += 1)
  {
    const uint32_t a = chosen[k], b = chosen[rng.below(chosen.size())];
    if (a == b || a + 1 == b || b + 1 == a) continue;
    edges.push_back(Edge{a, b, !floating && rng.unit() >= 0.2});
    if (rng.unit() < 0.1) edges.push_back(Edge{b, a, true});   // a duplicate, reversed
  }
  std::vector<uint32_t> begin, end;
  for (const Edge & e : edges)
  {
    begin.push_back(e.a);
    end.push_back(e.b);
  }
  sp::Layout layout;
  sp::make_layout(n, edges.size(), begin.data(), end.data(), &layout);
  const sp::Tables t = layout.tables();
  const uint32_t fixed = static_cast<uint32_t>(rng.below(n));
  // H, g densely; a node that is fixed or without an enabled edge is not active
  const size_t N = 3 * n;
  std::vector<double> H(N * N, 0.0), g(N, 0.0);
  std::vector<uint8_t> active(n, 0);
  for (const Edge & e : edges)
  {
    if (e.on) active[e.a] = active[e.b] = 1;
  }
  active[fixed] = 0;
  for (const Edge & e : edges)
  {
    if (!e.on) continue;
    const double weight = std::pow(10.0, 2.0 * rng.sym());
    double Ja[9], Jb[9];
    for (int k = 0; k < 9; ++k)
    {
      Ja[k] = weight * rng.sym();
      Jb[k] = weight * rng.sym();
    }
    const size_t nodes[2] = {e.a, e.b};
    const double * J[2] = {Ja, Jb};
    for (int x = 0; x < 2; ++x)
    {
      for (int y = 0; y < 2; ++y)
      {
        if (!active[nodes[x]] || !active[nodes[y]]) continue;
        for (int r = 0; r < 3; ++r)
        {
          for (int c = 0; c < 3; ++c)
          {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += J[x][3 * k + r] * J[y][3 * k + c];
            H[(3 * nodes[x] + r) * N + 3 * nodes[y] + c] += v;
          }
        }
      }
    }
  }
  const double lambda = std::pow(10.0, -6.0 + 6.0 * rng.unit());
  std::vector<double> A(H);
  for (size_t i = 0; i < n; ++i)
  {
    for (int j = 0; j < 3; ++j)
    {
      const size_t at = 3 * i + j;
      if (!active[i])
      {
        A[at * N + at] = 1.0;
        continue;
      }
      const double dj = std::fmin(std::fmax(H[at * N + at], 1e-6), 1e32);
      A[at * N + at] += lambda * dj;
      g[at] = 10.0 * rng.sym();
    }
  }
  // the sparse structures from A
  const size_t ni = t.ni, ns = t.s, ld = cov::padded(3 * ns);
  std::vector<double> interior(sp::interior_doubles(ni) + 1, 0.0), S(ld * ld + 1, 0.0), diag(ld + 1, 1.0), gs(3 * ns + 1, 0.0), ds(3 * ns + 1, 0.0),
      d(N, 0.0);
  const sp::Interior in = sp::interior_at(interior.data(), ni);
  for (size_t k = 3 * ns; k < ld; ++k) S[k * ld + k] = 1.0;
  const auto block = [&](size_t i, size_t j, double * out) {
    for (int r = 0; r < 3; ++r)
    {
      for (int c = 0; c < 3; ++c) out[3 * r + c] = A[(3 * i + r) * N + 3 * j + c];
    }
  };
  for (uint32_t i = 0; i < n; ++i)
  {
    double B[9];
    if (t.separator(i))
    {
      const size_t row = 3 * static_cast<size_t>(t.index(i));
      for (uint32_t j = 0; j <= i; ++j)
      {
        if (!t.separator(j)) continue;
        block(i, j, B);
        for (int r = 0; r < 3; ++r)
        {
          for (int c = 0; c < 3; ++c) S[(row + r) * ld + 3 * t.index(j) + c] = B[3 * r + c];
        }
      }
      continue;
    }
    const size_t ii = t.index(i);
    block(i, i, B);
    const double sym[6] = {B[0], B[1], B[2], B[4], B[5], B[8]};
    for (int k = 0; k < 6; ++k) in.m.D[6 * ii + k] = sym[k];
    if (i + 1 < n)
    {
      block(i, i + 1, B);
      for (int k = 0; k < 9; ++k) (t.separator(i + 1) ? in.Cr : in.m.U)[9 * ii + k] = B[k];
    }
    if (i > 0 && t.separator(i - 1))
    {
      block(i, i - 1, B);
      for (int k = 0; k < 9; ++k) in.Cl[9 * ii + k] = B[k];
    }
  }
  double ratio_pivot = 0.0;
  const bool solved = sp::solve(t, in, S.data(), ld, diag.data(), g.data(), gs.data(), ds.data(), d.data(), &ratio_pivot);
  if (!solved)
  {
    fail("the driver refused a positive definite system", trial);
    return -1.0;
  }
  if (!(ratio_pivot > 0.0 && ratio_pivot <= 1.0)) fail("the pivot ratio is not in (0, 1]", trial);
  if (interior.back() != 0.0 || S.back() != 0.0 || diag.back() != 1.0 || gs.back() != 0.0 || ds.back() != 0.0) fail("a write past an array", trial);
  // the yardstick: a plain dense Cholesky
  std::vector<double> L(A), dd(N, 0.0);
  for (size_t j = 0; j < N; ++j)
  {
    double pivot = L[j * N + j];
    for (size_t k = 0; k < j; ++k) pivot -= L[j * N + k] * L[j * N + k];
    if (!(pivot > 0.0))
    {
      fail("the dense Cholesky met a pivot <= 0: the system is not as designed", trial);
      return -1.0;
    }
    const double root = std::sqrt(pivot);
    L[j * N + j] = root;
    for (size_t i = j + 1; i < N; ++i)
    {
      double v = L[i * N + j];
      for (size_t k = 0; k < j; ++k) v -= L[i * N + k] * L[j * N + k];
      L[i * N + j] = v / root;
    }
  }
  for (size_t i = 0; i < N; ++i)
  {
    double v = -g[i];
    for (size_t k = 0; k < i; ++k) v -= L[i * N + k] * dd[k];
    dd[i] = v / L[i * N + i];
  }
  for (size_t k = N; k > 0; --k)
  {
    const size_t i = k - 1;
    double v = dd[i];
    for (size_t r = i + 1; r < N; ++r) v -= L[r * N + i] * dd[r];
    dd[i] = v / L[i * N + i];
  }
  // the residuals, in long double
  long double res_sparse = 0.0L, res_dense = 0.0L, norm_a = 0.0L, norm_d = 0.0L;
  for (size_t i = 0; i < N; ++i)
  {
    long double rs = g[i], rd = g[i], row = 0.0L;
    for (size_t j = 0; j < N; ++j)
    {
      const long double a = A[i * N + j];
      rs += a * static_cast<long double>(d[j]);
      rd += a * static_cast<long double>(dd[j]);
      row += fabsl(a);
    }
    res_sparse = fmaxl(res_sparse, fabsl(rs));
    res_dense = fmaxl(res_dense, fabsl(rd));
    norm_a = fmaxl(norm_a, row);
    norm_d = fmaxl(norm_d, fabsl(static_cast<long double>(d[i])));
  }
  for (size_t i = 0; i < n; ++i)   // a node that is not active does not move
  {
    if (!active[i] && (d[3 * i] != 0.0 || d[3 * i + 1] != 0.0 || d[3 * i + 2] != 0.0)) fail("a node that is not active moved", trial);
  }
  const long double floor = 4.0L * kEps * norm_a * norm_d;
  const long double against = fmaxl(res_dense, floor);
  // (a system without a free node: both residuals and the floor are zero)
  const double ratio = against > 0.0L ? static_cast<double>(res_sparse / against) : (res_sparse == 0.0L ? 0.0 : INFINITY);
  *floored = res_dense < floor;
  if (!(ratio <= kBound))
  {
    std::printf("system %zu: n %zu s %zu lambda %.3e: sparse %.3Le dense %.3Le floor %.3Le ratio %.2f\n", trial, n, ns, lambda, res_sparse,
                res_dense, floor, ratio);
    fail("the sparse residual is over the bound", trial);
  }
  return ratio;
}

// A system that is not positive definite is refused: in an interior pivot, and in S.
void refusals()
{
  const uint32_t begin[3] = {0, 1, 0}, end[3] = {1, 2, 2};   // nodes 0 and 2 are separators, 1 interior
  sp::Layout layout;
  sp::make_layout(3, 3, begin, end, &layout);
  const sp::Tables t = layout.tables();
  const size_t ld = cov::padded(6);
  for (int which = 0; which < 2; ++which)
  {
    std::vector<double> interior(sp::interior_doubles(1), 0.0), S(ld * ld, 0.0), diag(ld, 1.0), gs(6, 0.0), ds(6, 0.0), d(9, 0.0), g(9, 1.0);
    const sp::Interior in = sp::interior_at(interior.data(), 1);
    for (size_t k = 0; k < ld; ++k) S[k * ld + k] = 1.0;
    in.m.D[0] = in.m.D[3] = in.m.D[5] = 1.0;
    if (which == 0) in.m.D[3] = -1.0;
    else S[ld + 1] = -2.0;
    double ratio = 0.0;
    if (sp::solve(t, in, S.data(), ld, diag.data(), g.data(), gs.data(), ds.data(), d.data(), &ratio)) fail("a system that is not definite was solved", which);
  }
}

}  // namespace

int main()
{
  Rng rng{0x9e3779b97f4a7c15ull};
  double worst = 0.0;
  size_t trial = 0, with_floor = 0;
  const size_t sizes[] = {2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33, 64, 65, 100, 127, 128, 129, 200};
  const size_t seps[] = {0, 1, 2, 3, 5, 8, 16, 17, 32, 40};
  for (size_t n : sizes)
  {
    for (size_t s : seps)
    {
      for (int variant = 0; variant < 4; ++variant)
      {
        const double p_off = variant == 1 ? 0.15 : (variant == 2 ? 0.5 : 0.0);
        bool floored = false;
        const double ratio = one_system(rng, trial, n, s, p_off, variant == 3, &floored);
        if (ratio > worst) worst = ratio;
        if (floored) ++with_floor;
        ++trial;
      }
    }
  }
  refusals();
  std::printf("worst ratio %.2f over %zu systems (%zu against the floor), the bound %.1f\n", worst, trial, with_floor, kBound);
  if (failures != 0) return 1;
  std::printf("ok\n");
  return 0;
}
