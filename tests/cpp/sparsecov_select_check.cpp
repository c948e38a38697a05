// csrc/sparsecov/ndt2d_sparsecov_select.h in a program of its own: random SPD systems of the sparse
// solve's structure (tests/cpp/sparse_schur_check.cpp's generator and ranges: a chain with lambda D,
// closures, disabled chain edges, a floating component held by lambda D alone, a fixed node anywhere,
// weights over four decades), each inverted three ways: by the header's sequential driver (the steps
// the kernels run), by a plain dense Cholesky in doubles, and by the same Cholesky in long double,
// which is the yardstick.  Compared are the block errors max |Sigma - Sigma_long| of the first two
// over every diagonal block and a sample of pairs (two nodes of one segment, two of different
// segments, a separator with an interior node, two separators, a = b, and each the other way round):
// the driver's may be kBound times the dense inverse's own, floored at 4 ulps of |Sigma|_max.  kBound
// is 4 x the worst ratio measured over these systems (the program prints it; it was 2165.17 while the
// reduction multiplied by explicitly inverted 3 x 3 pivots, and is 23.13 with the pivots kept factored).  Also: a diagonal block is symmetric bit for bit, (a, b) and (b, a)
// are transposes bit for bit, (a, a) is the diagonal block, a node that is not free has zero blocks,
// a pair's block does not depend on the other pairs, and a system that is not definite is refused.
// Prints "ok" and returns 0, or says what failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sparse/ndt2d_sparse_plan.h"
#include "sparse/ndt2d_sparse_schur.h"
#include "sparsecov/ndt2d_sparsecov_plan.h"
#include "sparsecov/ndt2d_sparsecov_select.h"

namespace sp = ndt2d::sparse;
namespace sc = ndt2d::sparsecov;
namespace cov = ndt2d::covariance;

namespace
{

constexpr double kBound = 4.0 * 23.13;   // 4 x the worst ratio measured over the systems below, 23.13 (printed at the end)
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

// T = L^-1 of A = L L^T (lower, N x N) in the type F; false where a pivot is not positive.
template <class F>
bool inverse_factor(const std::vector<double> & A, size_t N, std::vector<F> * out)
{
  std::vector<F> L(N * N);
  for (size_t k = 0; k < N * N; ++k) L[k] = A[k];
  for (size_t j = 0; j < N; ++j)
  {
    F pivot = L[j * N + j];
    for (size_t k = 0; k < j; ++k) pivot -= L[j * N + k] * L[j * N + k];
    if (!(pivot > 0)) return false;
    const F root = std::sqrt(pivot);
    L[j * N + j] = root;
    for (size_t i = j + 1; i < N; ++i)
    {
      F v = L[i * N + j];
      for (size_t k = 0; k < j; ++k) v -= L[i * N + k] * L[j * N + k];
      L[i * N + j] = v / root;
    }
  }
  std::vector<F> & T = *out;
  T.assign(N * N, 0);
  for (size_t j = 0; j < N; ++j)
  {
    T[j * N + j] = 1 / L[j * N + j];
    for (size_t i = j + 1; i < N; ++i)
    {
      F v = 0;
      for (size_t k = j; k < i; ++k) v += L[i * N + k] * T[k * N + j];
      T[i * N + j] = -v / L[i * N + i];
    }
  }
  return true;
}

// Block (a, b) of T^T T.
template <class F>
void block_of(const std::vector<F> & T, size_t N, size_t a, size_t b, F * out)
{
  const size_t first = 3 * (a > b ? a : b);
  for (int r = 0; r < 3; ++r)
  {
    for (int c = 0; c < 3; ++c)
    {
      F v = 0;
      for (size_t k = first; k < N; ++k) v += T[k * N + 3 * a + r] * T[k * N + 3 * b + c];
      out[3 * r + c] = v;
    }
  }
}

struct Built
{
  size_t n = 0;
  sp::Layout layout;
  std::vector<double> A;
  std::vector<uint8_t> active;
};

// The graph and A densely, as tests/cpp/sparse_schur_check.cpp builds them.
void build(Rng & rng, size_t n, size_t want_sep, double p_off, bool floating, Built * out)
{
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
  out->n = n;
  sp::make_layout(n, edges.size(), begin.data(), end.data(), &out->layout);
  const uint32_t fixed = static_cast<uint32_t>(rng.below(n));
  const size_t N = 3 * n;
  std::vector<double> H(N * N, 0.0);
  std::vector<uint8_t> & active = out->active;
  active.assign(n, 0);
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
  out->A = H;
  for (size_t i = 0; i < n; ++i)
  {
    for (int j = 0; j < 3; ++j)
    {
      const size_t at = 3 * i + j;
      if (!active[i])
      {
        out->A[at * N + at] = 1.0;
        continue;
      }
      out->A[at * N + at] += lambda * std::fmin(std::fmax(H[at * N + at], 1e-6), 1e32);
    }
  }
}

// The driver over the system with the asked pairs.  False: it refused.
bool run_driver(const Built & sys, const std::vector<uint32_t> & asked, std::vector<double> * diagonal, std::vector<double> * pairs, size_t trial)
{
  const sp::Tables t = sys.layout.tables();
  const size_t n = sys.n, N = 3 * n, ni = t.ni, ns = t.s, ld = cov::padded(3 * ns), P = asked.size() / 2;
  const std::vector<double> & A = sys.A;
  sc::Lists lists;
  sc::make_lists(t, asked.data(), P, &lists);
  std::vector<double> interior(sp::interior_doubles(ni) + 1, 0.0), S(ld * ld + 1, 0.0), T(ld * ld + 1, 0.0), diag(ld + 1, 1.0), gs(3 * ns + 1, 0.0),
      sel(sc::select_doubles(ni) + 1, 0.0), table(9 * lists.n_blocks() + 1, 0.0), columns(9 * P + 1, 0.0), zero(N, 0.0);
  diagonal->assign(9 * n + 1, 7.0);
  pairs->assign(9 * P + 1, 7.0);
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
  int stage = -1;
  double ratio = 0.0;
  sc::compute(t, in, S.data(), T.data(), ld, diag.data(), sys.active.data(), lists, sel.data(), table.data(), columns.data(), zero.data(), gs.data(),
              diagonal->data(), pairs->data(), &stage, &ratio);
  if (interior.back() != 0.0 || S.back() != 0.0 || T.back() != 0.0 || diag.back() != 1.0 || gs.back() != 0.0 || sel.back() != 0.0 ||
      table.back() != 0.0 || columns.back() != 0.0 || diagonal->back() != 7.0 || pairs->back() != 7.0)
  {
    fail("a write past an array", trial);
  }
  if (stage == 0 && !(ratio > 0.0 && ratio <= 1.0)) fail("the pivot ratio is not in (0, 1]", trial);
  return stage == 0;
}

// The sample of pairs: by kind where the layout has them, then a few at random, then each reversed.
std::vector<uint32_t> sample_pairs(Rng & rng, const sp::Tables & t)
{
  std::vector<uint32_t> out;
  const auto put = [&](uint32_t a, uint32_t b) {
    out.push_back(a);
    out.push_back(b);
  };
  const uint32_t n = t.n;
  std::vector<uint32_t> interior, separators;
  for (uint32_t i = 0; i < n; ++i) (t.separator(i) ? separators : interior).push_back(i);
  if (!interior.empty())
  {
    const uint32_t a = interior[rng.below(interior.size())];
    put(a, a);
    // two nodes of one segment: the nearest interior nodes with the same separator before them
    for (size_t tries = 0; tries < 8; ++tries)
    {
      const uint32_t x = interior[rng.below(interior.size())], y = interior[rng.below(interior.size())];
      if (x != y && t.before[t.index(x)] == t.before[t.index(y)])
      {
        put(x, y);
        break;
      }
    }
    for (uint32_t i = 0; i + 1 < n; ++i)
    {
      if (!t.separator(i) && !t.separator(i + 1))
      {
        put(i, i + 1);
        break;
      }
    }
    // two nodes of different segments
    for (size_t tries = 0; tries < 8; ++tries)
    {
      const uint32_t x = interior[rng.below(interior.size())], y = interior[rng.below(interior.size())];
      if (t.before[t.index(x)] != t.before[t.index(y)])
      {
        put(x, y);
        break;
      }
    }
  }
  if (!separators.empty())
  {
    const uint32_t v = separators[rng.below(separators.size())];
    put(v, v);
    put(v, separators[rng.below(separators.size())]);
    if (!interior.empty())
    {
      put(v, interior[rng.below(interior.size())]);
      if (v > 0 && !t.separator(v - 1)) put(v - 1, v);
    }
  }
  for (int k = 0; k < 4; ++k) put(static_cast<uint32_t>(rng.below(n)), static_cast<uint32_t>(rng.below(n)));
  const size_t forward = out.size() / 2;
  for (size_t q = 0; q < forward; ++q) put(out[2 * q + 1], out[2 * q]);
  return out;
}

// One system.  Returns the ratio driver error / max(dense error, floor), or -1 where it was not
// invertible as expected.
double one_system(Rng & rng, size_t trial, size_t n, size_t want_sep, double p_off, bool floating, bool * floored)
{
  Built sys;
  build(rng, n, want_sep, p_off, floating, &sys);
  const sp::Tables t = sys.layout.tables();
  const size_t N = 3 * n;
  const std::vector<uint32_t> asked = sample_pairs(rng, t);
  const size_t P = asked.size() / 2, forward = P / 2;
  std::vector<double> diagonal, pairs;
  if (!run_driver(sys, asked, &diagonal, &pairs, trial))
  {
    fail("the driver refused a positive definite system", trial);
    return -1.0;
  }
  std::vector<double> Td;
  std::vector<long double> Tl;
  if (!inverse_factor(sys.A, N, &Td) || !inverse_factor(sys.A, N, &Tl))
  {
    fail("the dense Cholesky met a pivot <= 0: the system is not as designed", trial);
    return -1.0;
  }
  long double err_sparse = 0.0L, err_dense = 0.0L, scale = 0.0L;
  const auto compare = [&](size_t a, size_t b, const double * got) {
    double dense[9];
    long double exact[9];
    block_of(Td, N, a, b, dense);
    block_of(Tl, N, a, b, exact);
    const bool free_pair = sys.active[a] && sys.active[b];
    for (int k = 0; k < 9; ++k)
    {
      if (!free_pair)
      {
        if (got[k] != 0.0) fail("a block of a node that is not free is not zero", trial);
        continue;
      }
      err_sparse = fmaxl(err_sparse, fabsl(static_cast<long double>(got[k]) - exact[k]));
      err_dense = fmaxl(err_dense, fabsl(static_cast<long double>(dense[k]) - exact[k]));
      scale = fmaxl(scale, fabsl(exact[k]));
    }
  };
  for (size_t i = 0; i < n; ++i)
  {
    const double * B = diagonal.data() + 9 * i;
    compare(i, i, B);
    if (B[1] != B[3] || B[2] != B[6] || B[5] != B[7]) fail("a diagonal block is not symmetric bit for bit", trial);
  }
  for (size_t q = 0; q < P; ++q)
  {
    const uint32_t a = asked[2 * q], b = asked[2 * q + 1];
    const double * B = pairs.data() + 9 * q;
    compare(a, b, B);
    if (a == b && std::memcmp(B, diagonal.data() + 9 * a, 9 * sizeof(double)) != 0) fail("(a, a) is not the diagonal block", trial);
    if (q < forward)
    {
      const double * R = pairs.data() + 9 * (forward + q);
      for (int r = 0; r < 3; ++r)
      {
        for (int c = 0; c < 3; ++c)
        {
          if (std::memcmp(&B[3 * r + c], &R[3 * c + r], sizeof(double)) != 0) fail("(a, b) and (b, a) are not transposes bit for bit", trial);
        }
      }
    }
  }
  // a pair's block does not depend on the other pairs, the diagonal not on the pair list
  if (P != 0)
  {
    const size_t q = rng.below(P);
    const std::vector<uint32_t> alone = {asked[2 * q], asked[2 * q + 1]};
    std::vector<double> diagonal_alone, pair_alone;
    if (!run_driver(sys, alone, &diagonal_alone, &pair_alone, trial)) fail("the driver refused the system with one pair", trial);
    if (std::memcmp(pair_alone.data(), pairs.data() + 9 * q, 9 * sizeof(double)) != 0) fail("a pair's block depends on the other pairs", trial);
    if (std::memcmp(diagonal_alone.data(), diagonal.data(), 9 * n * sizeof(double)) != 0) fail("the diagonal depends on the pair list", trial);
  }
  const long double floor = 4.0L * kEps * scale;
  const long double against = fmaxl(err_dense, floor);
  const double ratio = against > 0.0L ? static_cast<double>(err_sparse / against) : (err_sparse == 0.0L ? 0.0 : INFINITY);
  *floored = err_dense < floor;
  if (!(ratio <= kBound))
  {
    std::printf("system %zu: n %zu s %u: driver %.3Le dense %.3Le floor %.3Le ratio %.2f\n", trial, n, t.s, err_sparse, err_dense, floor, ratio);
    fail("the driver's block error is over the bound", trial);
  }
  return ratio;
}

// A system that is not positive definite is refused with its stage and zero blocks: in an interior
// pivot, and in S.
void refusals()
{
  const uint32_t begin[3] = {0, 1, 0}, end[3] = {1, 2, 2};   // nodes 0 and 2 are separators, 1 interior
  sp::Layout layout;
  sp::make_layout(3, 3, begin, end, &layout);
  const sp::Tables t = layout.tables();
  const size_t ld = cov::padded(6);
  const uint32_t asked[2] = {0, 1};
  sc::Lists lists;
  sc::make_lists(t, asked, 1, &lists);
  for (int which = 0; which < 2; ++which)
  {
    std::vector<double> interior(sp::interior_doubles(1), 0.0), S(ld * ld, 0.0), T(ld * ld, 0.0), diag(ld, 1.0), gs(6, 0.0), sel(sc::select_doubles(1), 0.0),
        table(9 * lists.n_blocks(), 0.0), columns(9, 0.0), zero(9, 0.0), diagonal(27, 7.0), pairs(9, 7.0);
    const uint8_t active[3] = {1, 1, 1};
    const sp::Interior in = sp::interior_at(interior.data(), 1);
    for (size_t k = 0; k < ld; ++k) S[k * ld + k] = 1.0;
    in.m.D[0] = in.m.D[3] = in.m.D[5] = 1.0;
    if (which == 0) in.m.D[3] = -1.0;
    else S[ld + 1] = -2.0;
    int stage = -1;
    double ratio = 0.0;
    sc::compute(t, in, S.data(), T.data(), ld, diag.data(), active, lists, sel.data(), table.data(), columns.data(), zero.data(), gs.data(),
                diagonal.data(), pairs.data(), &stage, &ratio);
    if (stage != which + 1) fail("a system that is not definite was not refused with its stage", which);
    for (double v : diagonal)
    {
      if (v != 0.0) fail("a refused system has a block that is not zero", which);
    }
    for (double v : pairs)
    {
      if (v != 0.0) fail("a refused system has a pair that is not zero", which);
    }
  }
}

}  // namespace

int main()
{
  Rng rng{0x9e3779b97f4a7c15ull};
  double worst = 0.0;
  size_t trial = 0, with_floor = 0;
  const size_t sizes[] = {2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 33, 64, 65, 100, 200};
  const size_t seps[] = {0, 1, 2, 3, 5, 8, 16, 17, 32, 40};
  for (size_t n : sizes)
  {
    for (size_t s : seps)
    {
      if (n >= 100 && s != 0 && s != 17 && s != 40) continue;   // (the long-double inverse is O(n^3): fewer of the largest)
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
