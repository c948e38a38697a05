// The linear step of the sparse pose-graph solve (sparse/ndt2d_sparse_kernel.h; include/ndt2d_hip.h,
// "Sparse solve"): A delta = -g for A = [A_ii A_is; A_si A_ss], the interior nodes' block A_ii one
// block-tridiagonal system in node order and A_is at most two 3 x 3 blocks per interior node, by the
// Schur complement on the separators,
//     Z = A_ii^-1 A_is,  y = A_ii^-1 (-g_i),  S = A_ss - A_si Z,  S delta_s = -g_s - A_si y,
//     delta_i = y - Z delta_s.
// A_ii^-1 is the block cyclic reduction of posegraph/ndt2d_posegraph_chain.h over ALL interior nodes
// at once (the segments between separators are decoupled: their couplings are zero), applied to
// seven columns together: -g_i, the three of R_left (the block A(p, p - 1) at an interior node p whose
// predecessor is a separator) and the three of R_right (A(q, q + 1) where the successor is one).
// Plain C++ without HIP types, host and device, as posegraph/ndt2d_posegraph_chain.h: the kernels run
// the per-node steps below, the sequential driver at the end runs the same steps over one system and
// is what a stand-alone host program checks against a dense Cholesky (tests/cpp/sparse_schur_check.cpp).
//
// Per interior node ii, in the job's arrays (sparse/ndt2d_sparse_plan.h):
//   m.D, m.U, m.L, m.P   the reduction's, as chain::System; in: the node's block and its coupling to
//                        the next interior node where that is node + 1, else zero
//   b [7][3]             the columns' right-hand sides, reduced in place; column 0 is -g
//   x [7][3]             their solutions: y, then Z_left and Z_right column by column
//   Cl [9], Cr [9]       row-major A(i, i - 1) and A(i, i + 1) where that neighbour is a separator,
//                        else zero: kept as assembled, A_si is their transposes
// A sum has a fixed order: a 3-vector product ascending from zero, then one subtraction.
#ifndef NDT2D_SPARSE_SCHUR_H_
#define NDT2D_SPARSE_SCHUR_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "posegraph/ndt2d_posegraph_chain.h"
#include "sparse/ndt2d_sparse_plan.h"

namespace ndt2d
{
namespace sparse
{

namespace chain = posegraph::chain;

constexpr size_t kColumnDoubles = 3 * kColumns;

struct Interior
{
  chain::System m;
  double * b, * x, * Cl, * Cr;
};

NDT2D_PG_HD inline Interior interior_at(double * base, size_t ni)
{
  Interior in;
  in.m.D = base;
  in.m.U = in.m.D + 6 * ni;
  in.m.L = in.m.U + 9 * ni;
  in.m.P = in.m.L + 9 * ni;
  in.b = in.m.P + 6 * ni;
  in.x = in.b + kColumnDoubles * ni;
  in.Cl = in.x + kColumnDoubles * ni;
  in.Cr = in.Cl + 9 * ni;
  return in;
}

// The seven right-hand sides of interior node ii from its gradient g3 and its Cl, Cr.
NDT2D_PG_HD inline void set_columns(const Interior & in, size_t ii, const double * g3)
{
  double * b = in.b + kColumnDoubles * ii;
  const double * Cl = in.Cl + 9 * ii, * Cr = in.Cr + 9 * ii;
  for (int r = 0; r < 3; ++r)
  {
    b[r] = -g3[r];
    for (int c = 0; c < 3; ++c)
    {
      b[3 * (1 + c) + r] = Cl[3 * r + c];
      b[3 * (4 + c) + r] = Cr[3 * r + c];
    }
  }
}

// ---- the reduction's right-hand-side and back-substitution steps over K columns: chain's
// forward_node, back_root and back_node, a level's L, P and U read once for the K ----

template <int K>
NDT2D_PG_HD inline void forward_columns(const chain::System & m, double * b, size_t n, size_t j, size_t s)
{
  double * bj = b + kColumnDoubles * j;
  if (j >= s)
  {
    const size_t lo = j - s;
    double P[6], U[9];
    for (int k = 0; k < 6; ++k) P[k] = m.P[6 * lo + k];
    for (int k = 0; k < 9; ++k) U[k] = m.U[9 * lo + k];
    const double * bl = b + kColumnDoubles * lo;
    for (int c = 0; c < K; ++c)
    {
      double t[3], y[3];
      chain::apply_pivot(P, bl + 3 * c, t);
      posegraph::mul_t(U, t, y);
      bj[3 * c] -= y[0];
      bj[3 * c + 1] -= y[1];
      bj[3 * c + 2] -= y[2];
    }
  }
  const size_t hi = j + s;
  if (hi < n)
  {
    double P[6], L[9];
    for (int k = 0; k < 6; ++k) P[k] = m.P[6 * hi + k];
    for (int k = 0; k < 9; ++k) L[k] = m.L[9 * hi + k];
    const double * bh = b + kColumnDoubles * hi;
    for (int c = 0; c < K; ++c)
    {
      double t[3], y[3];
      chain::apply_pivot(P, bh + 3 * c, t);
      posegraph::mul(L, t, y);
      bj[3 * c] -= y[0];
      bj[3 * c + 1] -= y[1];
      bj[3 * c + 2] -= y[2];
    }
  }
}

template <int K>
NDT2D_PG_HD inline void root_columns(const chain::System & m, const double * b, double * x)
{
  for (int c = 0; c < K; ++c) chain::apply_pivot(m.P, b + 3 * c, x + 3 * c);
}

template <int K>
NDT2D_PG_HD inline void back_columns(const chain::System & m, const double * b, double * x, size_t n, size_t i, size_t s)
{
  double P[6], L[9], U[9];
  for (int k = 0; k < 6; ++k) P[k] = m.P[6 * i + k];
  for (int k = 0; k < 9; ++k) L[k] = m.L[9 * i + k];
  const bool above = i + s < n;
  for (int k = 0; k < 9; ++k) U[k] = above ? m.U[9 * i + k] : 0.0;
  const double * bi = b + kColumnDoubles * i, * xl = x + kColumnDoubles * (i - s);
  const double * xh = x + kColumnDoubles * (above ? i + s : i);
  double * xi = x + kColumnDoubles * i;
  for (int c = 0; c < K; ++c)
  {
    double t[3] = {bi[3 * c], bi[3 * c + 1], bi[3 * c + 2]}, y[3];
    posegraph::mul_t(L, xl + 3 * c, y);
    t[0] -= y[0];
    t[1] -= y[1];
    t[2] -= y[2];
    if (above)
    {
      posegraph::mul(U, xh + 3 * c, y);
      t[0] -= y[0];
      t[1] -= y[1];
      t[2] -= y[2];
    }
    chain::apply_pivot(P, t, y);
    xi[3 * c] = y[0];
    xi[3 * c + 1] = y[1];
    xi[3 * c + 2] = y[2];
  }
}

// ---- the separators ----

// Separator si, the owner of block row si of S (row-major, leading dimension ld; the lower triangle
// and the whole diagonal block are kept): subtracts A_si Z from its diagonal block and from the block
// to the separator before it, notes the diagonal, and forms gs = g_s + A_si y = -b_s.  With the
// interior nodes q = node - 1 and p = node + 1 (where they are interior) and u the separator before q:
//   S(si, si) -= A(v, q) Z_right[q] + A(v, p) Z_left[p],   S(si, u) -= A(v, q) Z_left[q],
//   A(v, q) = Cr[q]^T, A(v, p) = Cl[p]^T.
NDT2D_PG_HD inline void schur_separator(const Tables & t, const Interior & in, const double * g, uint32_t si, double * S, size_t ld, double * diag,
                                        double * gs)
{
  const size_t v = t.node[si], at = 3 * static_cast<size_t>(si);
  const uint32_t q = t.previous[si], p = t.next[si];
  double own[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double bv[3] = {g[3 * v], g[3 * v + 1], g[3 * v + 2]}, col[3];
  if (q != kNone)
  {
    const double * C = in.Cr + 9 * static_cast<size_t>(q), * x = in.x + kColumnDoubles * q;
    for (int c = 0; c < 3; ++c)
    {
      posegraph::mul_t(C, x + 3 * (4 + c), col);
      for (int a = 0; a < 3; ++a) own[3 * a + c] += col[a];
    }
    posegraph::mul_t(C, x, col);
    for (int a = 0; a < 3; ++a) bv[a] += col[a];
    const uint32_t u = t.before[q];
    if (u != kNone)
    {
      double * block = S + at * ld + 3 * static_cast<size_t>(u);
      for (int c = 0; c < 3; ++c)
      {
        posegraph::mul_t(C, x + 3 * (1 + c), col);
        for (int a = 0; a < 3; ++a) block[a * ld + c] -= col[a];
      }
    }
  }
  if (p != kNone)
  {
    const double * C = in.Cl + 9 * static_cast<size_t>(p), * x = in.x + kColumnDoubles * p;
    for (int c = 0; c < 3; ++c)
    {
      posegraph::mul_t(C, x + 3 * (1 + c), col);
      for (int a = 0; a < 3; ++a) own[3 * a + c] += col[a];
    }
    posegraph::mul_t(C, x, col);
    for (int a = 0; a < 3; ++a) bv[a] += col[a];
  }
  double * block = S + at * ld + at;
  for (int a = 0; a < 3; ++a)
  {
    for (int c = 0; c < 3; ++c) block[a * ld + c] -= own[3 * a + c];
    diag[at + a] = block[a * ld + a];
    gs[at + a] = bv[a];
  }
}

// The step of node i into d [n][3]: a separator's from ds, an interior node's
// y - Z_left delta(before) - Z_right delta(after).
NDT2D_PG_HD inline void expand_node(const Tables & t, const Interior & in, const double * ds, uint32_t i, double * d)
{
  const size_t at = 3 * static_cast<size_t>(i), k = t.index(i);
  if (t.separator(i))
  {
    for (int j = 0; j < 3; ++j) d[at + j] = ds[3 * k + j];
    return;
  }
  const double * x = in.x + kColumnDoubles * k;
  double r[3] = {x[0], x[1], x[2]};
  const uint32_t sides[2] = {t.before[k], t.after[k]};
  for (int side = 0; side < 2; ++side)
  {
    if (sides[side] == kNone) continue;
    const double * e = ds + 3 * static_cast<size_t>(sides[side]), * Z = x + 3 * (1 + 3 * side);
    for (int j = 0; j < 3; ++j)
    {
      double sum = 0.0;
      for (int c = 0; c < 3; ++c) sum += Z[3 * c + j] * e[c];
      r[j] -= sum;
    }
  }
  for (int j = 0; j < 3; ++j) d[at + j] = r[j];
}

// ---- the sequential driver (host) ----

// The whole linear step over one system.  In: in.m.D, in.m.U, in.Cl, in.Cr as assembled; S the
// separators' block A_ss (its lower triangle and diagonal blocks, the identity from 3 s on); g [n][3].
// Out: d [n][3]; gs and ds [3 s], diag [ld] are its scratch; *ratio the smallest pivot / diagonal of
// S's factorisation (1 without a separator).  False: a pivot of the reduction or of S was not
// positive -- d is then not to be used.
inline bool solve(const Tables & t, const Interior & in, double * S, size_t ld, double * diag, const double * g, double * gs, double * ds, double * d,
                  double * ratio)
{
  const size_t ni = t.ni, dim = 3 * static_cast<size_t>(t.s);
  for (uint32_t i = 0; i < t.n; ++i)
  {
    if (!t.separator(i)) set_columns(in, t.index(i), g + 3 * static_cast<size_t>(i));
  }
  bool ok = chain::factor(in.m, ni);
  if (ni != 0)
  {
    for (size_t s = 1; s < ni; s *= 2)
    {
      const size_t count = chain::stay_count(ni, s);
      for (size_t q = 0; q < count; ++q) forward_columns<kColumns>(in.m, in.b, ni, chain::stay_node(s, q), s);
    }
    root_columns<kColumns>(in.m, in.b, in.x);
    for (size_t s = chain::top_stride(ni); s >= 1; s /= 2)
    {
      const size_t count = chain::gone_count(ni, s);
      for (size_t q = 0; q < count; ++q) back_columns<kColumns>(in.m, in.b, in.x, ni, chain::gone_node(s, q), s);
    }
  }
  for (uint32_t si = 0; si < t.s; ++si) schur_separator(t, in, g, si, S, ld, diag, gs);
  *ratio = 1.0;
  for (size_t j = 0; j < dim; ++j)   // S = L L^T in its lower triangle
  {
    double pivot = S[j * ld + j];
    for (size_t k = 0; k < j; ++k) pivot -= S[j * ld + k] * S[j * ld + k];
    if (!(pivot > 0.0) || !(pivot <= 1.7976931348623157e308)) return false;
    if (pivot / diag[j] < *ratio) *ratio = pivot / diag[j];
    const double root = sqrt(pivot);
    S[j * ld + j] = root;
    for (size_t i = j + 1; i < dim; ++i)
    {
      double v = S[i * ld + j];
      for (size_t k = 0; k < j; ++k) v -= S[i * ld + k] * S[j * ld + k];
      S[i * ld + j] = v / root;
    }
  }
  if (!ok) return false;
  for (size_t i = 0; i < dim; ++i)
  {
    double v = -gs[i];
    for (size_t k = 0; k < i; ++k) v -= S[i * ld + k] * ds[k];
    ds[i] = v / S[i * ld + i];
  }
  for (size_t k = dim; k > 0; --k)
  {
    const size_t i = k - 1;
    double v = ds[i];
    for (size_t r = i + 1; r < dim; ++r) v -= S[r * ld + i] * ds[r];
    ds[i] = v / S[i * ld + i];
  }
  for (uint32_t i = 0; i < t.n; ++i) expand_node(t, in, ds, i, d);
  return true;
}

}  // namespace sparse
}  // namespace ndt2d

#endif  // NDT2D_SPARSE_SCHUR_H_
