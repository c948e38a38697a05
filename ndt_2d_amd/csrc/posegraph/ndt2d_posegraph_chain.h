// The chain preconditioner of the pose graph (posegraph/ndt2d_posegraph_kernel.h, "chain"): a symmetric
// positive definite block-tridiagonal system of n nodes with 3 x 3 blocks, factored and solved
// exactly by block cyclic reduction without pivoting, for any n.  Plain C++ without HIP types, host
// and device, as posegraph/ndt2d_posegraph_fn.h: the kernel runs the per-node steps below with one
// barrier between levels, the sequential drivers at the end run the same steps over a whole system
// and are what a stand-alone host program checks (tests/cpp/posegraph_chain_check.cpp).
//
// The reduction.  At stride s = 1, 2, 4, ... < n the live nodes are the multiples of s.  Those whose
// index is an odd multiple of s are eliminated into their neighbours at -s and +s, the even
// multiples stay.  The step of a level is written for the node that STAYS (j, a multiple of 2 s):
// it alone reads and writes its own diagonal D[j] and coupling U[j], and it only reads what its
// eliminated neighbours lo = j - s and hi = j + s hold, which no step of the level writes -- but
// for P[hi] and L[hi], which j alone writes.  The steps of one level are therefore independent.
// Node 0 is never eliminated: the root.
//
// Per node, in the caller's arrays:
//   D [6]  the working diagonal block, symmetric as (00, 01, 02, 11, 12, 22); in: the block of M
//   U [9]  row-major, the block (i, i + s) at the node's current stride; in: the block (i, i + 1).
//          After the node's elimination at stride s it stays as it was: its coupling to i + s
//   L [9]  kept at the node's elimination: the block (i - s, i)
//   P [6]  kept at the node's elimination (the root's: at the end): its pivot D[i] factored, M = L^-1 of
//          D[i] = L L^T (factor_spd); D[i]^-1 v is apply_pivot's M^T (M v), D[i]^-1 itself pivot_inverse's M^T M
// and for a solve b [3], the right-hand side reduced in place, and x [3].
#ifndef NDT2D_POSEGRAPH_CHAIN_H_
#define NDT2D_POSEGRAPH_CHAIN_H_

#include <stddef.h>

#include "ndt2d_posegraph_fn.h"

namespace ndt2d
{
namespace posegraph
{
namespace chain
{

struct System
{
  double * D, * U, * L, * P;
};

// ---- levels and indices ----

// The nodes that stay at stride s are j = 2 s q, q = 0 .. stay_count - 1.
NDT2D_PG_HD inline size_t stay_count(size_t n, size_t s) { return (n + 2 * s - 1) / (2 * s); }
NDT2D_PG_HD inline size_t stay_node(size_t s, size_t q) { return 2 * s * q; }

// The nodes eliminated at stride s are i = s + 2 s q, q = 0 .. gone_count - 1.
NDT2D_PG_HD inline size_t gone_count(size_t n, size_t s) { return n > s ? (n - s + 2 * s - 1) / (2 * s) : 0; }
NDT2D_PG_HD inline size_t gone_node(size_t s, size_t q) { return s + 2 * s * q; }

// The last stride of the reduction (the largest power of two below n), 0 for n <= 1: no level.
NDT2D_PG_HD inline size_t top_stride(size_t n)
{
  if (n <= 1) return 0;
  size_t s = 1;
  while (2 * s < n) s *= 2;
  return s;
}

// ---- 3 x 3 blocks ----

// C = A B, A^T B, A B^T of row-major 3 x 3.
NDT2D_PG_HD inline void mm(const double * A, const double * B, double * C)
{
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  }
}

NDT2D_PG_HD inline void mtm(const double * A, const double * B, double * C)
{
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
  }
}

NDT2D_PG_HD inline void mmt(const double * A, const double * B, double * C)
{
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
  }
}

// S -= the upper triangle of the (symmetric up to rounding) row-major X.
NDT2D_PG_HD inline void sub_sym(const double * X, double * S)
{
  S[0] -= X[0]; S[1] -= X[1]; S[2] -= X[2];
  S[3] -= X[4]; S[4] -= X[5]; S[5] -= X[8];
}

// A node's pivot is kept factored (factor_spd, apply_pivot and pivot_inverse of ndt2d_posegraph_fn.h): a product with
// the explicit inverse D^-1 leaves a residual kappa(D) times a solve's, which the reduction carried from level to
// level.
using posegraph::apply_pivot;
using posegraph::factor_spd;
using posegraph::pivot_inverse;

// The inverse itself, D^-1 = M^T M; false (out zeroed) where factor_spd refuses.  No kernel calls it: kept for the
// host checks (tests/cpp/posegraph_chain_check.cpp, posegraph_fn_check.cpp), which hold its refusals.
NDT2D_PG_HD inline bool invert_spd(const double * S, double * out)
{
  double M[6];
  const bool ok = factor_spd(S, M);
  pivot_inverse(M, out);
  return ok;
}

// ---- the per-node steps ----

// Factoring, stride s, the staying node j (a multiple of 2 s): eliminates lo = j - s and hi = j + s
// out of j's row.  False when a pivot met is not positive definite (its inverse is then zero and
// the factors are not to be used).
NDT2D_PG_HD inline bool factor_node(const System & m, size_t n, size_t j, size_t s)
{
  bool ok = true;
  double Dj[6], inv[6], T[9], X[9];
  for (int k = 0; k < 6; ++k) Dj[k] = m.D[6 * j + k];
  if (j >= s)
  {
    const size_t lo = j - s;
    ok = factor_spd(m.D + 6 * lo, inv) && ok;   // (lo's own P is written by the node at lo - s)
    const double * C = m.U + 9 * lo;            // the block (lo, j)
    for (int b = 0; b < 3; ++b)                 // T = P C, column by column
    {
      const double c[3] = {C[b], C[3 + b], C[6 + b]};
      double t[3];
      apply_pivot(inv, c, t);
      T[b] = t[0];
      T[3 + b] = t[1];
      T[6 + b] = t[2];
    }
    mtm(C, T, X);                               // C^T P C
    sub_sym(X, Dj);
  }
  const size_t hi = j + s;
  if (hi < n)
  {
    ok = factor_spd(m.D + 6 * hi, inv) && ok;
    for (int k = 0; k < 6; ++k) m.P[6 * hi + k] = inv[k];
    double C[9];                                // the block (j, hi)
    for (int k = 0; k < 9; ++k)
    {
      C[k] = m.U[9 * j + k];
      m.L[9 * hi + k] = C[k];
    }
    for (int a = 0; a < 3; ++a) apply_pivot(inv, C + 3 * a, T + 3 * a);   // T = C P, row by row (P is symmetric)
    mmt(T, C, X);                               // C P C^T
    sub_sym(X, Dj);
    if (hi + s < n)
    {
      mm(T, m.U + 9 * hi, X);                   // the block (j, j + 2 s) = -C P U[hi]
      for (int k = 0; k < 9; ++k) m.U[9 * j + k] = -X[k];
    }
    else
    {
      for (int k = 0; k < 9; ++k) m.U[9 * j + k] = 0.0;
    }
  }
  for (int k = 0; k < 6; ++k) m.D[6 * j + k] = Dj[k];
  return ok;
}

// Behind the last level: the root's pivot.
NDT2D_PG_HD inline bool factor_root(const System & m) { return factor_spd(m.D, m.P); }

// The right-hand side, stride s, the staying node j: b_j -= (j, lo) P_lo b_lo + (j, hi) P_hi b_hi.
NDT2D_PG_HD inline void forward_node(const System & m, double * b, size_t n, size_t j, size_t s)
{
  double bj[3] = {b[3 * j], b[3 * j + 1], b[3 * j + 2]}, t[3], y[3];
  if (j >= s)
  {
    const size_t lo = j - s;
    apply_pivot(m.P + 6 * lo, b + 3 * lo, t);
    mul_t(m.U + 9 * lo, t, y);
    bj[0] -= y[0];
    bj[1] -= y[1];
    bj[2] -= y[2];
  }
  const size_t hi = j + s;
  if (hi < n)
  {
    apply_pivot(m.P + 6 * hi, b + 3 * hi, t);
    mul(m.L + 9 * hi, t, y);
    bj[0] -= y[0];
    bj[1] -= y[1];
    bj[2] -= y[2];
  }
  b[3 * j] = bj[0];
  b[3 * j + 1] = bj[1];
  b[3 * j + 2] = bj[2];
}

NDT2D_PG_HD inline void back_root(const System & m, const double * b, double * x) { apply_pivot(m.P, b, x); }

// Back-substitution, stride s, the eliminated node i: x_i = P_i (b_i - (i, i - s) x_{i-s} - (i, i + s) x_{i+s}).
NDT2D_PG_HD inline void back_node(const System & m, const double * b, double * x, size_t n, size_t i, size_t s)
{
  double t[3] = {b[3 * i], b[3 * i + 1], b[3 * i + 2]}, y[3];
  mul_t(m.L + 9 * i, x + 3 * (i - s), y);
  t[0] -= y[0];
  t[1] -= y[1];
  t[2] -= y[2];
  if (i + s < n)
  {
    mul(m.U + 9 * i, x + 3 * (i + s), y);
    t[0] -= y[0];
    t[1] -= y[1];
    t[2] -= y[2];
  }
  apply_pivot(m.P + 6 * i, t, y);
  x[3 * i] = y[0];
  x[3 * i + 1] = y[1];
  x[3 * i + 2] = y[2];
}

// ---- the sequential drivers (host) ----

// Factors the system in place (D, U in; D, U, L, P out).  False: a pivot was not positive definite.
inline bool factor(const System & m, size_t n)
{
  if (n == 0) return true;
  bool ok = true;
  for (size_t s = 1; s < n; s *= 2)
  {
    const size_t count = stay_count(n, s);
    for (size_t q = 0; q < count; ++q) ok = factor_node(m, n, stay_node(s, q), s) && ok;
  }
  return factor_root(m) && ok;
}

// x = M^-1 b by the factors; b is reduced in place.
inline void solve(const System & m, size_t n, double * b, double * x)
{
  if (n == 0) return;
  for (size_t s = 1; s < n; s *= 2)
  {
    const size_t count = stay_count(n, s);
    for (size_t q = 0; q < count; ++q) forward_node(m, b, n, stay_node(s, q), s);
  }
  back_root(m, b, x);
  for (size_t s = top_stride(n); s >= 1; s /= 2)
  {
    const size_t count = gone_count(n, s);
    for (size_t q = 0; q < count; ++q) back_node(m, b, x, n, gone_node(s, q), s);
  }
}

}  // namespace chain
}  // namespace posegraph
}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_CHAIN_H_
