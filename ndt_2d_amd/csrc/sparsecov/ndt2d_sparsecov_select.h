// The arithmetic of the sparse covariance (sparsecov/ndt2d_sparsecov_kernel.h; include/ndt2d_hip.h,
// "Sparse covariance"): blocks of Sigma = A^-1 for the sparse solve's A = [A_ii A_is; A_si A_ss] from
// the factorisation that solve already makes -- the block cyclic reduction of A_ii
// (posegraph/ndt2d_posegraph_chain.h), Z = A_ii^-1 A_is and the separators' S = A_ss - A_si Z
// (sparse/ndt2d_sparse_schur.h) -- without a dense 3n x 3n matrix:
//     Sigma_ss = S^-1,  Sigma_is = -Z Sigma_ss,  Sigma_ii = G + Z Sigma_ss Z^T,  G = A_ii^-1.
// Plain C++ without HIP types, host and device: the kernels run the per-node and per-pair steps
// below, the sequential driver at the end runs the same steps over one system and is what a
// stand-alone host program checks against a dense inverse (tests/cpp/sparsecov_select_check.cpp).
//
// The selected inversion.  The reduction eliminated node i at stride s into lo = i - s and
// hi = i + s (where hi < n) and kept L[i] = the block (lo, i), U[i] = the block (i, hi) and P[i], the
// inverse of its pivot.  G restricted to the nodes alive at stride 2 s is the inverse of the system
// reduced to them, so from the root G_00 = P[0], level by level from the top stride down to 1:
//     G_i,lo = -P[i] (L[i]^T G_lo,lo + U[i] G_hi,lo)
//     G_i,hi = -P[i] (L[i]^T G_lo,hi + U[i] G_hi,hi)
//     G_i,i  =  P[i] - (G_i,lo L[i] + G_i,hi U[i]^T) P[i]
// without the hi terms where hi >= n.  lo and hi are neighbours at stride 2 s, one of them eliminated
// there with the other as its neighbour: with q = lo / (2 s), G_lo,hi is lo's G_.,hi for q odd and
// the transpose of hi's G_.,lo for q even.  Per interior node, kSelectDoubles: G_ii as
// (00, 01, 02, 11, 12, 22), then G_i,lo and G_i,hi row-major.  The nodes of a level are independent:
// each reads what the levels above wrote and writes its own 24 doubles.
//
// A sum has a fixed order: a 3-term product ascending, the separators' terms (before, before),
// (before, after), (after, before), (after, after), then G.
#ifndef NDT2D_SPARSECOV_SELECT_H_
#define NDT2D_SPARSECOV_SELECT_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "posegraph/ndt2d_posegraph_chain.h"
#include "sparse/ndt2d_sparse_plan.h"
#include "sparse/ndt2d_sparse_schur.h"
#include "sparsecov/ndt2d_sparsecov_plan.h"

namespace ndt2d
{
namespace sparsecov
{

namespace chain = posegraph::chain;

// ---- 3 x 3 blocks ----

// The row-major square of a symmetric (00, 01, 02, 11, 12, 22).
NDT2D_PG_HD inline void full(const double * S, double * M)
{
  M[0] = S[0]; M[1] = S[1]; M[2] = S[2];
  M[3] = S[1]; M[4] = S[3]; M[5] = S[4];
  M[6] = S[2]; M[7] = S[4]; M[8] = S[5];
}

NDT2D_PG_HD inline void transposed(const double * A, double * M)
{
  for (int r = 0; r < 3; ++r)
  {
    for (int c = 0; c < 3; ++c) M[3 * r + c] = A[3 * c + r];
  }
}

// ---- the selected inversion ----

NDT2D_PG_HD inline void select_root(const chain::System & m, double * sel)
{
  chain::pivot_inverse(m.P, sel);
  for (int k = 6; k < 24; ++k) sel[k] = 0.0;
}

// Between the phases of select_node on the device: the loads of a phase are not moved in front of
// it, so that the blocks of one phase do not wait in registers through the one before (the kernel
// then stays within its 128 registers).  Nothing on the host.
#if defined(__AMDGCN__)
#define NDT2D_SPARSECOV_PHASE() asm volatile("" ::: "memory")
#else
#define NDT2D_SPARSECOV_PHASE() ((void)0)
#endif

// Node i of n, eliminated at stride s: its 24 doubles from those of lo and hi.
NDT2D_PG_HD inline void select_node(const chain::System & m, double * sel, size_t n, size_t i, size_t s)
{
  const size_t lo = i - s, hi = i + s;
  const bool above = hi < n;
  double * out = sel + kSelectDoubles * i;
  double T1[9], T2[9], X[9];
  {
    double L[9], Gll[9];
    for (int k = 0; k < 9; ++k) L[k] = m.L[9 * i + k];
    full(sel + kSelectDoubles * lo, Gll);
    chain::mtm(L, Gll, T1);                      // L^T G_lo,lo
    for (int k = 0; k < 9; ++k) T2[k] = 0.0;
    if (above)
    {
      NDT2D_SPARSECOV_PHASE();
      double Glh[9];
      if ((lo / (2 * s)) & 1u)
      {
        for (int k = 0; k < 9; ++k) Glh[k] = sel[kSelectDoubles * lo + 15 + k];
      }
      else
      {
        transposed(sel + kSelectDoubles * hi + 6, Glh);
      }
      chain::mtm(L, Glh, T2);                    // L^T G_lo,hi
      NDT2D_SPARSECOV_PHASE();
      double U[9];
      for (int k = 0; k < 9; ++k) U[k] = m.U[9 * i + k];
      chain::mmt(U, Glh, X);                     // U G_hi,lo
      for (int k = 0; k < 9; ++k) T1[k] += X[k];
      NDT2D_SPARSECOV_PHASE();
      double Ghh[9];
      full(sel + kSelectDoubles * hi, Ghh);
      chain::mm(U, Ghh, X);                      // U G_hi,hi
      for (int k = 0; k < 9; ++k) T2[k] += X[k];
    }
  }
  NDT2D_SPARSECOV_PHASE();
  double P[9], Gl[9], Gh[9];
  double Pi[6];
  chain::pivot_inverse(m.P + 6 * i, Pi);
  full(Pi, P);
  chain::mm(P, T1, Gl);
  chain::mm(P, T2, Gh);
  for (int k = 0; k < 9; ++k)
  {
    Gl[k] = -Gl[k];
    Gh[k] = above ? -Gh[k] : 0.0;
    out[6 + k] = Gl[k];
    out[15 + k] = Gh[k];
  }
  NDT2D_SPARSECOV_PHASE();
  {
    double L[9];
    for (int k = 0; k < 9; ++k) L[k] = m.L[9 * i + k];
    chain::mm(Gl, L, T1);                        // G_i,lo L
  }
  if (above)
  {
    NDT2D_SPARSECOV_PHASE();
    double U[9];
    for (int k = 0; k < 9; ++k) U[k] = m.U[9 * i + k];
    chain::mmt(Gh, U, X);                        // G_i,hi U^T
    for (int k = 0; k < 9; ++k) T1[k] += X[k];
  }
  chain::mm(T1, P, X);
  out[0] = P[0] - X[0];
  out[1] = P[1] - X[1];
  out[2] = P[2] - X[2];
  out[3] = P[4] - X[4];
  out[4] = P[5] - X[5];
  out[5] = P[8] - X[8];
}

// ---- the assembly of a block of Sigma ----

// What node reaches Sigma_ss with: C[0], C[1] row-major -- a separator the identity (and nothing),
// an interior node -Z_left and -Z_right.
NDT2D_PG_HD inline void coefficients(const sparse::Tables & t, const sparse::Interior & in, uint32_t node, double (*C)[9])
{
  for (int k = 0; k < 9; ++k) C[0][k] = C[1][k] = 0.0;
  if (t.separator(node))
  {
    C[0][0] = C[0][4] = C[0][8] = 1.0;
    return;
  }
  const double * x = in.x + sparse::kColumnDoubles * static_cast<size_t>(t.index(node));
  for (int r = 0; r < 3; ++r)
  {
    for (int c = 0; c < 3; ++c)
    {
      C[0][3 * r + c] = -x[3 * (1 + c) + r];
      C[1][3 * r + c] = -x[3 * (4 + c) + r];
    }
  }
}

// X = sum over ia, ib of Ca[ia] B(slot[2 ia + ib]) Cb[ib]^T, B a block of the table of S^-1's blocks
// (or its transpose); a slot that is kNone adds nothing.
NDT2D_PG_HD inline void sandwich(const double * table, const uint32_t * slot, const double (*Ca)[9], const double (*Cb)[9], double * X)
{
  for (int k = 0; k < 9; ++k) X[k] = 0.0;
  for (int ia = 0; ia < 2; ++ia)
  {
    for (int ib = 0; ib < 2; ++ib)
    {
      const uint32_t at = slot[2 * ia + ib];
      if (at == kNone) continue;
      const double * stored = table + 9 * static_cast<size_t>(at & ~kSlotTransposed);
      double B[9], M[9], Y[9];
      if (at & kSlotTransposed) transposed(stored, B);
      else
      {
        for (int k = 0; k < 9; ++k) B[k] = stored[k];
      }
      chain::mmt(B, Cb[ib], M);
      chain::mm(Ca[ia], M, Y);
      for (int k = 0; k < 9; ++k) X[k] += Y[k];
    }
  }
}

// Sigma_kk of node k, row-major: a separator's block of S^-1; an interior node's G_kk + the four
// separator terms, the upper triangle computed and mirrored.
NDT2D_PG_HD inline void diagonal_block(const sparse::Tables & t, const sparse::Interior & in, const double * sel, const double * table, uint32_t node,
                                       double * out)
{
  if (t.separator(node))
  {
    const double * B = table + 9 * static_cast<size_t>(t.index(node));
    for (int k = 0; k < 9; ++k) out[k] = B[k];
    return;
  }
  const size_t k = t.index(node);
  const uint32_t u = t.before[k], w = t.after[k];
  uint32_t slot[4] = {u, kNone, kNone, w};
  if (u != kNone && w != kNone)
  {
    slot[1] = t.s + u;                            // (w == u + 1: an interior node lies between consecutive separators)
    slot[2] = (t.s + u) | kSlotTransposed;
  }
  double C[2][9], X[9];
  coefficients(t, in, node, C);
  sandwich(table, slot, C, C, X);
  const double * G = sel + kSelectDoubles * k;
  out[0] = G[0] + X[0];
  out[1] = out[3] = G[1] + X[1];
  out[2] = out[6] = G[2] + X[2];
  out[4] = G[3] + X[4];
  out[5] = out[7] = G[4] + X[5];
  out[8] = G[5] + X[8];
}

// The block of an asked pair from its words (sparsecov/ndt2d_sparsecov_plan.h) and its G_ab (read
// where the pair has a pass), row-major, as the caller asked for it.
NDT2D_PG_HD inline void pair_block(const sparse::Tables & t, const sparse::Interior & in, const double * sel, const double * table, const uint32_t * words,
                                   const double * gab, double * out)
{
  const uint32_t a = words[0], b = words[1];
  if (a == b)
  {
    diagonal_block(t, in, sel, table, a, out);
    return;
  }
  double Ca[2][9], Cb[2][9], X[9];
  coefficients(t, in, a, Ca);
  coefficients(t, in, b, Cb);
  sandwich(table, words + 2, Ca, Cb, X);
  if (words[6] != kNone)
  {
    for (int k = 0; k < 9; ++k) X[k] += gab[k];
  }
  if (words[7] & kFlagTransposed) transposed(X, out);
  else
  {
    for (int k = 0; k < 9; ++k) out[k] = X[k];
  }
}

// ---- a column pass: G E_b through the reduction's right-hand-side, root and back levels with three
// columns (sparse::forward_columns<3>, root_columns<3>, back_columns<3>).  The right-hand sides are
// the first nine doubles of a node's b, the solutions the nine behind them: b is free once Z is known. ----

constexpr int kPassColumns = 3;
constexpr size_t kPassSolution = 3 * kPassColumns;   // where a node's solution lies in its b

NDT2D_PG_HD inline void pass_seed(double * b, size_t ii, size_t column)
{
  double * at = b + sparse::kColumnDoubles * ii;
  for (int k = 0; k < 9; ++k) at[k] = 0.0;
  if (ii == column) at[0] = at[4] = at[8] = 1.0;
}

// G_ab, row-major, from the pass of b's interior index: column c of the solution at a is G_ab's column c.
NDT2D_PG_HD inline void pass_gather(const double * b, size_t ia, double * gab)
{
  const double * x = b + sparse::kColumnDoubles * ia + kPassSolution;
  for (int r = 0; r < 3; ++r)
  {
    for (int c = 0; c < 3; ++c) gab[3 * r + c] = x[3 * c + r];
  }
}

// ---- the sequential driver (host) ----

// Every node's block and the asked pairs' over one system.  In: in.m.D, in.m.U, in.Cl, in.Cr as
// assembled; S the separators' A_ss (its lower triangle and diagonal blocks, the identity from 3 s on),
// T [ld][ld] anything; active [n] whether a node is free.  sel [24 n_i], table [9 blocks],
// columns [9 pairs], zero [3 n] zeros, gs [3 s], diag [ld] are its scratch.  Out: diagonal [n][9],
// pairs [P][9]; *stage 0, or 1 where a pivot of the reduction, 2 where a pivot of S was not
// positive -- the blocks are then zero; *ratio the smallest pivot / diagonal of S (1 without a separator).
inline void compute(const sparse::Tables & t, const sparse::Interior & in, double * S, double * T, size_t ld, double * diag, const uint8_t * active,
                    const Lists & lists, double * sel, double * table, double * columns, const double * zero, double * gs, double * diagonal,
                    double * pairs, int * stage, double * ratio)
{
  const size_t ni = t.ni, dim = 3 * static_cast<size_t>(t.s), P = lists.n_pairs();
  for (size_t k = 0; k < 9 * static_cast<size_t>(t.n); ++k) diagonal[k] = 0.0;
  for (size_t k = 0; k < 9 * P; ++k) pairs[k] = 0.0;
  *stage = 0;
  *ratio = 1.0;
  for (uint32_t i = 0; i < t.n; ++i)
  {
    if (!t.separator(i)) sparse::set_columns(in, t.index(i), zero + 3 * static_cast<size_t>(i));
  }
  const bool reduced = chain::factor(in.m, ni);
  if (ni != 0)
  {
    for (size_t s = 1; s < ni; s *= 2)
    {
      const size_t count = chain::stay_count(ni, s);
      for (size_t q = 0; q < count; ++q) sparse::forward_columns<sparse::kColumns>(in.m, in.b, ni, chain::stay_node(s, q), s);
    }
    sparse::root_columns<sparse::kColumns>(in.m, in.b, in.x);
    for (size_t s = chain::top_stride(ni); s >= 1; s /= 2)
    {
      const size_t count = chain::gone_count(ni, s);
      for (size_t q = 0; q < count; ++q) sparse::back_columns<sparse::kColumns>(in.m, in.b, in.x, ni, chain::gone_node(s, q), s);
    }
  }
  for (uint32_t si = 0; si < t.s; ++si) sparse::schur_separator(t, in, zero, si, S, ld, diag, gs);
  bool factored = true;
  for (size_t j = 0; j < dim && factored; ++j)   // S = L L^T in its lower triangle
  {
    double pivot = S[j * ld + j];
    for (size_t k = 0; k < j; ++k) pivot -= S[j * ld + k] * S[j * ld + k];
    if (!(pivot > 0.0) || !(pivot <= 1.7976931348623157e308))
    {
      factored = false;
      break;
    }
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
  if (!reduced) *stage = 1;
  else if (!factored) *stage = 2;
  if (*stage != 0) return;
  for (size_t j = 0; j < dim; ++j)   // T = L^-1, column by column
  {
    for (size_t i = 0; i < j; ++i) T[i * ld + j] = 0.0;
    T[j * ld + j] = 1.0 / S[j * ld + j];
    for (size_t i = j + 1; i < dim; ++i)
    {
      double v = 0.0;
      for (size_t k = j; k < i; ++k) v += S[i * ld + k] * T[k * ld + j];
      T[i * ld + j] = -v / S[i * ld + i];
    }
  }
  for (size_t e = 0; e < lists.n_blocks(); ++e)   // the blocks of S^-1 = T^T T
  {
    const size_t x = lists.blocks[2 * e], y = lists.blocks[2 * e + 1];
    for (int r = 0; r < 3; ++r)
    {
      for (int c = 0; c < 3; ++c)
      {
        double v = 0.0;
        for (size_t k = 3 * y; k < dim; ++k) v += T[k * ld + 3 * x + r] * T[k * ld + 3 * y + c];
        table[9 * e + 3 * r + c] = v;
      }
    }
  }
  if (ni != 0)
  {
    select_root(in.m, sel);
    for (size_t s = chain::top_stride(ni); s >= 1; s /= 2)
    {
      const size_t count = chain::gone_count(ni, s);
      for (size_t q = 0; q < count; ++q) select_node(in.m, sel, ni, chain::gone_node(s, q), s);
    }
  }
  for (size_t p = 0; p < lists.n_passes(); ++p)
  {
    const size_t column = lists.passes[p];
    for (size_t ii = 0; ii < ni; ++ii) pass_seed(in.b, ii, column);
    for (size_t s = 1; s < ni; s *= 2)
    {
      const size_t count = chain::stay_count(ni, s);
      for (size_t q = 0; q < count; ++q) sparse::forward_columns<kPassColumns>(in.m, in.b, ni, chain::stay_node(s, q), s);
    }
    sparse::root_columns<kPassColumns>(in.m, in.b, in.b + kPassSolution);
    for (size_t s = chain::top_stride(ni); s >= 1; s /= 2)
    {
      const size_t count = chain::gone_count(ni, s);
      for (size_t q = 0; q < count; ++q) sparse::back_columns<kPassColumns>(in.m, in.b, in.b + kPassSolution, ni, chain::gone_node(s, q), s);
    }
    for (size_t q = 0; q < P; ++q)
    {
      const uint32_t * w = lists.pairs.data() + q * kPairWords;
      if (w[6] == p) pass_gather(in.b, t.index(w[0]), columns + 9 * q);
    }
  }
  for (uint32_t i = 0; i < t.n; ++i)
  {
    if (active[i]) diagonal_block(t, in, sel, table, i, diagonal + 9 * static_cast<size_t>(i));
  }
  for (size_t q = 0; q < P; ++q)
  {
    const uint32_t * w = lists.pairs.data() + q * kPairWords;
    if (active[w[0]] && active[w[1]]) pair_block(t, in, sel, table, w, columns + 9 * q, pairs + 9 * q);
  }
}

}  // namespace sparsecov
}  // namespace ndt2d

#endif  // NDT2D_SPARSECOV_SELECT_H_
