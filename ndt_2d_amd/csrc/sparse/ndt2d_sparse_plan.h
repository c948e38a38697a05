// The plan of the sparse pose-graph solve (sparse/ndt2d_sparse.hip; include/ndt2d_hip.h, "Sparse
// solve"): which nodes are separators, the tables the kernels index with, what a job holds on the
// device, in doubles, how many jobs a byte budget holds, and what the call refuses.  Plain C++
// without HIP types, host and device; a stand-alone host program walks it
// (tests/cpp/sparse_plan_check.cpp).  The panels and the padding of the separators' dense matrix are
// the dense covariance's (covariance/ndt2d_covariance_plan.h).
//
// A constraint is a chain edge when |begin - end| == 1, a closure edge otherwise.  A node that is an
// end of a closure edge of the graph -- whatever a job's mask says -- is a separator; every other
// node is interior.  Both kinds are numbered in node order: s separators, n_i interior nodes.  The
// fixed node and the nodes a mask leaves without a constraint keep their place in the layout (an
// identity block, no coupling): the layout is one per graph.
//
// The tables, one array of 32-bit words [n + 2 n_i + 3 s]:
//   role     [n]    (the node's index among its kind) << 1 | (it is a separator)
//   before   [n_i]  the index of the nearest separator before the interior node, or kNone
//   after    [n_i]  ... behind it, or kNone
//   node     [s]    the separator's node
//   previous [s]    the interior index of node - 1 where that is an interior node, or kNone
//   next     [s]    ... of node + 1
//
// A chunk's workspace is five regions, each [job][...]:
//   interior  per interior node kInteriorDoubles: the reduction's D (6), U (9), L (9), P (6); the
//             seven right-hand-side columns, reduced in place (21); their solutions y, Z_left, Z_right
//             (21); the couplings A(i, i - 1) and A(i, i + 1) to a separator as assembled (9 + 9)
//   schur     the separators' matrix S (then its factor), padded(3 s)^2; its diagonal, padded(3 s);
//             the substitution's vector, padded(3 s)                       -- schur_doubles(s)
//   vectors   -b_s and delta_s, 3 s each
//   work      the solver's PgWork, kNodeDoubles a node, m doubles in front under a loss
//   state     the LM state, the dense factor's record and the reduction's flag -- kStateDoubles
#ifndef NDT2D_SPARSE_PLAN_H_
#define NDT2D_SPARSE_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "covariance/ndt2d_covariance_plan.h"

namespace ndt2d
{
namespace sparse
{

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kColumns = 7;                 // -g_i, the three of R_left, the three of R_right
constexpr size_t kInteriorDoubles = 6 + 9 + 9 + 6 + 3 * kColumns + 3 * kColumns + 9 + 9;
constexpr size_t kNodeDoubles = 41;         // kPgNodeDoubles (the kernel header holds them equal)
constexpr size_t kStateDoubles = 17;        // the direct solve's 16 and the reduction's flag
constexpr size_t kMaxNodes = size_t(1) << 30;               // kPgMaxNodes
constexpr size_t kMaxDim = covariance::kMaxDim;             // what the substitution's vector holds

NDT2D_COV_HD inline bool chain_edge(uint32_t begin, uint32_t end) { return (begin < end ? end - begin : begin - end) == 1u; }

// The tables as the kernels and the host's driver index them.
struct Tables
{
  const uint32_t * role, * before, * after, * node, * previous, * next;
  uint32_t n, s, ni;
  NDT2D_COV_HD bool separator(uint32_t i) const { return (role[i] & 1u) != 0u; }
  NDT2D_COV_HD uint32_t index(uint32_t i) const { return role[i] >> 1; }
};

NDT2D_COV_HD inline size_t table_words(size_t n, size_t s) { return n + 2 * (n - s) + 3 * s; }

NDT2D_COV_HD inline Tables tables_at(const uint32_t * words, size_t n, size_t s)
{
  Tables t;
  const size_t ni = n - s;
  t.role = words;
  t.before = t.role + n;
  t.after = t.before + ni;
  t.node = t.after + ni;
  t.previous = t.node + s;
  t.next = t.previous + s;
  t.n = static_cast<uint32_t>(n);
  t.s = static_cast<uint32_t>(s);
  t.ni = static_cast<uint32_t>(ni);
  return t;
}

// The layout of a graph of n nodes and m constraints (host): the words of the tables.
struct Layout
{
  size_t n = 0, s = 0, ni = 0;
  std::vector<uint32_t> words;
  Tables tables() const { return tables_at(words.data(), n, s); }
};

inline void make_layout(size_t n, size_t m, const uint32_t * begin, const uint32_t * end, Layout * out)
{
  std::vector<uint8_t> sep(n, 0);
  for (size_t c = 0; c < m; ++c)
  {
    if (chain_edge(begin[c], end[c])) continue;
    sep[begin[c]] = 1;
    sep[end[c]] = 1;
  }
  size_t s = 0;
  for (size_t i = 0; i < n; ++i) s += sep[i];
  out->n = n;
  out->s = s;
  out->ni = n - s;
  out->words.assign(table_words(n, s), kNone);
  uint32_t * role = out->words.data(), * before = role + n, * after = before + out->ni, * node = after + out->ni, * previous = node + s,
           * next = previous + s;
  uint32_t si = 0, ii = 0, last = kNone;
  for (size_t i = 0; i < n; ++i)
  {
    if (sep[i])
    {
      role[i] = si << 1 | 1u;
      node[si] = static_cast<uint32_t>(i);
      last = si++;
    }
    else
    {
      role[i] = ii << 1;
      before[ii++] = last;
    }
  }
  last = kNone;
  for (size_t k = n; k > 0; --k)
  {
    const size_t i = k - 1;
    if (sep[i]) last = role[i] >> 1;
    else after[role[i] >> 1] = last;
  }
  for (size_t i = 0; i < n; ++i)
  {
    if (!sep[i]) continue;
    const uint32_t at = role[i] >> 1;
    if (i > 0 && !sep[i - 1]) previous[at] = role[i - 1] >> 1;
    if (i + 1 < n && !sep[i + 1]) next[at] = role[i + 1] >> 1;
  }
}

// ---- a job's doubles ----

NDT2D_COV_HD inline size_t interior_doubles(size_t ni) { return kInteriorDoubles * ni; }

NDT2D_COV_HD inline size_t schur_doubles(size_t s)
{
  const size_t ld = covariance::padded(3 * s);
  return ld * ld + 2 * ld;
}

NDT2D_COV_HD inline size_t vector_doubles(size_t s) { return 6 * s; }

NDT2D_COV_HD inline size_t work_doubles(size_t n, size_t m, bool loss) { return kNodeDoubles * n + (loss ? m : 0); }

NDT2D_COV_HD inline size_t job_doubles(size_t n, size_t s, size_t m, bool loss)
{
  return interior_doubles(n - s) + schur_doubles(s) + vector_doubles(s) + work_doubles(n, m, loss) + kStateDoubles;
}

// The jobs of a chunk: what the budget holds, at most max_jobs; 0 where not even one fits.
NDT2D_COV_HD inline size_t chunk_jobs(size_t max_jobs, size_t workspace_bytes, size_t job_bytes)
{
  return covariance::chunk_jobs(max_jobs, workspace_bytes, job_bytes);
}

// What a solve refuses about the graph (the text, prefixed with `entry`, or an empty string): more
// nodes than the solver's, more separators than the substitution's vector holds, a job that does
// not fit the budget.
inline std::string refusal(const char * entry, size_t n, size_t s, size_t chunk, size_t job_bytes, size_t workspace_bytes)
{
  if (n > kMaxNodes) return std::string(entry) + ": " + std::to_string(n) + " poses, the solver holds " + std::to_string(kMaxNodes);
  if (covariance::padded(3 * s) > kMaxDim)
  {
    return std::string(entry) + ": " + std::to_string(s) + " separators, the dense matrix holds " + std::to_string(kMaxDim / 3);
  }
  if (chunk == 0)
  {
    return std::string(entry) + ": a job of " + std::to_string(n) + " poses and " + std::to_string(s) + " separators needs " +
           std::to_string(job_bytes) + " bytes, the workspace is " + std::to_string(workspace_bytes);
  }
  return std::string();
}

}  // namespace sparse
}  // namespace ndt2d

#endif  // NDT2D_SPARSE_PLAN_H_
