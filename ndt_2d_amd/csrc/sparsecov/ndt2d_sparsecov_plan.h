// The plan of the sparse covariance (sparsecov/ndt2d_sparsecov.hip; include/ndt2d_hip.h, "Sparse
// covariance"): what a job holds on the device, in doubles, how many jobs a byte budget holds, what
// the call refuses, and the lists the host derives from the graph's layout and the asked pairs --
// the blocks of S^-1 that are wanted, the asked pairs as the kernels take them, and the column passes
// of the reduction that give G_ab.  Plain C++ without HIP types, host and device; a stand-alone host
// program walks it (tests/cpp/sparsecov_plan_check.cpp).  The layout, the tables and the interior
// region are the sparse solve's (sparse/ndt2d_sparse_plan.h), the padding of the separators' dense
// matrices the dense covariance's (covariance/ndt2d_covariance_plan.h).
//
// With A = [A_ii A_is; A_si A_ss], Z = A_ii^-1 A_is, S = A_ss - A_si Z and G = A_ii^-1:
//     Sigma_ss = S^-1,  Sigma_is = -Z Sigma_ss,  Sigma_ii = G + Z Sigma_ss Z^T.
// A node has at most two separators it reaches Sigma_ss through -- a separator itself (with the
// identity), an interior node the separator before it and the one after it (with -Z_left, -Z_right) --
// so a block of Sigma takes at most four blocks of S^-1.
//
// The blocks of S^-1, 9 doubles each, one table a job.  Block (x, y), x <= y separator indices, lies at
//   x                  x == y          (always there)
//   s + x              y == x + 1      (always there: an interior node's two separators)
//   2 s - 1 + e        the e-th other block the asked pairs touch, in the order they first ask for it
// and (y, x) is its transpose.
//
// An asked pair, kPairWords 32-bit words: {a, b, slot[4], pass, flags}.  a <= b are the pair's nodes
// in ascending order: the block is computed for (a, b) and written transposed where the caller asked
// for (b, a) (flags & kFlagTransposed).  slot[2 ia + ib] is the block of S^-1 between a's ia-th and
// b's ib-th separator: its place in the table, | kSlotTransposed where the table holds the transpose,
// or kNone.  pass: the column pass whose solution holds G_ab (two interior nodes of one segment,
// a != b), or kNone.
//
// A chunk's workspace is regions, each [job][...]:
//   inverse    T = L^-1 of the separators' factor, padded(3 s)^2, the jobs in DESCENDING order in
//              front of `schur` (a job's T lies (job + 1) matrices before the region behind it: the
//              dense covariance's kernels form a job's layout from one pointer, n and the job)
//   schur      the sparse solve's: S, its diagonal, a vector -- sparse::schur_doubles(s)
//   interior   the sparse solve's, kInteriorDoubles an interior node
//   select     per interior node kSelectDoubles: G_ii (6, symmetric), G_i,lo (9), G_i,hi (9)
//   vectors    the sparse solve's, 6 s (what its Schur kernel writes beside S)
//   blocks     the table of S^-1's blocks, 9 each
//   columns    G_ab of each asked pair, 9 each
//   work       the solver's PgWork, kNodeDoubles a node, m doubles in front under a loss
//   state      the LM state the sparse solve's kernels read, the dense factor's record, the
//              reduction's flag -- sparse::kStateDoubles
#ifndef NDT2D_SPARSECOV_PLAN_H_
#define NDT2D_SPARSECOV_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "covariance/ndt2d_covariance_plan.h"
#include "sparse/ndt2d_sparse_plan.h"

namespace ndt2d
{
namespace sparsecov
{

constexpr uint32_t kNone = sparse::kNone;
constexpr size_t kSelectDoubles = 6 + 9 + 9;
constexpr size_t kPairWords = 8;
constexpr uint32_t kSlotTransposed = 0x80000000u;
constexpr uint32_t kFlagTransposed = 1u;
constexpr size_t kMaxBlocks = 0x7fffffffu;   // a block a workgroup of a launch, a slot in 31 bits

// ---- a job's doubles ----

NDT2D_COV_HD inline size_t inverse_doubles(size_t s)
{
  const size_t ld = covariance::padded(3 * s);
  return ld * ld;
}

NDT2D_COV_HD inline size_t select_doubles(size_t ni) { return kSelectDoubles * ni; }

NDT2D_COV_HD inline size_t job_doubles(size_t n, size_t s, size_t m, bool loss, size_t blocks, size_t pairs)
{
  return inverse_doubles(s) + sparse::schur_doubles(s) + sparse::interior_doubles(n - s) + select_doubles(n - s) + sparse::vector_doubles(s) +
         9 * blocks + 9 * pairs + sparse::work_doubles(n, m, loss) + sparse::kStateDoubles;
}

// The jobs of a chunk: what the budget holds, at most max_jobs; 0 where not even one fits.
NDT2D_COV_HD inline size_t chunk_jobs(size_t max_jobs, size_t workspace_bytes, size_t job_bytes)
{
  return covariance::chunk_jobs(max_jobs, workspace_bytes, job_bytes);
}

// The blocks of S^-1 that are always there.
NDT2D_COV_HD inline size_t fixed_blocks(size_t s) { return s == 0 ? 0 : 2 * s - 1; }

// What a call refuses about the graph (the text, prefixed with `entry`, or an empty string): the
// sparse solve's limits, more blocks than a launch holds, a job that does not fit the budget.
inline std::string refusal(const char * entry, size_t n, size_t s, size_t blocks, size_t pairs, size_t chunk, size_t job_bytes,
                           size_t workspace_bytes)
{
  const std::string graph = sparse::refusal(entry, n, s, 1, job_bytes, workspace_bytes);
  if (!graph.empty()) return graph;
  if (blocks > kMaxBlocks || pairs > kMaxBlocks) return std::string(entry) + ": more than 2^31 - 1 blocks a job";
  return sparse::refusal(entry, n, s, chunk, job_bytes, workspace_bytes);
}

// ---- the lists (host) ----

// The separators a node reaches Sigma_ss through: its own index, or the interior node's before and
// after; kNone where there is none.
inline void reach(const sparse::Tables & t, uint32_t node, uint32_t out[2])
{
  if (t.separator(node))
  {
    out[0] = t.index(node);
    out[1] = kNone;
    return;
  }
  out[0] = t.before[t.index(node)];
  out[1] = t.after[t.index(node)];
}

struct Lists
{
  std::vector<uint32_t> blocks;   // [n_blocks][2]: (x, y), x <= y, in the table's order
  std::vector<uint32_t> pairs;    // [n_pairs][kPairWords]
  std::vector<uint32_t> passes;   // [n_passes]: the interior index of the node whose three columns of G a pass solves for
  size_t n_blocks() const { return blocks.size() / 2; }
  size_t n_pairs() const { return pairs.size() / kPairWords; }
  size_t n_passes() const { return passes.size(); }
};

// The lists for the asked pairs [n_pairs][2] (node ids below t.n) on the layout t.  A pair's words
// depend on the pairs before it only through the places of its blocks and its pass, never its values.
inline void make_lists(const sparse::Tables & t, const uint32_t * asked, size_t n_pairs, Lists * out)
{
  const uint32_t s = t.s;
  out->blocks.clear();
  out->pairs.assign(n_pairs * kPairWords, kNone);
  out->passes.clear();
  for (uint32_t x = 0; x < s; ++x)
  {
    out->blocks.push_back(x);
    out->blocks.push_back(x);
  }
  for (uint32_t x = 0; x + 1 < s; ++x)
  {
    out->blocks.push_back(x);
    out->blocks.push_back(x + 1);
  }
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> extra;
  std::map<uint32_t, uint32_t> pass_of;
  const auto place = [&](uint32_t x, uint32_t y) -> uint32_t {
    if (x == kNone || y == kNone) return kNone;
    const uint32_t flag = x > y ? kSlotTransposed : 0u;
    const uint32_t lo = x > y ? y : x, hi = x > y ? x : y;
    if (lo == hi) return lo;
    if (hi == lo + 1) return (s + lo) | flag;
    const auto key = std::make_pair(lo, hi);
    auto found = extra.find(key);
    if (found == extra.end())
    {
      found = extra.emplace(key, static_cast<uint32_t>(out->blocks.size() / 2)).first;
      out->blocks.push_back(lo);
      out->blocks.push_back(hi);
    }
    return found->second | flag;
  };
  for (size_t q = 0; q < n_pairs; ++q)
  {
    uint32_t * w = out->pairs.data() + q * kPairWords;
    const uint32_t first = asked[2 * q], second = asked[2 * q + 1];
    const uint32_t a = first < second ? first : second, b = first < second ? second : first;
    w[0] = a;
    w[1] = b;
    w[7] = first > second ? kFlagTransposed : 0u;
    uint32_t ra[2], rb[2];
    reach(t, a, ra);
    reach(t, b, rb);
    for (int ia = 0; ia < 2; ++ia)
    {
      for (int ib = 0; ib < 2; ++ib) w[2 + 2 * ia + ib] = place(ra[ia], rb[ib]);
    }
    if (a != b && !t.separator(a) && !t.separator(b) && ra[0] == rb[0])   // one segment: the same separator before both
    {
      const uint32_t column = t.index(b);
      auto found = pass_of.find(column);
      if (found == pass_of.end())
      {
        found = pass_of.emplace(column, static_cast<uint32_t>(out->passes.size())).first;
        out->passes.push_back(column);
      }
      w[6] = found->second;
    }
  }
}

// The words of the lists as one array behind the layout's tables: [blocks | pairs | passes].
NDT2D_COV_HD inline size_t list_words(size_t blocks, size_t pairs, size_t passes) { return 2 * blocks + kPairWords * pairs + passes; }

}  // namespace sparsecov
}  // namespace ndt2d

#endif  // NDT2D_SPARSECOV_PLAN_H_
