// csrc/sparse/ndt2d_sparse_plan.h in a program of its own: the separator set and the tables of
// designed graphs against a restatement written here, every table index in range, the byte counts
// and the refusals.  Prints "ok" and returns 0, or says what failed.
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "sparse/ndt2d_sparse_plan.h"

namespace sp = ndt2d::sparse;
namespace cov = ndt2d::covariance;

namespace
{

int failures = 0;

void expect(bool ok, const char * what, const char * name)
{
  if (ok) return;
  std::printf("FAILED: %s (%s)\n", what, name);
  ++failures;
}

typedef std::vector<std::pair<uint32_t, uint32_t>> Edges;

// The layout of the graph against the definitions, by brute force; want: the separators' nodes.
void check(const char * name, size_t n, const Edges & edges, const std::vector<uint32_t> & want)
{
  std::vector<uint32_t> begin, end;
  for (const auto & e : edges)
  {
    begin.push_back(e.first);
    end.push_back(e.second);
  }
  sp::Layout L;
  L.words.assign(3, 7u);   // (what an earlier graph left)
  sp::make_layout(n, edges.size(), begin.data(), end.data(), &L);
  expect(L.n == n && L.s == want.size() && L.ni == n - want.size(), "the counts", name);
  expect(L.words.size() == sp::table_words(n, L.s) && L.words.size() == n + 2 * L.ni + 3 * L.s, "the words", name);
  if (L.s != want.size() || L.words.size() != sp::table_words(n, L.s)) return;
  const sp::Tables t = L.tables();
  expect(t.n == n && t.s == L.s && t.ni == L.ni, "the tables' counts", name);
  std::vector<uint8_t> sep(n, 0);
  for (uint32_t v : want) sep[v] = 1;
  uint32_t si = 0, ii = 0;
  for (uint32_t i = 0; i < n; ++i)
  {
    expect(t.separator(i) == (sep[i] != 0), "a node's role", name);
    if (sep[i])
    {
      expect(t.index(i) == si && si < t.s && t.node[si] == i, "a separator's index and node", name);
      // the interior neighbours
      const uint32_t prev = i > 0 && !sep[i - 1] ? t.index(i - 1) : sp::kNone, next = i + 1 < n && !sep[i + 1] ? t.index(i + 1) : sp::kNone;
      expect(t.previous[si] == prev && t.next[si] == next, "a separator's interior neighbours", name);
      expect((prev == sp::kNone || prev < t.ni) && (next == sp::kNone || next < t.ni), "a neighbour's range", name);
      ++si;
    }
    else
    {
      expect(t.index(i) == ii && ii < t.ni, "an interior node's index", name);
      uint32_t before = sp::kNone, after = sp::kNone;
      for (uint32_t j = 0; j < i; ++j)
      {
        if (sep[j]) before = t.index(j);
      }
      for (uint32_t j = static_cast<uint32_t>(n); j > i + 1; --j)
      {
        if (sep[j - 1]) after = t.index(j - 1);
      }
      expect(t.before[ii] == before && t.after[ii] == after, "an interior node's separators", name);
      expect((before == sp::kNone || before < t.s) && (after == sp::kNone || after < t.s), "a separator's range", name);
      ++ii;
    }
  }
  expect(si == t.s && ii == t.ni, "every node has a place", name);
}

Edges chain(uint32_t n)
{
  Edges e;
  for (uint32_t i = 0; i + 1 < n; ++i) e.push_back({i, i + 1});
  return e;
}

Edges with(Edges e, const Edges & more)
{
  e.insert(e.end(), more.begin(), more.end());
  return e;
}

}  // namespace

int main()
{
  // the designed graphs (the fixed node is no part of the layout: the same tables wherever it lies --
  // inside a segment or on a separator, it is an identity block there)
  check("no closure", 9, chain(9), {});
  check("no constraint", 4, {}, {});
  check("one pose", 1, {}, {});
  check("separators at node 0 and n - 1", 8, with(chain(8), {{0, 7}}), {0, 7});
  check("adjacent separators, a segment of length 0", 10, with(chain(10), {{2, 6}, {3, 8}}), {2, 3, 6, 8});
  check("segments of length 1 and 2", 10, with(chain(10), {{1, 3}, {3, 6}, {9, 6}}), {1, 3, 6, 9});
  check("a hub", 12, with(chain(12), {{5, 0}, {5, 2}, {5, 8}, {5, 11}, {11, 5}}), {0, 2, 5, 8, 11});
  check("every node a separator", 6, with(chain(6), {{0, 2}, {1, 3}, {2, 4}, {3, 5}}), {0, 1, 2, 3, 4, 5});
  check("reversed chain edges and a duplicate are chain edges", 5, {{1, 0}, {1, 2}, {2, 1}, {3, 2}, {3, 4}}, {});
  check("a closure without a chain", 5, {{0, 3}}, {0, 3});
  check("a self edge is a closure edge", 4, with(chain(4), {{2, 2}}), {2});
  check("a long chain", 2100, with(chain(2100), {{10, 2000}, {1024, 3}}), {3, 10, 1024, 2000});
  expect(sp::chain_edge(0, 1) && sp::chain_edge(1, 0) && !sp::chain_edge(0, 0) && !sp::chain_edge(0, 2) && !sp::chain_edge(0xffffffffu, 0),
         "chain_edge", "edges");

  // the byte counts: 90 doubles an interior node, padded(3 s)^2 + 2 padded(3 s) + 6 s, 41 n [+ m], 17
  expect(sp::kInteriorDoubles == 90 && sp::kColumns == 7 && sp::kStateDoubles == 17 && sp::kNodeDoubles == 41, "the constants", "bytes");
  expect(sp::schur_doubles(0) == 0 && sp::schur_doubles(1) == 48 * 48 + 96 && sp::schur_doubles(16) == 48 * 48 + 96 &&
         sp::schur_doubles(17) == 96 * 96 + 192 && sp::schur_doubles(33) == 144 * 144 + 288, "schur_doubles", "bytes");
  expect(sp::job_doubles(10, 0, 9, false) == 900 + 410 + 17, "a job without a separator", "bytes");
  expect(sp::job_doubles(10, 4, 12, false) == 6 * 90 + (48 * 48 + 96) + 24 + 410 + 17, "a job with separators", "bytes");
  expect(sp::job_doubles(10, 4, 12, true) == sp::job_doubles(10, 4, 12, false) + 12, "a job under a loss", "bytes");
  expect(sp::job_doubles(6, 6, 9, false) == (48 * 48 + 96) + 36 + 246 + 17, "every node a separator", "bytes");
  expect(sp::chunk_jobs(8, 1000, 100) == 8 && sp::chunk_jobs(8, 799, 100) == 7 && sp::chunk_jobs(8, 99, 100) == 0, "chunk_jobs", "bytes");
  // 10,000 poses with 101 closures: 202 separators at most, under 16 MB a job (the direct solve: 7.2 GB)
  expect(sp::job_doubles(10000, 202, 10100, false) * 8 < 16u * 1000u * 1000u, "10,000 poses", "bytes");

  // the refusals
  const char * entry = "ndt2d_sparse_solve";
  expect(sp::refusal(entry, 100, 10, 3, 8000, 1 << 20).empty(), "a graph that fits", "refusals");
  expect(sp::refusal(entry, 100, 10, 0, 123456, 1000) == "ndt2d_sparse_solve: a job of 100 poses and 10 separators needs 123456 bytes, the workspace is 1000",
         "the budget's text", "refusals");
  expect(sp::refusal(entry, 30000, 21840, 1, 8, 1 << 20).empty() && cov::padded(3 * 21840) == sp::kMaxDim, "the most separators", "refusals");
  expect(sp::refusal(entry, 30000, 21841, 1, 8, 1 << 20) == "ndt2d_sparse_solve: 21841 separators, the dense matrix holds 21840", "too many separators",
         "refusals");
  expect(sp::refusal(entry, sp::kMaxNodes + 1, 0, 1, 8, 1 << 20).find("poses, the solver holds 1073741824") != std::string::npos, "too many poses",
         "refusals");
  if (failures != 0) return 1;
  std::printf("ok\n");
  return 0;
}
