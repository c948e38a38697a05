// csrc/sparsecov/ndt2d_sparsecov_plan.h in a program of its own: a job's doubles term by term, the
// chunking by the byte budget, the refusals' texts, and the lists the host derives from the layout and
// the asked pairs -- the blocks of S^-1 (the fixed ones, then the others in the order they are first
// asked for, none twice), the pairs' words (ascending nodes, the transposed flag, the four slots with
// their transposed bit, the pass), and the column passes (one per distinct column node, only for two
// interior nodes of one segment).  Prints "ok" and returns 0, or says what failed.
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "sparse/ndt2d_sparse_plan.h"
#include "sparsecov/ndt2d_sparsecov_plan.h"

namespace sp = ndt2d::sparse;
namespace sc = ndt2d::sparsecov;
namespace cov = ndt2d::covariance;

namespace
{

int failures = 0;

void expect(bool ok, const char * what)
{
  if (ok) return;
  std::printf("FAILED: %s\n", what);
  ++failures;
}

void doubles_and_chunks()
{
  expect(sc::kSelectDoubles == 24 && sc::kPairWords == 8, "24 doubles a node of G, 8 words a pair");
  expect(sc::inverse_doubles(0) == 0 && sc::inverse_doubles(1) == 48 * 48 && sc::inverse_doubles(16) == 48 * 48 && sc::inverse_doubles(17) == 96 * 96,
         "T is padded(3 s)^2");
  expect(sc::fixed_blocks(0) == 0 && sc::fixed_blocks(1) == 1 && sc::fixed_blocks(8) == 15, "2 s - 1 blocks are always there");
  for (size_t n : {2u, 33u, 1000u})
  {
    for (size_t s : {0u, 1u, 2u, 17u})
    {
      if (s > n) continue;
      for (size_t m : {0u, 40u})
      {
        for (int loss = 0; loss < 2; ++loss)
        {
          const size_t ld = cov::padded(3 * s), ni = n - s, blocks = sc::fixed_blocks(s) + 3, pairs = 5;
          const size_t want = 114 * ni + 2 * ld * ld + 2 * ld + 6 * s + 9 * blocks + 9 * pairs + 41 * n + (loss ? m : 0) + 17;
          expect(sc::job_doubles(n, s, m, loss != 0, blocks, pairs) == want, "a job's doubles, term by term");
          expect(sc::job_doubles(n, s, m, loss != 0, blocks, pairs) ==
                     sp::job_doubles(n, s, m, loss != 0) + sc::inverse_doubles(s) + 24 * ni + 9 * blocks + 9 * pairs,
                 "the sparse solve's job, T, the select region, the blocks and the pairs");
        }
      }
    }
  }
  expect(sc::chunk_jobs(8, 1000, 100) == 8 && sc::chunk_jobs(8, 799, 100) == 7 && sc::chunk_jobs(8, 99, 100) == 0 && sc::chunk_jobs(8, 100, 100) == 1,
         "the jobs of a chunk");
}

void refusals()
{
  const char * e = "entry";
  expect(sc::refusal(e, 100, 10, 30, 5, 4, 1000, 8000).empty(), "nothing to refuse");
  expect(sc::refusal(e, (size_t(1) << 30) + 1, 10, 30, 5, 4, 1000, 8000) == "entry: 1073741825 poses, the solver holds 1073741824", "too many poses");
  expect(sc::refusal(e, 100000, 21841, 30, 5, 4, 1000, 8000) == "entry: 21841 separators, the dense matrix holds 21840", "too many separators");
  expect(sc::refusal(e, 100, 10, size_t(1) << 31, 5, 4, 1000, 8000) == "entry: more than 2^31 - 1 blocks a job", "too many blocks");
  expect(sc::refusal(e, 100, 10, 30, size_t(1) << 31, 4, 1000, 8000) == "entry: more than 2^31 - 1 blocks a job", "too many pairs");
  expect(sc::refusal(e, 100, 10, 30, 5, 0, 9000, 8000) == "entry: a job of 100 poses and 10 separators needs 9000 bytes, the workspace is 8000",
         "a job that does not fit, with its bytes");
}

void lists()
{
  // 12 nodes, closures (2, 6) and (6, 9): the separators 2, 6, 9 (indices 0, 1, 2); the segments {0, 1}, {3, 4, 5}, {7, 8}, {10, 11}
  const uint32_t begin[13] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2, 6}, end[13] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 6, 9};
  sp::Layout layout;
  sp::make_layout(12, 13, begin, end, &layout);
  const sp::Tables t = layout.tables();
  expect(t.s == 3 && t.ni == 9, "three separators");
  uint32_t r[2];
  sc::reach(t, 6, r);
  expect(r[0] == 1 && r[1] == sc::kNone, "a separator reaches itself");
  sc::reach(t, 4, r);
  expect(r[0] == 0 && r[1] == 1, "an interior node its two separators");
  sc::reach(t, 0, r);
  expect(r[0] == sc::kNone && r[1] == 0, "the first segment has none before it");
  sc::reach(t, 11, r);
  expect(r[0] == 2 && r[1] == sc::kNone, "the last segment has none after it");
  sc::Lists none;
  sc::make_lists(t, nullptr, 0, &none);
  const std::vector<uint32_t> fixed = {0, 0, 1, 1, 2, 2, 0, 1, 1, 2};
  expect(none.blocks == fixed && none.n_pairs() == 0 && none.n_passes() == 0, "without pairs: the diagonal and the consecutive blocks");
  //                      same segment  reversed  a == b  separators far   interior x far segment  separator x interior  same column again
  const uint32_t asked[] = {3, 5,        5, 3,     4, 4,   9, 2,            0, 11,                  6, 8,                 4, 5,             7, 8};
  sc::Lists l;
  sc::make_lists(t, asked, 8, &l);
  expect(l.n_pairs() == 8 && l.pairs.size() == 64, "eight words a pair");
  const auto w = [&](size_t q, size_t k) { return l.pairs[q * sc::kPairWords + k]; };
  const uint32_t T = sc::kSlotTransposed, N = sc::kNone;
  // (3, 5): both reach {0, 1}: slots (0,0) = 0, (0,1) = s + 0 = 3, (1,0) = 3 | T, (1,1) = 1; pass 0 (column 5: interior index 4)
  expect(w(0, 0) == 3 && w(0, 1) == 5 && w(0, 2) == 0 && w(0, 3) == 3 && w(0, 4) == (3 | T) && w(0, 5) == 1 && w(0, 6) == 0 && w(0, 7) == 0, "(3, 5)");
  expect(w(1, 0) == 3 && w(1, 1) == 5 && w(1, 6) == 0 && w(1, 7) == sc::kFlagTransposed, "(5, 3) is (3, 5) transposed, in the same pass");
  for (size_t k = 2; k < 6; ++k) expect(w(1, k) == w(0, k), "(5, 3) has (3, 5)'s slots");
  expect(w(2, 0) == 4 && w(2, 1) == 4 && w(2, 6) == N && w(2, 7) == 0, "(4, 4) has no pass");
  // (9, 2) -> (2, 9) transposed: separators 0 and 2, the first block that is not fixed: place 5
  expect(w(3, 0) == 2 && w(3, 1) == 9 && w(3, 2) == 5 && w(3, 3) == N && w(3, 4) == N && w(3, 5) == N && w(3, 6) == N && w(3, 7) == 1, "(9, 2)");
  // (0, 11): reach {N, 0} x {2, N}: only (after a, before b) = (0, 2): place 5 again
  expect(w(4, 2) == N && w(4, 3) == N && w(4, 4) == 5 && w(4, 5) == N && w(4, 6) == N, "(0, 11): one block, no pass across segments");
  // (6, 8): separator 1 x {1, 2}: (1,1) = 1, (1,2) = s + 1 = 4
  expect(w(5, 2) == 1 && w(5, 3) == 4 && w(5, 4) == N && w(5, 5) == N && w(5, 6) == N, "(6, 8): a separator with an interior node");
  expect(w(6, 6) == 0, "(4, 5) shares (3, 5)'s pass: the same column node");
  expect(w(7, 6) == 1, "(7, 8) has a pass of its own");
  const std::vector<uint32_t> passes = {4, 6};   // the interior indices of nodes 5 and 8
  expect(l.passes == passes, "the passes' column nodes");
  std::vector<uint32_t> blocks = fixed;
  blocks.push_back(0);
  blocks.push_back(2);
  expect(l.blocks == blocks && l.n_blocks() == sc::fixed_blocks(3) + 1, "one more block, asked for twice, listed once");
  std::set<std::pair<uint32_t, uint32_t>> seen;
  for (size_t e = 0; e < l.n_blocks(); ++e)
  {
    expect(l.blocks[2 * e] <= l.blocks[2 * e + 1] && l.blocks[2 * e + 1] < t.s, "a block is (x, y), x <= y < s");
    expect(seen.insert({l.blocks[2 * e], l.blocks[2 * e + 1]}).second, "no block twice");
  }
  for (size_t q = 0; q < l.n_pairs(); ++q)
  {
    for (size_t k = 2; k < 6; ++k) expect(w(q, k) == N || (w(q, k) & ~T) < l.n_blocks(), "a slot lies in the table");
    expect(w(q, 6) == N || w(q, 6) < l.n_passes(), "a pass lies in the list");
  }
  // a pair's words but for the places do not depend on the other pairs
  const uint32_t alone[] = {0, 11};
  sc::Lists one;
  sc::make_lists(t, alone, 1, &one);
  expect(one.pairs[4] == 5 && one.blocks.size() == 12 && one.blocks[10] == 0 && one.blocks[11] == 2, "(0, 11) alone asks for its block itself");
  expect(sc::list_words(l.n_blocks(), l.n_pairs(), l.n_passes()) == l.blocks.size() + l.pairs.size() + l.passes.size(), "the words of the lists");
  // no separator at all
  const uint32_t b2[3] = {0, 1, 2}, e2[3] = {1, 2, 3};
  sp::make_layout(4, 3, b2, e2, &layout);
  const uint32_t asked2[] = {1, 3, 2, 2};
  sc::make_lists(layout.tables(), asked2, 2, &l);
  expect(l.n_blocks() == 0 && l.n_passes() == 1 && l.passes[0] == 3 && l.pairs[6] == 0 && l.pairs[8 + 6] == N, "s = 0: one segment, a pass for (1, 3)");
  for (size_t k = 2; k < 6; ++k) expect(l.pairs[k] == N, "s = 0: no slot");
}

}  // namespace

int main()
{
  doubles_and_chunks();
  refusals();
  lists();
  if (failures != 0) return 1;
  std::printf("ok\n");
  return 0;
}
