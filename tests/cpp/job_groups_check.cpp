// Host-only check of the grouping of a chunk's jobs by their number of partial sums
// (ndt_2d_amd/csrc/batch/ndt2d_job_groups.h): the group table, the stable order within a group,
// the table that maps a job back to its launch position, and the C of the beam counts the tests
// use, worked out by hand and cross-checked against sum_chunks.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ndt2d_job_groups.h"

static int bad = 0;

static void expect(bool ok, const char * what)
{
  if (!ok)
  {
    std::printf("FAILED: %s\n", what);
    ++bad;
  }
}

// What holds for every grouping: order and position are permutations and each other's inverse,
// groups are contiguous, ascending in C, every job sits in the group of its C, and a group keeps
// its jobs in the caller's order.
static void check_invariants(const std::vector<uint32_t> & beams, const ndt2d::JobGroups & g)
{
  const size_t n = beams.size();
  expect(g.order.size() == n && g.position.size() == n, "table sizes");
  expect(g.n_groups <= ndt2d::kMaxSumChunks, "at most eight groups");
  expect(g.first[0] == 0 && g.first[g.n_groups] == n, "groups cover the jobs");
  std::vector<int> seen(n, 0);
  for (size_t p = 0; p < n; ++p)
  {
    expect(g.order[p] < n, "order in range");
    if (g.order[p] < n)
    {
      ++seen[g.order[p]];
      expect(g.position[g.order[p]] == p, "position inverts order");
    }
  }
  for (size_t j = 0; j < n; ++j) expect(seen[j] == 1, "order is a permutation");
  for (uint32_t k = 0; k < g.n_groups; ++k)
  {
    expect(g.first[k] < g.first[k + 1], "no empty group");
    if (k > 0) expect(g.chunks[k - 1] < g.chunks[k], "groups ascend in C");
    expect(g.chunks[k] >= 1 && g.chunks[k] <= ndt2d::kMaxSumChunks, "C in 1 .. 8");
    for (uint32_t p = g.first[k]; p < g.first[k + 1]; ++p)
    {
      expect(ndt2d::sum_chunks(beams[g.order[p]]) == g.chunks[k], "a job sits in the group of its C");
      if (p > g.first[k]) expect(g.order[p - 1] < g.order[p], "caller's order within a group");
    }
  }
}

int main()
{
  ndt2d::JobGroups g;
  // the beam counts of the tests and their C by hand: groups of four beams, chunks of five groups
  const uint32_t cases[10][2] = {{1, 1}, {20, 1}, {21, 2}, {60, 3}, {80, 4}, {100, 5}, {120, 6}, {140, 7}, {160, 8}, {720, 8}};
  for (const auto & c : cases)
  {
    const uint32_t got = ndt2d::sum_chunks(c[0]);
    std::printf("beams %u: C %u (expected %u)\n", c[0], got, c[1]);
    expect(got == c[1], "C of a beam count");
    ndt2d::group_jobs(&c[0], 1, g);
    expect(g.n_groups == 1 && g.chunks[0] == c[1] && g.order[0] == 0 && g.position[0] == 0, "a single job");
  }

  // 0 jobs
  ndt2d::group_jobs(nullptr, 0, g);
  expect(g.n_groups == 0 && g.first[0] == 0 && g.order.empty() && g.position.empty(), "0 jobs");
  check_invariants({}, g);

  // one group: the identity
  {
    const std::vector<uint32_t> beams = {100, 97, 100, 98, 99};   // 25 groups of four each: C = 5
    ndt2d::group_jobs(beams.data(), beams.size(), g);
    expect(g.n_groups == 1 && g.chunks[0] == 5 && g.first[1] == 5, "one group");
    for (uint32_t j = 0; j < 5; ++j) expect(g.order[j] == j && g.position[j] == j, "one group: the identity");
    check_invariants(beams, g);
  }

  // all eight C values present, interleaved, several jobs each
  {
    const std::vector<uint32_t> beams = {720, 1, 140, 21, 160, 60, 120, 80, 100, 20, 100, 80, 120, 60, 160, 21, 140, 1};
    ndt2d::group_jobs(beams.data(), beams.size(), g);
    expect(g.n_groups == 8, "eight groups");
    for (uint32_t k = 0; k < 8 && k < g.n_groups; ++k) expect(g.chunks[k] == k + 1, "C = 1 .. 8 in order");
    // C = 1: jobs 1, 9, 17 (1, 20 and 1 beams); C = 8: jobs 0, 4, 14 (720, 160, 160)
    expect(g.first[1] == 3 && g.order[0] == 1 && g.order[1] == 9 && g.order[2] == 17, "group C = 1, caller's order");
    expect(g.first[8] - g.first[7] == 3 && g.order[15] == 0 && g.order[16] == 4 && g.order[17] == 14, "group C = 8, caller's order");
    expect(g.position[0] == 15 && g.position[1] == 0, "job -> launch position");
    check_invariants(beams, g);
    // the object is reused: a smaller call after a larger one
    const std::vector<uint32_t> two = {720, 5};
    ndt2d::group_jobs(two.data(), two.size(), g);
    expect(g.n_groups == 2 && g.chunks[0] == 1 && g.chunks[1] == 8 && g.order[0] == 1 && g.order[1] == 0, "reuse");
    check_invariants(two, g);
  }

  // every beam count up to 4,096 as one call: the invariants, and 1,024 jobs of one count
  {
    std::vector<uint32_t> beams;
    for (uint32_t n = 1; n <= 4096; ++n) beams.push_back((n * 2654435761u) % 800u + 1u);
    ndt2d::group_jobs(beams.data(), beams.size(), g);
    check_invariants(beams, g);
    const std::vector<uint32_t> same(1024, 100);
    ndt2d::group_jobs(same.data(), same.size(), g);
    expect(g.n_groups == 1 && g.first[1] == 1024, "1,024 jobs of one count");
    check_invariants(same, g);
  }
  std::printf(bad == 0 ? "OK\n" : "FAILED\n");
  return bad == 0 ? 0 : 1;
}
