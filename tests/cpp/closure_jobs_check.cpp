// The chunk plan of ndt2d_closure_refine (ndt_2d_amd/csrc/closure/ndt2d_closure_jobs.h), a program
// of its own over the plain-C++ header: built with the host compiler and the sanitizers, run
// directly (tests/test_closure_refine_host.py).  Prints OK, or FAILED lines.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "ndt2d_closure_jobs.h"

using ndt2d::ClosureJobChunk;
using ndt2d::plan_closure_jobs;

static int failures = 0;

#define CHECK(cond)                                                      \
  do                                                                     \
  {                                                                      \
    if (!(cond))                                                         \
    {                                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

// What every plan must hold: every job exactly once, on the slot of its own candidate; candidates
// ascending within a chunk and named by a job of it; the limits; jobs of a candidate in job order.
static void check_plan(const std::vector<ClosureJobChunk> & plan, const uint32_t * job_candidate, size_t n_jobs,
                       size_t n_candidates, size_t max_candidates, size_t max_jobs)
{
  std::vector<int> seen(n_jobs, 0);
  size_t last_candidate = 0;
  bool any = false;
  for (const ClosureJobChunk & c : plan)
  {
    CHECK(!c.jobs.empty() && !c.candidates.empty());
    CHECK(c.jobs.size() == c.job_slot.size());
    CHECK(c.candidates.size() <= max_candidates && c.jobs.size() <= max_jobs);
    CHECK(std::is_sorted(c.candidates.begin(), c.candidates.end()));
    CHECK(std::adjacent_find(c.candidates.begin(), c.candidates.end()) == c.candidates.end());
    // candidates are taken in ascending index over the whole plan (a split one repeats)
    if (any) CHECK(c.candidates.front() >= last_candidate);
    any = true;
    last_candidate = c.candidates.back();
    std::vector<int> used(c.candidates.size(), 0);
    for (size_t b = 0; b < c.jobs.size(); ++b)
    {
      const uint32_t k = c.jobs[b];
      CHECK(k < n_jobs);
      if (k >= n_jobs) continue;
      ++seen[k];
      CHECK(c.job_slot[b] < c.candidates.size());
      if (c.job_slot[b] >= c.candidates.size()) continue;
      const uint32_t want = job_candidate != nullptr ? job_candidate[k] : k;
      CHECK(c.candidates[c.job_slot[b]] == want && want < n_candidates);
      used[c.job_slot[b]] = 1;
      if (b > 0 && c.job_slot[b] == c.job_slot[b - 1]) CHECK(c.jobs[b] > c.jobs[b - 1]);
      if (b > 0) CHECK(c.job_slot[b] >= c.job_slot[b - 1]);
    }
    CHECK(std::all_of(used.begin(), used.end(), [](int u) { return u == 1; }));   // no candidate is built for nothing
  }
  CHECK(std::all_of(seen.begin(), seen.end(), [](int s) { return s == 1; }));
}

int main()
{
  // K = 1
  {
    const auto plan = plan_closure_jobs(nullptr, 1, 1, 16, 4096);
    check_plan(plan, nullptr, 1, 1, 16, 4096);
    CHECK(plan.size() == 1 && plan[0].candidates == std::vector<uint32_t>{0} && plan[0].jobs == std::vector<uint32_t>{0});
  }
  // no job_candidate: job k on candidate k, 17 through 16 slots
  {
    const auto plan = plan_closure_jobs(nullptr, 17, 17, 16, 4096);
    check_plan(plan, nullptr, 17, 17, 16, 4096);
    CHECK(plan.size() == 2 && plan[0].candidates.size() == 16 && plan[1].candidates == std::vector<uint32_t>{16});
  }
  // candidates no job names are skipped
  {
    const uint32_t jc[4] = {5, 2, 5, 7};
    const auto plan = plan_closure_jobs(jc, 4, 9, 16, 4096);
    check_plan(plan, jc, 4, 9, 16, 4096);
    CHECK(plan.size() == 1 && (plan[0].candidates == std::vector<uint32_t>{2, 5, 7}));
    CHECK((plan[0].jobs == std::vector<uint32_t>{1, 0, 2, 3}) && (plan[0].job_slot == std::vector<uint32_t>{0, 1, 1, 2}));
  }
  // a job list in scrambled order
  {
    const uint32_t jc[6] = {0, 0, 1, 2, 2, 1};
    const auto plan = plan_closure_jobs(jc, 6, 3, 16, 4096);
    check_plan(plan, jc, 6, 3, 16, 4096);
    CHECK(plan.size() == 1 && (plan[0].jobs == std::vector<uint32_t>{0, 1, 2, 5, 3, 4}));
    const uint32_t jd[7] = {6, 3, 0, 3, 6, 1, 0};
    const auto p2 = plan_closure_jobs(jd, 7, 7, 2, 4096);
    check_plan(p2, jd, 7, 7, 2, 4096);
    CHECK(p2.size() == 2 && (p2[0].candidates == std::vector<uint32_t>{0, 1}) && (p2[1].candidates == std::vector<uint32_t>{3, 6}));
  }
  // max_candidates 2 with 5 candidates: 2 + 2 + 1
  {
    const uint32_t jc[8] = {4, 3, 2, 1, 0, 0, 2, 4};
    const auto plan = plan_closure_jobs(jc, 8, 5, 2, 4096);
    check_plan(plan, jc, 8, 5, 2, 4096);
    CHECK(plan.size() == 3 && plan[0].candidates.size() == 2 && plan[1].candidates.size() == 2 && plan[2].candidates.size() == 1);
    CHECK((plan[2].jobs == std::vector<uint32_t>{0, 7}));
  }
  // one candidate with 4,097 jobs: chunks of its own, 4,096 + 1; the candidates round it keep theirs
  {
    std::vector<uint32_t> jc(4097 + 2, 1);
    jc[0] = 0;
    jc[4098] = 2;
    const auto plan = plan_closure_jobs(jc.data(), jc.size(), 3, 16, 4096);
    check_plan(plan, jc.data(), jc.size(), 3, 16, 4096);
    CHECK(plan.size() == 4);
    if (plan.size() == 4)
    {
      CHECK(plan[0].candidates == std::vector<uint32_t>{0} && plan[0].jobs.size() == 1);
      CHECK(plan[1].candidates == std::vector<uint32_t>{1} && plan[1].jobs.size() == 4096);
      CHECK(plan[2].candidates == std::vector<uint32_t>{1} && plan[2].jobs.size() == 1 && plan[2].jobs[0] == 4097);
      CHECK(plan[3].candidates == std::vector<uint32_t>{2} && plan[3].jobs == std::vector<uint32_t>{4098});
    }
    // alone
    std::vector<uint32_t> one(4097, 0);
    const auto p1 = plan_closure_jobs(one.data(), one.size(), 1, 16, 4096);
    check_plan(p1, one.data(), one.size(), 1, 16, 4096);
    CHECK(p1.size() == 2 && p1[0].jobs.size() == 4096 && p1[1].jobs.size() == 1);
  }
  // the job limit closes a chunk before the candidate limit does
  {
    std::vector<uint32_t> jc;
    for (uint32_t c = 0; c < 5; ++c) jc.insert(jc.end(), 3, c);
    const auto plan = plan_closure_jobs(jc.data(), jc.size(), 5, 16, 7);
    check_plan(plan, jc.data(), jc.size(), 5, 16, 7);
    CHECK(plan.size() == 3 && plan[0].jobs.size() == 6 && plan[1].jobs.size() == 6 && plan[2].jobs.size() == 3);
  }
  // a pseudo-random sweep: every plan returns each job exactly once
  {
    uint32_t state = 12345u;
    for (int round = 0; round < 200; ++round)
    {
      const auto next = [&]() { state = state * 1664525u + 1013904223u; return state >> 8; };
      const size_t n_candidates = 1 + next() % 12, n_jobs = next() % 40;
      const size_t max_candidates = 1 + next() % 5, max_jobs = 1 + next() % 9;
      std::vector<uint32_t> jc(n_jobs);
      for (uint32_t & c : jc) c = next() % n_candidates;
      const auto plan = plan_closure_jobs(jc.data(), n_jobs, n_candidates, max_candidates, max_jobs);
      check_plan(plan, jc.data(), n_jobs, n_candidates, max_candidates, max_jobs);
      if (n_jobs == 0) CHECK(plan.empty());
    }
  }
  std::printf(failures == 0 ? "OK\n" : "%d checks FAILED\n", failures);
  return failures == 0 ? 0 : 1;
}
