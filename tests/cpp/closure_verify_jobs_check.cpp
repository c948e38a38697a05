// The chunk plan of ndt2d_closure_verify (ndt_2d_amd/csrc/closure/ndt2d_closure_jobs.h with the
// jobs' beams as weights), a program of its own over the plain-C++ header: built with the host
// compiler and the sanitizers, run directly (tests/test_closure_verify_host.py).  Prints OK, or
// FAILED lines.
#include <algorithm>
#include <cstdint>
#include <cstdio>
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

constexpr size_t kCap = size_t(1) << 24;   // per-beam results of one chunk

// What every plan must hold: every job exactly once, on the slot of its own candidate; candidates
// ascending within a chunk and over the plan, each named by a job of its chunk; the limits -- a
// chunk over the weight cap holds one job --; jobs of a candidate in job order.
static void check_plan(const std::vector<ClosureJobChunk> & plan, const uint32_t * job_candidate, const size_t * weight,
                       size_t n_jobs, size_t n_candidates, size_t max_candidates, size_t max_jobs, size_t max_weight)
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
    if (any) CHECK(c.candidates.front() >= last_candidate);
    any = true;
    last_candidate = c.candidates.back();
    std::vector<int> used(c.candidates.size(), 0);
    size_t w = 0;
    for (size_t b = 0; b < c.jobs.size(); ++b)
    {
      const uint32_t k = c.jobs[b];
      CHECK(k < n_jobs);
      if (k >= n_jobs) continue;
      ++seen[k];
      w += weight[k];
      CHECK(c.job_slot[b] < c.candidates.size());
      if (c.job_slot[b] >= c.candidates.size()) continue;
      const uint32_t want = job_candidate != nullptr ? job_candidate[k] : k;
      CHECK(c.candidates[c.job_slot[b]] == want && want < n_candidates);
      used[c.job_slot[b]] = 1;
      if (b > 0 && c.job_slot[b] == c.job_slot[b - 1]) CHECK(c.jobs[b] > c.jobs[b - 1]);
      if (b > 0) CHECK(c.job_slot[b] >= c.job_slot[b - 1]);
    }
    CHECK(w <= max_weight || c.jobs.size() == 1);
    CHECK(std::all_of(used.begin(), used.end(), [](int u) { return u == 1; }));   // no candidate is built for nothing
  }
  CHECK(std::all_of(seen.begin(), seen.end(), [](int s) { return s == 1; }));
}

static bool same_plan(const std::vector<ClosureJobChunk> & a, const std::vector<ClosureJobChunk> & b)
{
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
  {
    if (a[i].candidates != b[i].candidates || a[i].jobs != b[i].jobs || a[i].job_slot != b[i].job_slot) return false;
  }
  return true;
}

int main()
{
  // candidates in ascending order among those named, unnamed ones not built, records in job order
  // (a chunk says where each of its jobs' records goes: jobs[b])
  {
    const uint32_t jc[6] = {7, 2, 7, 5, 2, 5};
    const size_t w[6] = {100, 100, 100, 100, 100, 100};
    const auto plan = plan_closure_jobs(jc, 6, 9, 16, 4096, w, kCap);
    check_plan(plan, jc, w, 6, 9, 16, 4096, kCap);
    CHECK(plan.size() == 1 && (plan[0].candidates == std::vector<uint32_t>{2, 5, 7}));
    CHECK((plan[0].jobs == std::vector<uint32_t>{1, 4, 3, 5, 0, 2}) && (plan[0].job_slot == std::vector<uint32_t>{0, 0, 1, 1, 2, 2}));
  }
  // five candidates through two slots: 2 + 2 + 1
  {
    const uint32_t jc[8] = {4, 3, 2, 1, 0, 0, 2, 4};
    const size_t w[8] = {1, 63, 64, 65, 256, 257, 100, 720};
    const auto plan = plan_closure_jobs(jc, 8, 5, 2, 4096, w, kCap);
    check_plan(plan, jc, w, 8, 5, 2, 4096, kCap);
    CHECK(plan.size() == 3 && plan[0].candidates.size() == 2 && plan[1].candidates.size() == 2 && plan[2].candidates.size() == 1);
    CHECK((plan[2].jobs == std::vector<uint32_t>{0, 7}));
  }
  // the 2^24 beam cap: three candidates of 2^23 beams each -- two fit, the third opens a chunk
  {
    const uint32_t jc[3] = {0, 1, 2};
    const size_t w[3] = {kCap / 2, kCap / 2, kCap / 2};
    const auto plan = plan_closure_jobs(jc, 3, 3, 16, 4096, w, kCap);
    check_plan(plan, jc, w, 3, 3, 16, 4096, kCap);
    CHECK(plan.size() == 2 && (plan[0].candidates == std::vector<uint32_t>{0, 1}) && (plan[1].candidates == std::vector<uint32_t>{2}));
    // one beam more in the second: it no longer fits beside the first
    const size_t w2[3] = {kCap / 2, kCap / 2 + 1, kCap / 2 - 1};
    const auto p2 = plan_closure_jobs(jc, 3, 3, 16, 4096, w2, kCap);
    check_plan(p2, jc, w2, 3, 3, 16, 4096, kCap);
    CHECK(p2.size() == 2 && (p2[0].candidates == std::vector<uint32_t>{0}) && (p2[1].candidates == std::vector<uint32_t>{1, 2}));
  }
  // one candidate whose jobs weigh more than a chunk: chunks of its own, the candidates round it keep theirs
  {
    const uint32_t jc[6] = {0, 1, 1, 1, 1, 2};
    const size_t w[6] = {10, 1u << 20, kCap - (1u << 20), 1u << 20, 1u << 20, 10};
    const auto plan = plan_closure_jobs(jc, 6, 3, 16, 4096, w, kCap);
    check_plan(plan, jc, w, 6, 3, 16, 4096, kCap);
    CHECK(plan.size() == 4);
    if (plan.size() == 4)
    {
      CHECK(plan[0].candidates == std::vector<uint32_t>{0} && plan[0].jobs == std::vector<uint32_t>{0});
      CHECK(plan[1].candidates == std::vector<uint32_t>{1} && (plan[1].jobs == std::vector<uint32_t>{1, 2}));
      CHECK(plan[2].candidates == std::vector<uint32_t>{1} && (plan[2].jobs == std::vector<uint32_t>{3, 4}));
      CHECK(plan[3].candidates == std::vector<uint32_t>{2} && plan[3].jobs == std::vector<uint32_t>{5});
    }
  }
  // a job heavier than the cap is taken whole, alone
  {
    const uint32_t jc[3] = {0, 0, 1};
    const size_t w[3] = {5, 9, 3};
    const auto plan = plan_closure_jobs(jc, 3, 2, 16, 4096, w, 8);
    check_plan(plan, jc, w, 3, 2, 16, 4096, 8);
    CHECK(plan.size() == 3 && plan[1].jobs == std::vector<uint32_t>{1});
    const size_t heavy[1] = {100};
    const auto p1 = plan_closure_jobs(nullptr, 1, 1, 16, 4096, heavy, 8);
    check_plan(p1, nullptr, heavy, 1, 1, 16, 4096, 8);
    CHECK(p1.size() == 1);
  }
  // a candidate with more jobs than a launch: 4,096 + 1, as the refinement's plan
  {
    std::vector<uint32_t> jc(4097 + 2, 1);
    jc[0] = 0;
    jc[4098] = 2;
    std::vector<size_t> w(jc.size(), 100);
    const auto plan = plan_closure_jobs(jc.data(), jc.size(), 3, 16, 4096, w.data(), kCap);
    check_plan(plan, jc.data(), w.data(), jc.size(), 3, 16, 4096, kCap);
    CHECK(plan.size() == 4);
    if (plan.size() == 4)
    {
      CHECK(plan[1].candidates == std::vector<uint32_t>{1} && plan[1].jobs.size() == 4096);
      CHECK(plan[2].candidates == std::vector<uint32_t>{1} && plan[2].jobs.size() == 1 && plan[2].jobs[0] == 4097);
    }
    CHECK(same_plan(plan, plan_closure_jobs(jc.data(), jc.size(), 3, 16, 4096)));
  }
  // a pseudo-random sweep: every plan returns each job exactly once within the limits, and where the
  // weights never bind the plan is the refinement's -- which is what it is without weights at all
  {
    uint32_t state = 54321u;
    int bound = 0;
    for (int round = 0; round < 300; ++round)
    {
      const auto next = [&]() { state = state * 1664525u + 1013904223u; return state >> 8; };
      const size_t n_candidates = 1 + next() % 12, n_jobs = next() % 40;
      const size_t max_candidates = 1 + next() % 5, max_jobs = 1 + next() % 9, max_weight = 1 + next() % 60;
      std::vector<uint32_t> jc(n_jobs);
      std::vector<size_t> w(n_jobs);
      for (uint32_t & c : jc) c = next() % n_candidates;
      for (size_t & v : w) v = 1 + next() % 20;
      const auto plan = plan_closure_jobs(jc.data(), n_jobs, n_candidates, max_candidates, max_jobs, w.data(), max_weight);
      check_plan(plan, jc.data(), w.data(), n_jobs, n_candidates, max_candidates, max_jobs, max_weight);
      if (n_jobs == 0) CHECK(plan.empty());
      const auto plain = plan_closure_jobs(jc.data(), n_jobs, n_candidates, max_candidates, max_jobs);
      if (!same_plan(plan, plain)) ++bound;
      CHECK(same_plan(plain, plan_closure_jobs(jc.data(), n_jobs, n_candidates, max_candidates, max_jobs, nullptr, 0)));
      CHECK(same_plan(plain, plan_closure_jobs(jc.data(), n_jobs, n_candidates, max_candidates, max_jobs, w.data(), kCap)));
    }
    CHECK(bound > 50);   // (the weights did bind in many rounds)
  }
  std::printf(failures == 0 ? "OK\n" : "%d checks FAILED\n", failures);
  return failures == 0 ? 0 : 1;
}
