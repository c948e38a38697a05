// The chunk plan of ndt2d_closure_refine and what a slot takes of a launch's arrays
// (ndt_2d_amd/csrc/closure/ndt2d_closure_jobs.h), and the sent scans of a chunk with their copy into
// the stage (ndt_2d_amd/csrc/batch/ndt2d_refine_jobs.h): a program of its own over the plain-C++
// headers, built with the host compiler and the sanitizers, run directly
// (tests/test_closure_refine_host.py).  Prints OK, or FAILED lines.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "ndt2d_closure_jobs.h"
#include "ndt2d_refine_jobs.h"

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
  // what a slot takes of a launch's arrays: list entries max(1, min(n_points, ncell)), table
  // entries a multiple of 8 that hold the cells, "off the grid" and the pair store's padding;
  // slots placed one behind the other by the running sums do not overlap
  {
    const size_t cases[4][2] = {{0, 1}, {3, 65534}, {2048, 7}, {5, 6}};
    const size_t want_list[4] = {1, 3, 7, 5};
    size_t list_off = 0, lookup_off = 0;
    for (int i = 0; i < 4; ++i)
    {
      const size_t n_points = cases[i][0], ncell = cases[i][1];
      const ndt2d::SlotExtent e = ndt2d::slot_extent(n_points, ncell);
      CHECK(e.list == want_list[i] && e.list >= 1 && e.list >= std::min(n_points, ncell));
      CHECK(e.lookup % 8 == 0 && e.lookup >= ncell + 2 && e.lookup < ncell + 2 + 8);
      // the build clears (ncell + 2) / 2 pairs of entries from the slot's first: within the slot
      CHECK(2 * ((ncell + 2) / 2) <= e.lookup);
      // this slot is [off, off + extent); the next starts where it ends, on a multiple of 8
      const size_t list_end = list_off + e.list, lookup_end = lookup_off + e.lookup;
      CHECK(lookup_off % 8 == 0 && list_end > list_off && lookup_end >= lookup_off + ncell + 2);
      list_off = list_end;
      lookup_off = lookup_end;
    }
    CHECK(list_off == 1 + 3 + 7 + 5 && lookup_off == 8 + 65536 + 16 + 8);
  }
  // the sent scans of a chunk and their copy into the stage: each named scan once, in the order the
  // jobs first name them, its beams at its scan_first, nothing written beyond the chunk's beams
  {
    const size_t beam_offsets[5] = {0, 3, 3 + 1, 3 + 1 + 4, 3 + 1 + 4 + 2};   // scans of 3, 1, 4, 2 beams
    std::vector<double> beams(2 * 10);
    for (size_t i = 0; i < beams.size(); ++i) beams[i] = 100.0 + static_cast<double>(i);
    const uint32_t job_scan[5] = {2, 0, 2, 3, 0};   // scan 1 is not named
    const uint32_t chunk_jobs[4] = {4, 2, 3, 0};    // the chunk's jobs, as indices into the call's
    std::vector<uint64_t> scan_first;
    std::vector<uint32_t> sent;
    const size_t n_beams = ndt2d::refine_jobs::plan_sent_scans(
      4, [&](size_t b) { return static_cast<size_t>(chunk_jobs[b]); }, [&](size_t k) { return static_cast<size_t>(job_scan[k]); },
      beam_offsets, 4, scan_first, sent);
    CHECK(n_beams == 3 + 4 + 2 && (sent == std::vector<uint32_t>{0, 2, 3}));
    CHECK(scan_first.size() == 4 && scan_first[0] == 0 && scan_first[2] == 3 && scan_first[3] == 7);
    CHECK(scan_first[1] == ndt2d::refine_jobs::kNotSent);
    std::vector<double> stage(2 * n_beams, -1.0);   // (exactly the chunk's beams: a write beyond is the sanitizer's)
    ndt2d::refine_jobs::copy_sent_scans(sent, scan_first, beams.data(), beam_offsets, stage.data());
    for (const uint32_t sc : sent)
    {
      for (size_t i = 0; i < 2 * (beam_offsets[sc + 1] - beam_offsets[sc]); ++i)
      {
        CHECK(stage[2 * scan_first[sc] + i] == beams[2 * beam_offsets[sc] + i]);
      }
    }
    CHECK(std::none_of(stage.begin(), stage.end(), [](double v) { return v == -1.0; }));
    // no job: nothing is sent, nothing copied
    const size_t none = ndt2d::refine_jobs::plan_sent_scans(
      0, [&](size_t b) { return b; }, [&](size_t k) { return k; }, beam_offsets, 4, scan_first, sent);
    CHECK(none == 0 && sent.empty());
    ndt2d::refine_jobs::copy_sent_scans(sent, scan_first, beams.data(), beam_offsets, nullptr);
  }
  std::printf(failures == 0 ? "OK\n" : "%d checks FAILED\n", failures);
  return failures == 0 ? 0 : 1;
}
