// The chunk plan of ndt2d_closure_refine and ndt2d_closure_verify (closure/ndt2d_closure.hip): which
// candidate maps a launch builds and which jobs run on them -- and what a slot takes of a launch's
// arrays (slot_extent: every entry point's slot offsets are its running sums).  Plain C++ -- no HIP
// -- so that a host program can check it (tests/cpp/closure_jobs_check.cpp).
//
// Candidates are taken in ascending index among those a job names (a candidate no job names is
// not built); a candidate's jobs in ascending job index.  A chunk closes before it would exceed
// max_candidates candidates or max_jobs jobs -- the blocks of a launch.  A candidate with more
// jobs than one launch holds continues in chunks of its own (it is built once per such chunk).
// Every job is in exactly one chunk; a chunk names where each of its jobs' records goes, so the
// results land in job order whatever the plan.
//
// The verification's jobs carry a weight, their beams: a chunk also closes before its jobs' weights
// would pass max_weight (a job heavier than that is taken alone, whole), and a candidate whose jobs
// weigh more than one chunk continues in chunks of its own like one with too many jobs.  Without
// weights -- the refinement -- the plan is what it was.
#ifndef NDT2D_CLOSURE_JOBS_H_
#define NDT2D_CLOSURE_JOBS_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ndt2d
{

// What one slot -- a candidate map of n_points points on ncell cells -- takes of a launch's arrays:
// touched-cell records (at least one, so that no slot is empty) and uint16 table entries (the
// cells, "off the grid" and padding to a multiple of 8, so that every slot's table starts on 16
// bytes).  The slots' offsets are the running sums of these, nothing else.
struct SlotExtent
{
  size_t list, lookup;
};

inline SlotExtent slot_extent(size_t n_points, size_t ncell)
{
  return SlotExtent{std::max<size_t>(1, std::min(n_points, ncell)), (ncell + 2 + 7) & ~size_t(7)};
}

struct ClosureJobChunk
{
  std::vector<uint32_t> candidates;   // ascending: slot s of the launch is candidate candidates[s]
  std::vector<uint32_t> jobs;         // block b of the launch is job jobs[b] of the call
  std::vector<uint32_t> job_slot;     // ... on slot job_slot[b]
};

// job_candidate: n_jobs entries, each < n_candidates (the caller has checked), or NULL: job k uses
// candidate k (n_jobs == n_candidates).  max_candidates, max_jobs >= 1.  job_weight: n_jobs entries
// with max_weight, or NULL: no job weighs anything.
inline std::vector<ClosureJobChunk> plan_closure_jobs(const uint32_t * job_candidate, size_t n_jobs, size_t n_candidates,
                                                      size_t max_candidates, size_t max_jobs,
                                                      const size_t * job_weight = nullptr, size_t max_weight = 0)
{
  const auto weight_of = [&](size_t k) { return job_weight != nullptr ? job_weight[k] : size_t(0); };
  // the jobs of every candidate, in job order (a counting sort: stable)
  std::vector<size_t> first(n_candidates + 1, 0);
  for (size_t k = 0; k < n_jobs; ++k) ++first[(job_candidate != nullptr ? job_candidate[k] : k) + 1];
  for (size_t c = 0; c < n_candidates; ++c) first[c + 1] += first[c];
  std::vector<uint32_t> by_candidate(n_jobs);
  {
    std::vector<size_t> at(first.begin(), first.end() - 1);
    for (size_t k = 0; k < n_jobs; ++k) by_candidate[at[job_candidate != nullptr ? job_candidate[k] : k]++] = static_cast<uint32_t>(k);
  }

  std::vector<ClosureJobChunk> plan;
  ClosureJobChunk cur;
  size_t cur_weight = 0;
  const auto close = [&]() {
    if (!cur.jobs.empty()) plan.push_back(std::move(cur));
    cur = ClosureJobChunk{};
    cur_weight = 0;
  };
  const auto take = [&](size_t c, size_t j0, size_t j1) {
    const uint32_t slot = static_cast<uint32_t>(cur.candidates.size());
    cur.candidates.push_back(static_cast<uint32_t>(c));
    for (size_t j = j0; j < j1; ++j)
    {
      cur.jobs.push_back(by_candidate[j]);
      cur.job_slot.push_back(slot);
      cur_weight += weight_of(by_candidate[j]);
    }
  };
  for (size_t c = 0; c < n_candidates; ++c)
  {
    const size_t j0 = first[c], j1 = first[c + 1];
    if (j1 == j0) continue;   // no job names it
    size_t weight = 0;
    for (size_t j = j0; j < j1; ++j) weight += weight_of(by_candidate[j]);
    if (j1 - j0 > max_jobs || (weight > max_weight && j1 - j0 > 1))
    {
      // more jobs, or more weight, than a launch holds: chunks of its own
      close();
      for (size_t j = j0; j < j1;)
      {
        size_t e = j + 1, w = weight_of(by_candidate[j]);
        while (e < j1 && e - j < max_jobs && w + weight_of(by_candidate[e]) <= max_weight) w += weight_of(by_candidate[e++]);
        take(c, j, e);
        close();
        j = e;
      }
      continue;
    }
    if (cur.candidates.size() == max_candidates || cur.jobs.size() + (j1 - j0) > max_jobs ||
        (!cur.jobs.empty() && cur_weight + weight > max_weight))
    {
      close();
    }
    take(c, j0, j1);
  }
  close();
  return plan;
}

}  // namespace ndt2d

#endif  // NDT2D_CLOSURE_JOBS_H_
