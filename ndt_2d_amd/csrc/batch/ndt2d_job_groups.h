// The jobs of one chunk of the batched scan tracking (scans/ndt2d_scans.hip) grouped by the number
// C of partial sums their scan's beam count asks for (ndt2d_sum_chunks.h): C is a
// template parameter of the lane's walk, so a chunk is searched with one launch per C present.
// A group keeps its jobs in the caller's order (a stable counting sort), groups follow each other
// by ascending C, and `position` maps a job back to its place in that launch order.  Records and
// scores are written by job, whatever the grouping.
// Plain C++: host code and a stand-alone check include it without the HIP headers.
#ifndef NDT2D_JOB_GROUPS_H_
#define NDT2D_JOB_GROUPS_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ndt2d_sum_chunks.h"

namespace ndt2d
{

struct JobGroups
{
  uint32_t n_groups = 0;                  // C values present
  uint32_t chunks[kMaxSumChunks] = {};    // the C of group g, ascending
  uint32_t first[kMaxSumChunks + 1] = {}; // order[first[g] .. first[g + 1]) are the jobs of group g
  std::vector<uint32_t> order;            // launch position -> job
  std::vector<uint32_t> position;         // job -> launch position (the inverse of order)
};

// job_beams[j]: the beam count of job j's scan.
inline void group_jobs(const uint32_t * job_beams, size_t n_jobs, JobGroups & out)
{
  size_t count[kMaxSumChunks + 1] = {};   // by C, 1 .. kMaxSumChunks
  for (size_t j = 0; j < n_jobs; ++j) ++count[sum_chunks(job_beams[j])];
  size_t start[kMaxSumChunks + 1] = {};
  out.n_groups = 0;
  size_t at = 0;
  for (uint32_t c = 1; c <= kMaxSumChunks; ++c)
  {
    start[c] = at;
    if (count[c] == 0) continue;
    out.chunks[out.n_groups] = c;
    out.first[out.n_groups] = static_cast<uint32_t>(at);
    ++out.n_groups;
    at += count[c];
  }
  out.first[out.n_groups] = static_cast<uint32_t>(at);
  out.order.resize(n_jobs);
  out.position.resize(n_jobs);
  for (size_t j = 0; j < n_jobs; ++j)
  {
    const size_t p = start[sum_chunks(job_beams[j])]++;
    out.order[p] = static_cast<uint32_t>(j);
    out.position[j] = static_cast<uint32_t>(p);
  }
}

}  // namespace ndt2d

#endif  // NDT2D_JOB_GROUPS_H_
