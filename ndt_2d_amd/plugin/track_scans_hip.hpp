// Localisation by scan matching for many scans at once on libndt2d_hip.so: K (scan, pose) jobs
// matched against the NDT in place in one call (ndt2d_matcher_match_scans, include/ndt2d_hip.h)
// instead of K matchScan() round trips.
//
// The reference's localisation branch (src/ndt_mapper.cpp:547-566) calls matchScan(scan,
// correction, covariance) on the global matcher and adds the correction to the scan's pose
// (:557-561).  A fleet server that localises many robots against one shared map, a node that
// replays a recorded bag against a loaded map, or a consistency pass that matches every scan of
// the graph against the global map after solver_->optimize (:680) runs that branch for many
// scans: add() collects the jobs, track() makes the one call.
//
// Plain arrays over the C-ABI, as the other mirrors in this directory: nothing of ROS or Eigen.
#ifndef NDT_2D_HIP__TRACK_SCANS_HIP_HPP_
#define NDT_2D_HIP__TRACK_SCANS_HIP_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "job_list.hpp"
#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// One job's answer.
struct TrackedScan
{
  std::size_t job;           // index into the jobs, in add order
  std::size_t scan;          // index into the scans
  double score;
  bool has_winner;           // a lattice candidate scored below 0 (else the correction is zero)
  double correction[3];      // matchScan's pose output (dx, dy, dth)
  double pose[3];            // job pose + correction, as src/ndt_mapper.cpp:557-561 adds it
  double covariance[9];      // row-major
};

// addScan() / addJob() / add(), clear(), jobs() and scans() are JobList's (job_list.hpp).
class TrackScansHip : public JobList, public MatcherCalls
{
public:
  explicit TrackScansHip(ndt2d_matcher * matcher) : MatcherCalls(matcher) {}

  // One batched match of every job collected; tracked_out in job order.  false when the device
  // call fails (last_error()).  The collected scans and jobs stay until clear().
  bool track(std::vector<TrackedScan> & tracked_out)
  {
    tracked_out.clear();
    const std::size_t n_jobs = jobs();
    if (n_jobs == 0) return true;
    corrections_.assign(3 * n_jobs, 0.0);
    covariances_.assign(9 * n_jobs, 0.0);
    scores_.assign(n_jobs, 0.0);
    best_.assign(n_jobs, NDT2D_NO_INDEX);
    if (!ok(ndt2d_matcher_match_scans(m_, jobs_.data(), job_scan_.data(), n_jobs, points_.data(), offsets_.data(), scans(),
                                      corrections_.data(), covariances_.data(), scores_.data(), best_.data(), nullptr, 0,
                                      nullptr)))
    {
      return false;
    }
    tracked_out.reserve(n_jobs);
    for (std::size_t k = 0; k < n_jobs; ++k)
    {
      TrackedScan r;
      r.job = k;
      r.scan = job_scan_[k];
      r.score = scores_[k];
      r.has_winner = best_[k] != NDT2D_NO_INDEX;
      for (int d = 0; d < 3; ++d)
      {
        r.correction[d] = corrections_[3 * k + d];
        r.pose[d] = r.correction[d] + jobs_[3 * k + d];   // correction.x += scan->getPose().x; ...
      }
      for (int d = 0; d < 9; ++d) r.covariance[d] = covariances_[9 * k + d];
      tracked_out.push_back(r);
    }
    return true;
  }

  // HIP events around the batched match's launches (after the first track()).
  bool lastMs(float * search_ms, float * reduce_ms)
  {
    ndt2d_scans * s = ndt2d_matcher_scans(m_);
    if (s == nullptr) return false;
    return ndt2d_scans_last_ms(s, search_ms, reduce_ms) == NDT2D_OK;
  }

private:
  std::vector<double> corrections_, covariances_, scores_;
  std::vector<uint64_t> best_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__TRACK_SCANS_HIP_HPP_
