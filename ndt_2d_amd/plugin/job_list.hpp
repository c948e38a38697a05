// What the matcher mirrors of this directory share: the (scan, pose) job list that track(),
// refine() and verify() hand to the library -- K jobs over S scans, each scan's points once however
// many jobs name it --, how many beams of a scan are in use, and the matcher with its last error.
//
// Plain arrays over the C-ABI, as the mirrors themselves: nothing of ROS or Eigen.
#ifndef NDT_2D_HIP__JOB_LIST_HPP_
#define NDT_2D_HIP__JOB_LIST_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// Beams of a scan in use: min(max_beams, its points) by matchScan's subsampling.  zero_means_all:
// max_beams 0 takes every point (otherwise it takes none).
inline std::size_t beams_in_use(std::size_t points, std::size_t max_beams, bool zero_means_all)
{
  if (max_beams == 0 && zero_means_all) return points;
  return points < max_beams ? points : max_beams;
}

// The jobs and scans collected for one call, as the ndt2d_matcher_*_scans entry points take them.
class JobList
{
public:
  JobList() { clear(); }

  // Forget the scans and jobs collected so far.
  void clear()
  {
    points_.clear();
    offsets_.assign(1, 0);
    jobs_.clear();
    job_scan_.clear();
  }

  // A scan's robot-frame points; returns its index.
  std::size_t addScan(const double * points_xy, std::size_t n_points)
  {
    points_.insert(points_.end(), points_xy, points_xy + 2 * n_points);
    offsets_.push_back(points_.size() / 2);
    return offsets_.size() - 2;
  }

  // A job: scan `scan` at (or from) pose_xyt.  Several jobs may name one scan: its points travel
  // once.  Returns the job's index.
  std::size_t addJob(std::size_t scan, const double * pose_xyt)
  {
    jobs_.insert(jobs_.end(), pose_xyt, pose_xyt + 3);
    job_scan_.push_back(static_cast<std::uint32_t>(scan));
    return job_scan_.size() - 1;
  }

  // A scan and the one job on it.
  std::size_t add(const double * pose_xyt, const double * points_xy, std::size_t n_points)
  {
    return addJob(addScan(points_xy, n_points), pose_xyt);
  }

  std::size_t jobs() const { return job_scan_.size(); }
  std::size_t scans() const { return offsets_.size() - 1; }
  std::size_t points_of(std::size_t scan) const { return offsets_[scan + 1] - offsets_[scan]; }

protected:
  std::vector<double> points_, jobs_;
  std::vector<std::size_t> offsets_;
  std::vector<std::uint32_t> job_scan_;
};

// The matcher a mirror calls and the text of its last refused call.
class MatcherCalls
{
public:
  explicit MatcherCalls(ndt2d_matcher * matcher) : m_(matcher) {}

  const std::string & last_error() const { return error_; }

protected:
  bool ok(int rc)
  {
    if (rc == NDT2D_OK) return true;
    error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_matcher_last_error(m_);
    return false;
  }

  ndt2d_matcher * m_;

private:
  std::string error_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__JOB_LIST_HPP_
