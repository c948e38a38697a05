// Newton NDT registration for many scans at once on libndt2d_hip.so: K (scan, pose) jobs refined
// against the NDT in place in one call (ndt2d_matcher_refine_scans, include/ndt2d_hip.h).
//
// Every search of the reference ends on the lattice (src/scan_matcher_ndt.cpp:103-143): with the
// declared defaults the correction matchScan returns is quantised to 5 mm / 2.5 mrad.  A node that
// wants the optimum under a lattice winner -- or under an odometry guess -- hands the scan and
// that pose to refine(): a damped Newton iteration on the scan's NDT score, the whole iteration of
// all jobs in one kernel launch.  addScan() / addJob() collect the jobs as TrackScansHip does,
// refine() makes the one call; the poses that come back are ABSOLUTE, not corrections.
//
// setNeighbourhood(9) scores a point against the 3 x 3 cells round it instead of the one it falls
// in: the objective is then smooth across the cell borders to two or three orders of magnitude,
// and the inverse of its Hessian is the covariance a constraint wants (RefinedScan::covariance,
// include/ndt2d_hip.h at ndt2d_refine_covariance).
//
// Plain arrays over the C-ABI, as the other mirrors in this directory: nothing of ROS or Eigen.
#ifndef NDT_2D_HIP__REFINE_HIP_HPP_
#define NDT_2D_HIP__REFINE_HIP_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "job_list.hpp"
#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// One job's answer.
struct RefinedScan
{
  std::size_t job;           // index into the jobs, in add order
  std::size_t scan;          // index into the scans
  double pose[3];            // the pose reached (absolute)
  double score;              // scorePoints at that pose
  double start_score;        // scorePoints at the job's own pose
  double gradient[3];        // of the score at the pose reached
  double hessian[9];         // row-major, of the score (the sum's Hessian / beams)
  std::size_t beams;         // the scan's beams in use: min(laser_max_beams, its points)
  double covariance[9];      // row-major inverse of hessian x beams (x, y, theta); valid if has_covariance
  bool has_covariance;       // false: that Hessian is not positive definite (or the job did not run)
  std::uint32_t evals;       // evaluations of the score and its derivatives
  std::uint32_t steps;       // accepted steps
  int status;                // NDT2D_REFINE_*
  bool converged() const { return status == NDT2D_REFINE_CONVERGED; }
};

// addScan() / addJob() / add(), clear(), jobs() and scans() are JobList's (job_list.hpp).
class RefineHip : public JobList, public MatcherCalls
{
public:
  explicit RefineHip(ndt2d_matcher * matcher) : MatcherCalls(matcher) {}

  // ndt2d_refine_run's rules; the defaults are the library's.
  void setRules(std::uint32_t max_evals, double tol_lin, double tol_ang)
  {
    max_evals_ = max_evals;
    tol_lin_ = tol_lin;
    tol_ang_ = tol_ang;
  }

  // Cells a point is scored against: 1 (its own, the default) or 9 (the 3 x 3 round it), from the
  // next refine() on.  laser_max_beams: the matcher's (initialize), which the covariance needs to
  // turn the score's Hessian back into the sum's.  false: refused (last_error()).
  bool setNeighbourhood(std::uint32_t cells) { return ok(ndt2d_matcher_set_refine_neighbourhood(m_, cells)); }
  std::uint32_t neighbourhood()
  {
    std::uint32_t cells = 0;
    return ok(ndt2d_matcher_refine_neighbourhood(m_, &cells)) ? cells : 0u;
  }
  void setLaserMaxBeams(std::size_t laser_max_beams) { laser_max_beams_ = laser_max_beams; }

  // One call for every job collected; refined_out in job order.  false when the device call fails
  // (last_error()).  The collected scans and jobs stay until clear().
  bool refine(std::vector<RefinedScan> & refined_out)
  {
    refined_out.clear();
    const std::size_t n_jobs = jobs();
    if (n_jobs == 0) return true;
    poses_.assign(3 * n_jobs, 0.0);
    scores_.assign(n_jobs, 0.0);
    start_scores_.assign(n_jobs, 0.0);
    gradients_.assign(3 * n_jobs, 0.0);
    hessians_.assign(9 * n_jobs, 0.0);
    status_.assign(n_jobs, NDT2D_REFINE_NO_OVERLAP);
    evals_.assign(2 * n_jobs, 0u);
    if (!ok(ndt2d_matcher_refine_scans(m_, jobs_.data(), job_scan_.data(), n_jobs, points_.data(), offsets_.data(), scans(),
                                       max_evals_, tol_lin_, tol_ang_, poses_.data(), scores_.data(), start_scores_.data(),
                                       gradients_.data(), hessians_.data(), status_.data(), evals_.data())))
    {
      return false;
    }
    refined_out.reserve(n_jobs);
    for (std::size_t k = 0; k < n_jobs; ++k)
    {
      RefinedScan r;
      r.job = k;
      r.scan = job_scan_[k];
      r.score = scores_[k];
      r.start_score = start_scores_[k];
      for (int d = 0; d < 3; ++d)
      {
        r.pose[d] = poses_[3 * k + d];
        r.gradient[d] = gradients_[3 * k + d];
      }
      for (int d = 0; d < 9; ++d) r.hessian[d] = hessians_[9 * k + d];
      r.evals = evals_[2 * k];
      r.steps = evals_[2 * k + 1];
      r.status = status_[k];
      r.beams = beams_in_use(points_of(r.scan), laser_max_beams_, false);
      double sum_hessian[6];
      const int upper[6] = {0, 1, 2, 4, 5, 8};   // xx, xy, xt, yy, yt, tt
      for (int d = 0; d < 6; ++d) sum_hessian[d] = r.hessian[upper[d]] * static_cast<double>(r.beams);
      for (int d = 0; d < 9; ++d) r.covariance[d] = 0.0;
      r.has_covariance = r.evals > 0 && ndt2d_refine_covariance(sum_hessian, r.covariance) == NDT2D_OK;
      refined_out.push_back(r);
    }
    return true;
  }

  // HIP events around the call's kernel launch and read-back (after the first refine()).
  bool lastMs(float * kernel_ms, float * fetch_ms)
  {
    ndt2d_refine * r = ndt2d_matcher_refine(m_);
    if (r == nullptr) return false;
    return ndt2d_refine_last_ms(r, kernel_ms, fetch_ms) == NDT2D_OK;
  }

private:
  std::uint32_t max_evals_ = 32;
  double tol_lin_ = 1.0e-6, tol_ang_ = 1.0e-6;
  std::size_t laser_max_beams_ = 100;   // the plugin's declared default
  std::vector<double> poses_, scores_, start_scores_, gradients_, hessians_;
  std::vector<std::int32_t> status_;
  std::vector<std::uint32_t> evals_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__REFINE_HIP_HPP_
