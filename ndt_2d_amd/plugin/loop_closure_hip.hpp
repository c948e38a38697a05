// The loop-closure thread's inner loop (reference src/ndt_mapper.cpp:619-671) on the batched
// match of libndt2d_hip.so: all candidate maps of a new scan in one call
// (ndt2d_matcher_match_candidates, include/ndt2d_hip.h) instead of reset() / addScans() /
// matchScan() per candidate.
//
// The node stores every scan on the matcher as it appends it to the graph (storeScan: the id is
// the scan's index in graph_->scans) and then, per new scan, hands closeLoops() the candidates
// findNearest returned.  The walk is the reference's: candidates in order, a candidate whose
// scan is empty is skipped and does not count, every other one counts against
// global_search_limit_, accepted when isfinite(score) && score < typical_matcher_response_.
// An accept corrects the scan's pose, which every later candidate starts from: the remaining
// candidates are matched again, in one batch, from the corrected pose.
//
// setRefine() adds the Newton registration on each candidate's OWN map: every round's match is
// followed by one ndt2d_matcher_refine_candidates call for the candidates of the round that pass
// the accept test, each started from the scan's pose + its correction.  The accept test stays the
// reference's, on the lattice score; the accepted closure gains the refined pose and the
// covariance from the Hessian there -- what the constraint of :658 wants -- and the scan goes on
// from the refined pose where the iteration converged (or ran out of evaluations) without raising f.
//
// setVerify() adds the match verification on each candidate's OWN map: every round makes one
// ndt2d_matcher_verify_candidates call for the candidates that pass the accept test, each at the
// pose the walk would adopt for it (the refined pose where it is usable, the lattice pose
// otherwise); the accepted closure gains the counts.  A verdict, no policy: the walk, the closures
// and the scan's pose are what they are without it.
//
// Plain arrays over the C-ABI, as the other mirrors in this directory: nothing of ROS or Eigen.
#ifndef NDT_2D_HIP__LOOP_CLOSURE_HIP_HPP_
#define NDT_2D_HIP__LOOP_CLOSURE_HIP_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "job_list.hpp"
#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// One accepted loop closure: what makeConstraint(candidate, scan, covariance) is given (:658).
struct LoopClosure
{
  std::size_t candidate;     // index of the candidate scan in the graph
  double score;
  double correction[3];      // matchScan's pose output (dx, dy, dth)
  double pose[3];            // the scan's pose after the correction (:652-655)
  double covariance[9];      // row-major
  // with setRefine(): the Newton registration on the candidate's own map, from `pose`
  bool refined = false;
  double refined_pose[3] = {0.0, 0.0, 0.0};   // absolute
  double refined_covariance[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // row-major; valid with has_refined_covariance
  bool has_refined_covariance = false;        // the Hessian at refined_pose is positive definite
  int refine_status = NDT2D_REFINE_NO_OVERLAP;   // NDT2D_REFINE_*
  // with setVerify(): the match verification on the candidate's own map, at verified_pose
  bool verified = false;
  double verified_pose[3] = {0.0, 0.0, 0.0};   // absolute: the pose the walk adopted
  // {n_beams, n_off, n_unseen, n_outlier, n_inlier, n_pierced, n_walked, 0}
  std::uint32_t verify[NDT2D_VERIFY_RECORD_U32] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
};

class LoopClosureHip : public MatcherCalls
{
public:
  explicit LoopClosureHip(ndt2d_matcher * matcher) : MatcherCalls(matcher) {}

  // A scan appended to the graph: its points go to the device once.  Returns false on failure.
  // The id the matcher hands out is the scan's index as long as every graph scan is stored in order.
  bool storeScan(const double * points_xy, std::size_t n_points, std::size_t * id_out = nullptr)
  {
    std::size_t id = 0;
    if (!ok(ndt2d_matcher_store_scan(m_, points_xy, n_points, &id))) return false;
    if (id >= sizes_.size()) sizes_.resize(id + 1, 0);
    sizes_[id] = n_points;
    if (id_out != nullptr) *id_out = id;
    return true;
  }

  // From the next closeLoops() on, refine the accepted candidates (see above).  max_evals, tol_lin,
  // tol_ang: ndt2d_refine_run's rules; cells: 1 or 9 cells per point (9 for a covariance);
  // laser_max_beams: the matcher's (initialize), which the covariance needs to turn the score's
  // Hessian back into the sum's.  false: the neighbourhood is refused (last_error()).
  bool setRefine(std::uint32_t max_evals, double tol_lin, double tol_ang, std::uint32_t cells, std::size_t laser_max_beams)
  {
    if (!ok(ndt2d_matcher_set_refine_neighbourhood(m_, cells))) return false;
    refine_ = true;
    max_evals_ = max_evals;
    tol_lin_ = tol_lin;
    tol_ang_ = tol_ang;
    laser_max_beams_ = laser_max_beams;
    return true;
  }
  void clearRefine() { refine_ = false; }

  // From the next closeLoops() on, verify the accepted candidates (see above).  max_beams: 0 takes
  // every point of the scan, otherwise the subsampling rule of matchScan (the matcher's
  // laser_max_beams: the beams the score was computed from); cells: 1 or 9; the gates and the ray
  // walk: ndt2d_verify's rules.  They are the matcher's verify parameters: verify_scans calls on the
  // same matcher take them too.  false: a parameter is refused (last_error()).
  bool setVerify(std::size_t max_beams, std::uint32_t cells, double gate_inlier, double gate_pierce, bool rays)
  {
    if (!ok(ndt2d_matcher_set_verify_neighbourhood(m_, cells))) return false;
    if (!ok(ndt2d_matcher_set_verify_gates(m_, gate_inlier, gate_pierce))) return false;
    if (!ok(ndt2d_matcher_set_verify_rays(m_, rays ? 1 : 0))) return false;
    verify_ = true;
    verify_max_beams_ = max_beams;
    return true;
  }
  void clearVerify() { verify_ = false; }

  // [begin_idx, end_idx) of src/ndt_mapper.cpp:628-631, quirk included: the candidate
  // i == rolling yields only scan i - 1.
  static void window(std::size_t i, std::size_t rolling, std::size_t * begin_idx, std::size_t * end_idx)
  {
    *begin_idx = (i > 0) ? i - 1 : i;
    *end_idx = (i < rolling) ? i + 1 : i;
  }

  // The walk of :619-671 for one new scan.  scan_pose_inout[3]: scan->getPose() / setPose();
  // candidates: findNearest's result; graph_poses_xyt[3 i ..]: the pose of graph scan i;
  // limit: global_search_limit_ (0: the reference's unsigned counter never reaches zero -- all).
  // Appends to closures_out; false when a device call fails (last_error()).
  bool closeLoops(double * scan_pose_inout, const double * points_xy, std::size_t n_points,
                  const std::vector<std::size_t> & candidates, const double * graph_poses_xyt,
                  std::size_t rolling, double typical_response, std::size_t limit,
                  std::vector<LoopClosure> & closures_out)
  {
    std::vector<std::size_t> todo;
    for (std::size_t i : candidates)
    {
      if (i < sizes_.size() && sizes_[i] == 0) continue;   // `if (candidate->getPoints().empty()) continue;`
      todo.push_back(i);
      if (limit != 0 && todo.size() == limit) break;      // `if (--num_scans_to_check == 0) break;`
    }
    while (!todo.empty())
    {
      offsets_.assign(1, 0);
      ids_.clear();
      poses_.clear();
      for (std::size_t i : todo)
      {
        std::size_t b = 0, e = 0;
        window(i, rolling, &b, &e);
        for (std::size_t j = b; j < e; ++j)
        {
          ids_.push_back(j);
          poses_.insert(poses_.end(), graph_poses_xyt + 3 * j, graph_poses_xyt + 3 * j + 3);
        }
        offsets_.push_back(ids_.size());
      }
      const std::size_t K = todo.size();
      corrections_.assign(3 * K, 0.0);
      covariances_.assign(9 * K, 0.0);
      scores_.assign(K, 0.0);
      if (!ok(ndt2d_matcher_match_candidates(m_, scan_pose_inout, points_xy, n_points, offsets_.data(), ids_.data(),
                                             poses_.data(), K, corrections_.data(), covariances_.data(),
                                             scores_.data(), nullptr, nullptr, 0, nullptr)))
      {
        return false;
      }
      std::size_t accepted = K;
      passing_.clear();
      for (std::size_t k = 0; k < K; ++k)
      {
        if (std::isfinite(scores_[k]) && scores_[k] < typical_response)
        {
          if (accepted == K) accepted = k;
          passing_.push_back(static_cast<std::uint32_t>(k));
        }
      }
      if (accepted == K) break;
      if (refine_ && !refineRound(scan_pose_inout, points_xy, n_points, K)) return false;
      if (verify_ && !verifyRound(scan_pose_inout, points_xy, n_points, K)) return false;
      LoopClosure c;
      c.candidate = todo[accepted];
      c.score = scores_[accepted];
      for (int d = 0; d < 3; ++d)
      {
        c.correction[d] = corrections_[3 * accepted + d];
        // correction.x += scan->getPose().x; ... scan->setPose(correction);
        scan_pose_inout[d] = c.correction[d] + scan_pose_inout[d];
        c.pose[d] = scan_pose_inout[d];
      }
      for (int d = 0; d < 9; ++d) c.covariance[d] = covariances_[9 * accepted + d];
      if (refine_)
      {
        // (job 0 of the round's refinement is the first candidate that passed: the accepted one)
        c.refined = true;
        c.refine_status = r_status_[0];
        for (int d = 0; d < 3; ++d) c.refined_pose[d] = r_poses_[d];
        const double n = static_cast<double>(beams_in_use(n_points, laser_max_beams_, false));
        const double * h = r_hessians_.data();
        const double sum_hessian[6] = {h[0] * n, h[1] * n, h[2] * n, h[4] * n, h[5] * n, h[8] * n};
        c.has_refined_covariance = r_evals_[0] > 0 && ndt2d_refine_covariance(sum_hessian, c.refined_covariance) == NDT2D_OK;
        if (refineUsable(0))
        {
          for (int d = 0; d < 3; ++d) scan_pose_inout[d] = c.refined_pose[d];
        }
      }
      if (verify_)
      {
        // (job 0 of the round's verification, likewise)
        c.verified = true;
        for (int d = 0; d < 3; ++d) c.verified_pose[d] = v_jobs_[d];
        for (int d = 0; d < NDT2D_VERIFY_RECORD_U32; ++d) c.verify[d] = v_records_[static_cast<std::size_t>(d)];
      }
      closures_out.push_back(c);
      todo.erase(todo.begin(), todo.begin() + static_cast<std::ptrdiff_t>(accepted) + 1);
    }
    return true;
  }

  // Forget every stored scan (the graph was reloaded): ids start from 0 again.
  bool dropScans()
  {
    sizes_.clear();
    return ok(ndt2d_matcher_drop_scans(m_));
  }

private:
  // One ndt2d_matcher_refine_candidates call for the candidates of the round that passed
  // (passing_), each from the scan's pose + its correction, all on the one scan.
  bool refineRound(const double * scan_pose, const double * points_xy, std::size_t n_points, std::size_t K)
  {
    const std::size_t n_jobs = passing_.size();
    r_jobs_.resize(3 * n_jobs);
    for (std::size_t j = 0; j < n_jobs; ++j)
    {
      for (int d = 0; d < 3; ++d) r_jobs_[3 * j + d] = corrections_[3 * passing_[j] + d] + scan_pose[d];
    }
    r_scan_.assign(n_jobs, 0u);
    r_poses_.assign(3 * n_jobs, 0.0);
    r_scores_.assign(n_jobs, 0.0);
    r_start_scores_.assign(n_jobs, 0.0);
    r_hessians_.assign(9 * n_jobs, 0.0);
    r_status_.assign(n_jobs, 0);
    r_evals_.assign(2 * n_jobs, 0u);
    const std::size_t point_offsets[2] = {0, n_points};
    return ok(ndt2d_matcher_refine_candidates(m_, offsets_.data(), ids_.data(), poses_.data(), K, r_jobs_.data(), r_scan_.data(),
                                              passing_.data(), n_jobs, points_xy, point_offsets, 1, max_evals_, tol_lin_,
                                              tol_ang_, r_poses_.data(), r_scores_.data(), r_start_scores_.data(), nullptr,
                                              r_hessians_.data(), r_status_.data(), r_evals_.data()));
  }

  // The walk adopts job j's refined pose: the registration ended in order and f did not rise.
  bool refineUsable(std::size_t j) const
  {
    const bool ended = r_status_[j] == NDT2D_REFINE_CONVERGED || r_status_[j] == NDT2D_REFINE_MAX_EVALS;
    return ended && r_scores_[j] <= r_start_scores_[j];
  }

  // One ndt2d_matcher_verify_candidates call for the candidates of the round that passed
  // (passing_), each at the pose the walk would adopt for it, all on the one scan.
  bool verifyRound(const double * scan_pose, const double * points_xy, std::size_t n_points, std::size_t K)
  {
    const std::size_t n_jobs = passing_.size();
    v_jobs_.resize(3 * n_jobs);
    for (std::size_t j = 0; j < n_jobs; ++j)
    {
      const bool refined = refine_ && refineUsable(j);
      for (int d = 0; d < 3; ++d)
      {
        v_jobs_[3 * j + d] = refined ? r_poses_[3 * j + d] : corrections_[3 * passing_[j] + d] + scan_pose[d];
      }
    }
    r_scan_.assign(n_jobs, 0u);
    v_records_.assign(NDT2D_VERIFY_RECORD_U32 * n_jobs, 0u);
    const std::size_t point_offsets[2] = {0, n_points};
    return ok(ndt2d_matcher_verify_candidates(m_, offsets_.data(), ids_.data(), poses_.data(), K, v_jobs_.data(), r_scan_.data(),
                                              passing_.data(), n_jobs, points_xy, point_offsets, 1, verify_max_beams_,
                                              v_records_.data(), nullptr, nullptr, nullptr, nullptr, 0));
  }

  std::vector<std::size_t> sizes_;   // point count of stored scan `id`
  std::vector<std::size_t> offsets_, ids_;
  std::vector<double> poses_, corrections_, covariances_, scores_;
  // setRefine()
  bool refine_ = false;
  std::uint32_t max_evals_ = 32;
  double tol_lin_ = 1e-6, tol_ang_ = 1e-6;
  std::size_t laser_max_beams_ = 0;
  std::vector<std::uint32_t> passing_, r_scan_, r_evals_;
  std::vector<std::int32_t> r_status_;
  std::vector<double> r_jobs_, r_poses_, r_scores_, r_start_scores_, r_hessians_;
  // setVerify()
  bool verify_ = false;
  std::size_t verify_max_beams_ = 0;
  std::vector<double> v_jobs_;
  std::vector<std::uint32_t> v_records_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__LOOP_CLOSURE_HIP_HPP_
