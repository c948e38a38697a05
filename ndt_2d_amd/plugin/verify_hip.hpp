// Match verification for many scans at once on libndt2d_hip.so: which beams of K (scan, pose) jobs
// the NDT in place explains, in one call (ndt2d_matcher_verify_scans, include/ndt2d_hip.h, "Match
// verification").
//
// matchScan, the batched matches and the registration turn a scan and a guess into a pose and one
// number, the mean NDT score, which the reference compares with typical_matcher_response_
// (src/ndt_mapper.cpp:645).  A mean cannot tell beams that land on a wall from beams that land in
// space the map never saw, and never looks at the rays, which in a wrong basin pass through walls.
// verify() gives, per job, the count of beams off the grid, unseen, outliers, inliers, and of beams
// whose ray is pierced by a cell's Gaussian on its way -- and, if wanted, the verdict per beam: a
// loop-closure or relocalisation gate looks at the counts; a node that stores every accepted scan
// keeps the beams explained() marks (setMaxBeams(0): every point of the scan).  addScan() /
// addJob() collect the jobs as RefineHip does, verify() makes the one call.  No policy is applied.
//
// Plain arrays over the C-ABI, as the other mirrors in this directory: nothing of ROS or Eigen.
#ifndef NDT_2D_HIP__VERIFY_HIP_HPP_
#define NDT_2D_HIP__VERIFY_HIP_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "job_list.hpp"
#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// One job's answer.  The per-beam vectors are filled only with setWantBeams(true).
struct VerifiedScan
{
  std::size_t job;           // index into the jobs, in add order
  std::size_t scan;          // index into the scans
  std::uint32_t beams;       // the scan's beams in use
  std::uint32_t off, unseen, outlier, inlier;   // the classes' counts: they add up to beams
  std::uint32_t pierced;     // beams whose ray met a piercing cell
  std::uint32_t walked;      // beams whose ray was walked
  std::vector<std::uint8_t> classes;        // NDT2D_BEAM_OFF .. NDT2D_BEAM_INLIER | NDT2D_BEAM_PIERCED
  std::vector<double> m2;                   // +inf for off and unseen
  std::vector<std::uint32_t> cells;         // [beam][2]: the cell whose m2 won, the first piercing cell
  // Is beam i worth storing: the map does not contradict it.
  bool explained(std::size_t i) const
  {
    return (classes[i] & 3u) != NDT2D_BEAM_OUTLIER && (classes[i] & NDT2D_BEAM_PIERCED) == 0u;
  }
};

// addScan() / addJob() / add(), clear(), jobs() and scans() are JobList's (job_list.hpp).
class VerifyHip : public JobList, public MatcherCalls
{
public:
  explicit VerifyHip(ndt2d_matcher * matcher) : MatcherCalls(matcher) {}

  // The parameters of the next verify() on; false: refused (last_error()), the value stays.
  bool setNeighbourhood(std::uint32_t cells) { return ok(ndt2d_matcher_set_verify_neighbourhood(m_, cells)); }
  bool setGates(double gate_inlier, double gate_pierce) { return ok(ndt2d_matcher_set_verify_gates(m_, gate_inlier, gate_pierce)); }
  bool setRays(bool enabled) { return ok(ndt2d_matcher_set_verify_rays(m_, enabled ? 1 : 0)); }
  // Beams of a scan in use: min(max_beams, its points) by matchScan's subsampling -- the matcher's
  // laser_max_beams for a verdict about the beams the score came from; 0: every point.
  void setMaxBeams(std::size_t max_beams) { max_beams_ = max_beams; }
  void setWantBeams(bool want) { want_beams_ = want; }

  // One call for every job collected; verified_out in job order.  false when the call fails
  // (last_error(); no NDT in place is such a failure).  The collected scans and jobs stay until clear().
  bool verify(std::vector<VerifiedScan> & verified_out)
  {
    verified_out.clear();
    const std::size_t n_jobs = jobs();
    if (n_jobs == 0) return true;
    std::size_t cap = 0;
    for (std::size_t k = 0; k < n_jobs; ++k)
    {
      const std::size_t sc = job_scan_[k];
      if (sc >= scans()) continue;   // (the call refuses the job)
      cap += beams_in_use(points_of(sc), max_beams_, true);
    }
    records_.assign(NDT2D_VERIFY_RECORD_U32 * n_jobs, 0u);
    table_.assign(n_jobs + 1, 0);
    if (want_beams_)
    {
      classes_.assign(cap, 0);
      m2_.assign(cap, 0.0);
      cells_.assign(2 * cap, NDT2D_VERIFY_NO_CELL);
    }
    if (!ok(ndt2d_matcher_verify_scans(m_, jobs_.data(), job_scan_.data(), n_jobs, points_.data(), offsets_.data(), scans(), max_beams_,
                                       records_.data(), table_.data(), want_beams_ ? classes_.data() : nullptr,
                                       want_beams_ ? m2_.data() : nullptr, want_beams_ ? cells_.data() : nullptr, cap)))
    {
      return false;
    }
    verified_out.reserve(n_jobs);
    for (std::size_t k = 0; k < n_jobs; ++k)
    {
      const std::uint32_t * rec = records_.data() + NDT2D_VERIFY_RECORD_U32 * k;
      VerifiedScan v;
      v.job = k;
      v.scan = job_scan_[k];
      v.beams = rec[0];
      v.off = rec[1];
      v.unseen = rec[2];
      v.outlier = rec[3];
      v.inlier = rec[4];
      v.pierced = rec[5];
      v.walked = rec[6];
      if (want_beams_)
      {
        v.classes.assign(classes_.begin() + table_[k], classes_.begin() + table_[k + 1]);
        v.m2.assign(m2_.begin() + table_[k], m2_.begin() + table_[k + 1]);
        v.cells.assign(cells_.begin() + 2 * table_[k], cells_.begin() + 2 * table_[k + 1]);
      }
      verified_out.push_back(v);
    }
    return true;
  }

  // HIP events around the call's kernel launch and read-back (after the first verify()).
  bool lastMs(float * kernel_ms, float * fetch_ms)
  {
    ndt2d_verify * v = ndt2d_matcher_verify(m_);
    if (v == nullptr) return false;
    return ndt2d_verify_last_ms(v, kernel_ms, fetch_ms) == NDT2D_OK;
  }

private:
  std::size_t max_beams_ = 100;   // the plugin's declared laser_max_beams default
  bool want_beams_ = false;
  std::vector<std::uint32_t> records_, cells_;
  std::vector<std::size_t> table_;
  std::vector<std::uint8_t> classes_;
  std::vector<double> m2_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__VERIFY_HIP_HPP_
