// Relocalisation in a loaded map on the batched match of libndt2d_hip.so: one scan matched from K
// start poses against the NDT in place in one call (ndt2d_matcher_match_starts,
// include/ndt2d_hip.h) instead of K matchScan() round trips.
//
// A node started with `map_file` (reference src/ndt_mapper.cpp:106-116,155-186) refuses every
// scan until somebody posts `initialpose` (:315-320, "Can not handle scan, not localized within
// map").  With this header it seeds the search itself: every graph node's pose under a few
// headings (headingFan), one relocalize() call, and the best response below its threshold --
// the loop-closure rule isfinite(score) && score < typical_matcher_response_ (:645) -- is the
// pose it would have been given.  The same call serves a tracker that keeps several hypotheses.
//
// Plain arrays over the C-ABI, as the other mirrors in this directory: nothing of ROS or Eigen.
#ifndef NDT_2D_HIP__RELOCALIZE_HIP_HPP_
#define NDT_2D_HIP__RELOCALIZE_HIP_HPP_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "job_list.hpp"
#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

// One start pose's answer.
struct Relocalization
{
  std::size_t start;         // index into the start poses
  double score;
  bool has_winner;           // a lattice candidate scored below 0 (else the correction is zero)
  double correction[3];      // matchScan's pose output (dx, dy, dth)
  double pose[3];            // start pose + correction, as src/ndt_mapper.cpp:557-561 adds it
  double covariance[9];      // row-major
};

class RelocalizeHip : public MatcherCalls
{
public:
  explicit RelocalizeHip(ndt2d_matcher * matcher) : MatcherCalls(matcher) {}

  // Every pose under n_headings equally spaced headings, the first its own: appends
  // (x, y, theta + 2 pi j / n_headings), j = 0 .. n_headings - 1, per pose to starts_out.
  static void headingFan(const double * poses_xyt, std::size_t n_poses, std::size_t n_headings,
                         std::vector<double> & starts_out)
  {
    const double two_pi = 6.283185307179586476925286766559;
    for (std::size_t k = 0; k < n_poses; ++k)
    {
      for (std::size_t j = 0; j < n_headings; ++j)
      {
        starts_out.push_back(poses_xyt[3 * k]);
        starts_out.push_back(poses_xyt[3 * k + 1]);
        starts_out.push_back(poses_xyt[3 * k + 2] + static_cast<double>(j) * (two_pi / static_cast<double>(n_headings)));
      }
    }
  }

  // One batched match from starts_xyt[3 k ..], k < n_starts.  ranked_out: the starts by score
  // (lower is better), ties in start order; starts without a winner follow those with one,
  // non-finite scores come last.  use_threshold: only isfinite(score) && score < accept_below are
  // kept.  false when the device call fails (last_error()).
  bool relocalize(const double * starts_xyt, std::size_t n_starts, const double * points_xy, std::size_t n_points,
                  bool use_threshold, double accept_below, std::vector<Relocalization> & ranked_out)
  {
    ranked_out.clear();
    if (n_starts == 0) return true;
    corrections_.assign(3 * n_starts, 0.0);
    covariances_.assign(9 * n_starts, 0.0);
    scores_.assign(n_starts, 0.0);
    best_.assign(n_starts, NDT2D_NO_INDEX);
    if (!ok(ndt2d_matcher_match_starts(m_, starts_xyt, n_starts, points_xy, n_points, corrections_.data(),
                                       covariances_.data(), scores_.data(), best_.data(), nullptr, 0, nullptr)))
    {
      return false;
    }
    for (std::size_t k = 0; k < n_starts; ++k)
    {
      if (use_threshold && !(std::isfinite(scores_[k]) && scores_[k] < accept_below)) continue;
      Relocalization r;
      r.start = k;
      r.score = scores_[k];
      r.has_winner = best_[k] != NDT2D_NO_INDEX;
      for (int d = 0; d < 3; ++d)
      {
        r.correction[d] = corrections_[3 * k + d];
        r.pose[d] = r.correction[d] + starts_xyt[3 * k + d];   // correction.x += scan->getPose().x; ...
      }
      for (int d = 0; d < 9; ++d) r.covariance[d] = covariances_[9 * k + d];
      ranked_out.push_back(r);
    }
    std::stable_sort(ranked_out.begin(), ranked_out.end(), [](const Relocalization & a, const Relocalization & b) {
      const bool fa = std::isfinite(a.score), fb = std::isfinite(b.score);
      if (fa != fb) return fa;
      if (!fa) return false;
      if (a.has_winner != b.has_winner) return a.has_winner;
      return a.score < b.score;
    });
    return true;
  }

  // HIP events around the batched match's launches (after the first relocalize()).
  bool lastMs(float * search_ms, float * reduce_ms)
  {
    ndt2d_starts * s = ndt2d_matcher_starts(m_);
    if (s == nullptr) return false;
    return ndt2d_starts_last_ms(s, search_ms, reduce_ms) == NDT2D_OK;
  }

private:
  std::vector<double> corrections_, covariances_, scores_;
  std::vector<uint64_t> best_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__RELOCALIZE_HIP_HPP_
