// matchScan over a window of metres and radians on the wide search of libndt2d_hip.so
// (ndt2d_matcher_match_wide, include/ndt2d_hip.h): the exhaustive lattice's winner -- the same
// score bits and the same index -- found by scoring only the tiles of the translation lattice
// whose rigorous upper bound can still hold it.
//
// The loop-closure thread of the reference matches a scan against each candidate's map with
// global_scan_matcher_, a ScanMatcherNDT whose lattice is global_search_size wide
// (src/ndt_mapper.cpp:127-150,600-660).  Where that window grows to metres after drift, matchWide()
// on the matcher that holds the candidate's NDT replaces its matchScan(): the correction and the
// score are matchScan's; a covariance comes from RefineHip with the 9-cell neighbourhood on the
// winner (refine_hip.hpp), since the reference's covariance sums need every candidate.
//
// Plain arrays over the C-ABI, as the other mirrors in this directory: nothing of ROS or Eigen.
#ifndef NDT_2D_HIP__WIDE_SEARCH_HIP_HPP_
#define NDT_2D_HIP__WIDE_SEARCH_HIP_HPP_

#include <cstddef>
#include <cstdint>

#include "job_list.hpp"
#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

struct WideMatch
{
  double score;              // best / N, as matchScan returns it (0.0: no NDT, or nothing scored below 0)
  bool has_winner;
  bool near_tie;             // another candidate within NDT2D_NEAR_TIE_REL of the winner (marked, not settled)
  uint64_t best_index;       // flat index in the call's lattice; NDT2D_NO_INDEX without a winner
  double correction[3];      // matchScan's pose output (dx, dy, dth); zeros without a winner
  double pose[3];            // scan pose + correction, as src/ndt_mapper.cpp:557-561 adds it
  uint64_t tiles_scored, tiles_total;
};

class WideSearchHip : public MatcherCalls
{
public:
  explicit WideSearchHip(ndt2d_matcher * matcher) : MatcherCalls(matcher) {}

  // The lattice is the call's: +-linear_size at linear_resolution, +-angular_size at
  // angular_resolution, visited as the reference's loops visit them.  tile_steps == 0 keeps the
  // tile steps in place.  false when the call is refused or fails (last_error()).
  bool matchWide(const double * scan_pose_xyt, const double * points_xy, std::size_t n_points, double linear_size,
                 double linear_resolution, double angular_size, double angular_resolution, WideMatch & out,
                 uint32_t tile_steps = 0)
  {
    out = WideMatch{};
    out.best_index = NDT2D_NO_INDEX;
    int near = 0;
    uint64_t stats[2] = {0, 0};
    if (!ok(ndt2d_matcher_match_wide(m_, scan_pose_xyt, points_xy, n_points, linear_size, linear_resolution, angular_size,
                                     angular_resolution, tile_steps, out.correction, &out.score, &out.best_index, &near,
                                     stats)))
    {
      return false;
    }
    out.has_winner = out.best_index != NDT2D_NO_INDEX;
    out.near_tie = near != 0;
    for (int d = 0; d < 3; ++d) out.pose[d] = out.correction[d] + scan_pose_xyt[d];   // correction.x += scan->getPose().x; ...
    out.tiles_scored = stats[0];
    out.tiles_total = stats[1];
    return true;
  }

  // Tile geometry of the matcher's object (after the first matchWide() with an NDT in place).
  bool setTile(uint32_t tile_steps, uint32_t pixels_per_tile)
  {
    ndt2d_wide * w = ndt2d_matcher_wide(m_);
    return w != nullptr && ndt2d_wide_set_tile(w, tile_steps, pixels_per_tile) == NDT2D_OK;
  }

  // HIP events round the image, the bounds, the sort and the exact rounds of the last matchWide().
  bool setTiming(bool enabled)
  {
    ndt2d_wide * w = ndt2d_matcher_wide(m_);
    return w != nullptr && ndt2d_wide_set_timing(w, enabled ? 1 : 0) == NDT2D_OK;
  }
  bool lastMs(float * image_ms, float * bounds_ms, float * sort_ms, float * exact_ms)
  {
    ndt2d_wide * w = ndt2d_matcher_wide(m_);
    return w != nullptr && ndt2d_wide_last_ms(w, image_ms, bounds_ms, sort_ms, exact_ms) == NDT2D_OK;
  }
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__WIDE_SEARCH_HIP_HPP_
