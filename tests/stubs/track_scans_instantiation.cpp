// Compile-only use of ndt_2d_hip::TrackScansHip (ndt_2d_amd/plugin/track_scans_hip.hpp): every
// member is instantiated against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/track_scans_hip.hpp"

int track_scans_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::TrackScansHip tracker(matcher);
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  const double pose_a[3] = {0.0, 0.0, 0.0}, pose_b[3] = {1.0, 0.5, 0.25};
  const std::size_t scan = tracker.addScan(points, 2);
  if (tracker.addJob(scan, pose_a) != 0 || tracker.addJob(scan, pose_b) != 1) return 1;   // two jobs, one scan
  if (tracker.add(pose_b, points, 2) != 2) return 2;
  if (tracker.jobs() != 3 || tracker.scans() != 2) return 3;
  std::vector<ndt_2d_hip::TrackedScan> tracked;
  if (!tracker.track(tracked)) return 4;
  float search_ms = 0.0f, reduce_ms = 0.0f;
  if (!tracker.lastMs(&search_ms, &reduce_ms)) return 5;
  tracker.clear();
  return tracker.last_error().empty() && tracked.size() == 3 && tracker.jobs() == 0 ? 0 : 6;
}
