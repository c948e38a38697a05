// Compile-only use of ndt_2d_hip::VerifyHip (ndt_2d_amd/plugin/verify_hip.hpp): every member is
// instantiated against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/verify_hip.hpp"

int verify_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::VerifyHip verifier(matcher);
  if (!verifier.setNeighbourhood(9) || !verifier.setGates(9.0, 1.0) || !verifier.setRays(true)) return 1;
  verifier.setMaxBeams(0);
  verifier.setWantBeams(true);
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  const double pose_a[3] = {0.0, 0.0, 0.0}, pose_b[3] = {1.0, 0.5, 0.25};
  const std::size_t scan = verifier.addScan(points, 2);
  if (verifier.addJob(scan, pose_a) != 0 || verifier.addJob(scan, pose_b) != 1) return 2;   // two jobs, one scan
  if (verifier.add(pose_b, points, 2) != 2) return 3;
  if (verifier.jobs() != 3 || verifier.scans() != 2) return 4;
  std::vector<ndt_2d_hip::VerifiedScan> verified;
  if (!verifier.verify(verified)) return 5;
  float kernel_ms = 0.0f, fetch_ms = 0.0f;
  if (!verifier.lastMs(&kernel_ms, &fetch_ms)) return 6;
  verifier.clear();
  const bool all = verified.size() == 3 && verified[0].beams == 2 && verified[0].classes.size() == 2 &&
                   verified[0].off + verified[0].unseen + verified[0].outlier + verified[0].inlier == verified[0].beams;
  return verifier.last_error().empty() && all && verified[0].explained(0) && verifier.jobs() == 0 ? 0 : 7;
}
