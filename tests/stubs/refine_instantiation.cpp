// Compile-only use of ndt_2d_hip::RefineHip (ndt_2d_amd/plugin/refine_hip.hpp): every member is
// instantiated against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/refine_hip.hpp"

int refine_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::RefineHip refiner(matcher);
  refiner.setRules(16, 1.0e-7, 1.0e-7);
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  const double pose_a[3] = {0.0, 0.0, 0.0}, pose_b[3] = {1.0, 0.5, 0.25};
  const std::size_t scan = refiner.addScan(points, 2);
  if (refiner.addJob(scan, pose_a) != 0 || refiner.addJob(scan, pose_b) != 1) return 1;   // two jobs, one scan
  if (refiner.add(pose_b, points, 2) != 2) return 2;
  if (refiner.jobs() != 3 || refiner.scans() != 2) return 3;
  std::vector<ndt_2d_hip::RefinedScan> refined;
  if (!refiner.refine(refined)) return 4;
  float kernel_ms = 0.0f, fetch_ms = 0.0f;
  if (!refiner.lastMs(&kernel_ms, &fetch_ms)) return 5;
  refiner.clear();
  const bool all = refined.size() == 3 && (refined[0].converged() || refined[0].status == NDT2D_REFINE_NO_OVERLAP);
  return refiner.last_error().empty() && all && refiner.jobs() == 0 ? 0 : 6;
}
