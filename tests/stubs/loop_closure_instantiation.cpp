// Compile-only use of ndt_2d_hip::LoopClosureHip (ndt_2d_amd/plugin/loop_closure_hip.hpp): every
// member is instantiated against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/loop_closure_hip.hpp"

int loop_closure_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::LoopClosureHip closer(matcher);
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  std::size_t id = 0;
  if (!closer.storeScan(points, 2, &id)) return 1;
  std::size_t b = 0, e = 0;
  ndt_2d_hip::LoopClosureHip::window(3, 3, &b, &e);
  if (b != 2 || e != 3) return 2;
  double pose[3] = {0.0, 0.0, 0.0};
  const double graph_poses[6] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  std::vector<ndt_2d_hip::LoopClosure> closures;
  if (!closer.closeLoops(pose, points, 2, std::vector<std::size_t>{0, 1}, graph_poses, 1, -0.5, 3, closures)) return 3;
  if (!closer.dropScans()) return 4;
  return closer.last_error().empty() && closures.empty() ? 0 : 5;
}
