// Compile-only use of the refinement members of ndt_2d_hip::LoopClosureHip
// (ndt_2d_amd/plugin/loop_closure_hip.hpp) against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/loop_closure_hip.hpp"

int closure_refine_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::LoopClosureHip closer(matcher);
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  if (!closer.storeScan(points, 2)) return 1;
  if (closer.setRefine(32, 1e-6, 1e-6, 5, 720)) return 2;   // refused: 1 or 9 cells
  if (!closer.setRefine(32, 1e-6, 1e-6, 9, 720)) return 3;
  double pose[3] = {0.0, 0.0, 0.0};
  const double graph_poses[6] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  std::vector<ndt_2d_hip::LoopClosure> closures;
  if (!closer.closeLoops(pose, points, 2, std::vector<std::size_t>{0, 1}, graph_poses, 1, -0.5, 3, closures)) return 4;
  double trace = 0.0;
  for (const ndt_2d_hip::LoopClosure & c : closures)
  {
    if (!c.refined) return 5;
    if (c.refine_status == NDT2D_REFINE_NOT_FINITE) continue;
    if (c.has_refined_covariance) trace += c.refined_covariance[0] + c.refined_covariance[4] + c.refined_covariance[8];
    trace += c.refined_pose[0] - c.pose[0];
  }
  closer.clearRefine();
  // the C entry points themselves
  const std::size_t offsets[2] = {0, 1}, ids[1] = {0}, point_offsets[2] = {0, 2};
  const double job[3] = {0.0, 0.0, 0.0};
  double pose_out[3], score = 0.0;
  std::int32_t status = 0;
  if (ndt2d_matcher_refine_candidates(matcher, offsets, ids, graph_poses, 1, job, nullptr, nullptr, 1, points, point_offsets, 1,
                                      32, 1e-6, 1e-6, pose_out, &score, nullptr, nullptr, nullptr, &status, nullptr) != NDT2D_OK)
  {
    return 6;
  }
  std::uint32_t cells = 0;
  ndt2d_closure * closure = ndt2d_matcher_closure(matcher);
  if (ndt2d_closure_set_neighbourhood(closure, 9) != NDT2D_OK || ndt2d_closure_neighbourhood(closure, &cells) != NDT2D_OK) return 7;
  double record[NDT2D_REFINE_RECORD_DOUBLES];
  if (ndt2d_closure_refine(closure, 1, offsets, ids, graph_poses, 0.25, 4.75, job, nullptr, nullptr, 1, points, point_offsets, 1,
                           32, 1e-6, 1e-6, record) != NDT2D_OK)
  {
    return 8;
  }
  return trace == trace && cells == 9 ? 0 : 9;
}
