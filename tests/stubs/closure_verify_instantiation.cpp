// Compile-only use of the verification members of ndt_2d_hip::LoopClosureHip
// (ndt_2d_amd/plugin/loop_closure_hip.hpp) against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/loop_closure_hip.hpp"

int closure_verify_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::LoopClosureHip closer(matcher);
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  if (!closer.storeScan(points, 2)) return 1;
  if (closer.setVerify(720, 5, 9.0, 1.0, true)) return 2;    // refused: 1 or 9 cells
  if (closer.setVerify(720, 9, -1.0, 1.0, true)) return 3;   // refused: a negative gate
  if (!closer.setVerify(720, 9, 9.0, 1.0, true)) return 4;
  if (!closer.setRefine(32, 1e-6, 1e-6, 9, 720)) return 5;   // (with the refinement: verified at the adopted pose)
  double pose[3] = {0.0, 0.0, 0.0};
  const double graph_poses[6] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0};
  std::vector<ndt_2d_hip::LoopClosure> closures;
  if (!closer.closeLoops(pose, points, 2, std::vector<std::size_t>{0, 1}, graph_poses, 1, -0.5, 3, closures)) return 6;
  std::uint32_t beams = 0;
  for (const ndt_2d_hip::LoopClosure & c : closures)
  {
    if (!c.verified) return 7;
    // {n_beams, n_off, n_unseen, n_outlier, n_inlier, n_pierced, n_walked, 0}
    if (c.verify[1] + c.verify[2] + c.verify[3] + c.verify[4] != c.verify[0] || c.verify[5] > c.verify[6]) return 8;
    beams += c.verify[0];
    if (!(c.verified_pose[0] == c.verified_pose[0])) return 9;
  }
  closer.clearVerify();
  closer.clearRefine();
  // the C entry points themselves
  const std::size_t offsets[2] = {0, 1}, ids[1] = {0}, point_offsets[2] = {0, 2};
  const double job[3] = {0.0, 0.0, 0.0};
  std::uint32_t record[NDT2D_VERIFY_RECORD_U32];
  std::size_t beam_offsets[2];
  std::uint8_t classes[2];
  double m2[2];
  std::uint32_t cells[4];
  if (ndt2d_matcher_verify_candidates(matcher, offsets, ids, graph_poses, 1, job, nullptr, nullptr, 1, points, point_offsets, 1, 0,
                                      record, beam_offsets, classes, m2, cells, 2) != NDT2D_OK)
  {
    return 10;
  }
  ndt2d_closure * closure = ndt2d_matcher_closure(matcher);
  std::uint32_t n = 0;
  double gate_inlier = 0.0, gate_pierce = 0.0;
  int rays = 0;
  if (ndt2d_closure_set_verify_neighbourhood(closure, 9) != NDT2D_OK || ndt2d_closure_verify_neighbourhood(closure, &n) != NDT2D_OK ||
      ndt2d_closure_set_verify_gates(closure, 9.0, 1.0) != NDT2D_OK ||
      ndt2d_closure_verify_gates(closure, &gate_inlier, &gate_pierce) != NDT2D_OK ||
      ndt2d_closure_set_verify_rays(closure, 1) != NDT2D_OK || ndt2d_closure_verify_rays(closure, &rays) != NDT2D_OK)
  {
    return 11;
  }
  if (ndt2d_closure_verify(closure, 1, offsets, ids, graph_poses, 0.25, 4.75, job, nullptr, nullptr, 1, points, point_offsets, 1,
                           record, classes, m2, cells) != NDT2D_OK)
  {
    return 12;
  }
  return n == 9 && rays == 1 && gate_inlier == 9.0 && gate_pierce == 1.0 && beams + record[0] > 0 ? 0 : 13;
}
