// Compile-only use of the neighbourhood and covariance members of ndt_2d_hip::RefineHip
// (ndt_2d_amd/plugin/refine_hip.hpp) against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/refine_hip.hpp"

int refine_neighbours_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::RefineHip refiner(matcher);
  if (!refiner.setNeighbourhood(9) || refiner.neighbourhood() != 9) return 1;
  if (refiner.setNeighbourhood(5)) return 2;   // refused: 1 or 9
  refiner.setLaserMaxBeams(720);
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  const double pose[3] = {1.0, 0.5, 0.25};
  refiner.add(pose, points, 2);
  std::vector<ndt_2d_hip::RefinedScan> refined;
  if (!refiner.refine(refined) || refined.size() != 1) return 3;
  const ndt_2d_hip::RefinedScan & r = refined[0];
  if (r.beams != 2) return 4;
  double trace = 0.0;
  if (r.has_covariance)
  {
    const double (&c)[9] = r.covariance;
    if (c[1] != c[3] || c[2] != c[6] || c[5] != c[7]) return 5;
    trace = c[0] + c[4] + c[8];
  }
  // the C entry point on a Hessian of the caller's own
  const double H6[6] = {4.0, 0.0, 0.0, 16.0, 0.0, 0.25};
  double cov9[9];
  if (ndt2d_refine_covariance(H6, cov9) != NDT2D_OK) return 6;
  return trace >= 0.0 && refiner.setNeighbourhood(1) ? 0 : 7;
}
