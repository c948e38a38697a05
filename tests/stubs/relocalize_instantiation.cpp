// Compile-only use of ndt_2d_hip::RelocalizeHip (ndt_2d_amd/plugin/relocalize_hip.hpp): every
// member is instantiated against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/relocalize_hip.hpp"

int relocalize_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::RelocalizeHip reloc(matcher);
  const double nodes[6] = {0.0, 0.0, 0.0, 1.0, 0.5, 0.25};
  std::vector<double> starts;
  ndt_2d_hip::RelocalizeHip::headingFan(nodes, 2, 4, starts);
  if (starts.size() != 2 * 4 * 3) return 1;
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  std::vector<ndt_2d_hip::Relocalization> ranked;
  if (!reloc.relocalize(starts.data(), starts.size() / 3, points, 2, true, -0.2, ranked)) return 2;
  float search_ms = 0.0f, reduce_ms = 0.0f;
  if (!reloc.lastMs(&search_ms, &reduce_ms)) return 3;
  return reloc.last_error().empty() && ranked.empty() ? 0 : 4;
}
