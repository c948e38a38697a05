// Compile-only use of ndt_2d_hip::WideSearchHip (ndt_2d_amd/plugin/wide_search_hip.hpp): every
// member is instantiated against include/ndt2d_hip.h.  Never linked or run.
#include "../../ndt_2d_amd/plugin/wide_search_hip.hpp"

int wide_search_instantiation(ndt2d_matcher * matcher)
{
  ndt_2d_hip::WideSearchHip wide(matcher);
  const double pose[3] = {0.1, -0.2, 0.3};
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  ndt_2d_hip::WideMatch match;
  if (!wide.matchWide(pose, points, 2, 1.0, 0.05, 0.2, 0.01, match)) return 1;
  if (!wide.matchWide(pose, points, 2, 1.0, 0.05, 0.2, 0.01, match, 4)) return 2;
  if (!wide.setTile(8, 2) || !wide.setTiming(true)) return 3;
  float image_ms = 0.0f, bounds_ms = 0.0f, sort_ms = 0.0f, exact_ms = 0.0f;
  if (!wide.lastMs(&image_ms, &bounds_ms, &sort_ms, &exact_ms)) return 4;
  return wide.last_error().empty() && match.has_winner && !match.near_tie && match.tiles_scored <= match.tiles_total ? 0 : 5;
}
