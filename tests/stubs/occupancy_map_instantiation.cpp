// Compile-only use of ndt_2d_hip::OccupancyMapHip (ndt_2d_amd/plugin/occupancy_map_hip.hpp): every
// member is instantiated against include/ndt2d_hip.h.  Never linked or run.
#include <vector>

#include "../../ndt_2d_amd/plugin/occupancy_map_hip.hpp"

int occupancy_map_instantiation(ndt2d_handle device)
{
  ndt_2d_hip::OccupancyMapHip map(0.05, 0.25, device);
  if (!map.valid()) return 1;
  const double points[4] = {1.0, 0.0, 0.0, 2.0};
  std::vector<ndt_2d_hip::ScanView> scans;
  scans.push_back(ndt_2d_hip::ScanView{{0.0, 0.0, 0.0}, points, 2});
  ndt_2d_hip::OccupancyGridMsg msg;
  if (!map.getMsg(scans, msg)) return 2;
  double bounds[4];
  std::size_t num_scans = 0;
  if (!map.bounds(bounds, &num_scans)) return 3;
  const ndt2d_occmap_result & last = map.last_update();
  if (last.mode != NDT2D_OCCMAP_FULL || last.beams_traced != 2) return 4;
  if (!map.reset()) return 5;
  return map.last_error().empty() && msg.data.size() == static_cast<std::size_t>(msg.width) * msg.height ? 0 : 6;
}
