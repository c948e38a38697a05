// ndt_2d::OccupancyGrid for a node that publishes after every scan: the resident counterpart
// of OccupancyGridHip (occupancy_grid_hip.hpp).
//
// Same constructor arguments, the same getMsg over plain arrays and the same message struct.
// The scans' points, the hit / empty counters and the map stay on the GPU in an
// ndt2d_occupancy_map (include/ndt2d_hip.h): getMsg appends the scans it has not seen, passes the
// poses, and patches into the caller's message only the rectangle of cells the update reports --
// the whole map after a full re-trace (new geometry or moved poses), the new scans' bounding box
// after an incremental one, nothing when nothing changed.  All map cells are written by the
// device; nothing here touches one.
//
// Ownership: one object per generator; it must be destroyed before the ndt2d_handle it was made
// on; a scan's points may not change once getMsg has seen it (reset() after dropping or
// replacing scans).  The message passed to getMsg must be the one the previous call filled (or
// an empty one): what lies outside the rectangle is kept, not written again.
#ifndef NDT_2D_HIP__OCCUPANCY_MAP_HIP_HPP_
#define NDT_2D_HIP__OCCUPANCY_MAP_HIP_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ndt2d_hip.h"
#include "occupancy_grid_hip.hpp"   // ScanView, OccupancyGridMsg

namespace ndt_2d_hip
{

class OccupancyMapHip
{
public:
  OccupancyMapHip(double resolution, double occ_thresh, ndt2d_handle device)
  {
    const int rc = ndt2d_occmap_create(device, resolution, occ_thresh, &map_);
    if (rc != NDT2D_OK) error_ = "ndt2d_occmap_create: ndt2d error " + std::to_string(rc);
  }
  ~OccupancyMapHip()
  {
    if (map_ != nullptr) (void)ndt2d_occmap_destroy(map_);
  }
  OccupancyMapHip(const OccupancyMapHip &) = delete;
  OccupancyMapHip & operator=(const OccupancyMapHip &) = delete;

  bool valid() const { return map_ != nullptr; }

  // src/occupancy_grid.cpp:44-152.  Returns false (and keeps last_error()) when a device call
  // fails or an already-seen scan changed its point count; the reference has no failure path.
  bool getMsg(const std::vector<ScanView> & scans, OccupancyGridMsg & grid)
  {
    if (map_ == nullptr) return false;
    for (std::size_t k = 0; k < scans.size(); ++k)
    {
      if (k < seen_.size())
      {
        if (scans[k].n_points != seen_[k])
        {
          error_ = "scan " + std::to_string(k) + " changed its point count: appended scans are "
                   "immutable, call reset() after replacing or dropping scans";
          return false;
        }
        continue;
      }
      if (!ok(ndt2d_occmap_append_scan(map_, scans[k].points_xy, scans[k].n_points, nullptr)))
      {
        return false;
      }
      seen_.push_back(scans[k].n_points);
    }
    poses_.clear();
    for (const ScanView & s : scans) poses_.insert(poses_.end(), s.pose, s.pose + 3);
    ndt2d_occmap_result res;
    if (!ok(ndt2d_occmap_update(map_, poses_.data(), scans.size(), &res))) return false;
    last_ = res;
    const std::size_t n_cells = static_cast<std::size_t>(res.info.width) * res.info.height;
    if (res.mode == NDT2D_OCCMAP_FULL || grid.data.size() != n_cells || grid.width != res.info.width)
    {
      // a message that is not the previous call's gets the whole map
      grid.data.assign(n_cells, 0);
      res.rect_x0 = 0;
      res.rect_y0 = 0;
      res.rect_w = res.info.width;
      res.rect_h = res.info.height;
    }
    grid.resolution = res.info.resolution;
    grid.width = res.info.width;
    grid.height = res.info.height;
    grid.origin_x = res.info.origin_x;
    grid.origin_y = res.info.origin_y;
    if (res.rect_w == 0 || res.rect_h == 0) return true;
    signed char * first = grid.data.data() + static_cast<std::size_t>(res.rect_y0) * grid.width + res.rect_x0;
    return ok(ndt2d_occmap_read(map_, res.rect_x0, res.rect_y0, res.rect_w, res.rect_h, first, grid.width));
  }

  // A new generator: scans, counters and bounds are forgotten.
  bool reset()
  {
    seen_.clear();
    return map_ != nullptr && ok(ndt2d_occmap_reset(map_));
  }

  // min_x_, max_x_, min_y_, max_y_ and num_scans_
  bool bounds(double * bounds4_out, std::size_t * num_scans_out)
  {
    return map_ != nullptr && ok(ndt2d_occmap_bounds(map_, bounds4_out, num_scans_out));
  }
  // mode, beams traced and dirty rectangle of the last getMsg
  const ndt2d_occmap_result & last_update() const { return last_; }
  const std::string & last_error() const { return error_; }

private:
  bool ok(int rc)
  {
    if (rc == NDT2D_OK) return true;
    error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_occmap_last_error(map_);
    return false;
  }

  ndt2d_occupancy_map * map_ = nullptr;
  std::vector<std::size_t> seen_;
  std::vector<double> poses_;
  ndt2d_occmap_result last_{};
  std::string error_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__OCCUPANCY_MAP_HIP_HPP_
