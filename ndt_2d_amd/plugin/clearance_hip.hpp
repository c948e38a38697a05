// The clearance map for a C++ node: a thin RAII mirror of the ndt2d_clearance_* calls
// (include/ndt2d_hip.h, "Clearance map").  For every cell of an int8 occupancy map the exact squared
// Euclidean distance in cells to the nearest obstacle, computed and kept on the GPU, and the map with
// the free cells nearer than a threshold marked 99 -- the inflated map a planner takes, and what
// ParticleFilterHip::initGlobal(..., min_clearance) seeds from.
//
// Ownership: one object per user; it must be destroyed before the ndt2d_handle it was made on.  The
// device pointers it hands out are its own, read-only, and valid until the next compute or mask.
// Error behaviour follows the other mirrors: no exceptions; a call returns false and last_error()
// tells why.
#ifndef NDT_2D_HIP__CLEARANCE_HIP_HPP_
#define NDT_2D_HIP__CLEARANCE_HIP_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ndt2d_hip.h"

namespace ndt_2d_hip
{

class ClearanceMapHip
{
public:
  explicit ClearanceMapHip(ndt2d_handle device)
  {
    const int rc = ndt2d_clearance_create(device, &c_);
    if (rc != NDT2D_OK) error_ = "ndt2d_clearance_create: ndt2d error " + std::to_string(rc);
  }
  ~ClearanceMapHip()
  {
    if (c_ != nullptr) (void)ndt2d_clearance_destroy(c_);
  }
  ClearanceMapHip(const ClearanceMapHip &) = delete;
  ClearanceMapHip & operator=(const ClearanceMapHip &) = delete;

  bool valid() const { return c_ != nullptr; }

  // ceil((clearance_m / resolution)^2); false when the library refuses the pair (host arithmetic only)
  static bool minD2(double clearance_m, double resolution, std::int64_t max_cells, std::uint32_t * out)
  {
    return ndt2d_clearance_min_d2(clearance_m, resolution, max_cells, out) == NDT2D_OK;
  }

  // The transform of a HOST row-major int8 map; max_cells = R > 0 reports every cell farther than R
  // cells as NDT2D_CLEARANCE_FAR.
  bool compute(const signed char * map, std::uint32_t width, std::uint32_t height, bool unknown_is_obstacle = false,
               std::int64_t max_cells = 0)
  {
    return c_ != nullptr && took(ndt2d_clearance_compute(c_, map, width, height, unknown_is_obstacle ? 1 : 0, max_cells),
                                 width, height);
  }
  // The same from a DEVICE map.
  bool computeDevice(const signed char * d_map, std::uint32_t width, std::uint32_t height,
                     bool unknown_is_obstacle = false, std::int64_t max_cells = 0)
  {
    return c_ != nullptr &&
           took(ndt2d_clearance_compute_device(c_, d_map, width, height, unknown_is_obstacle ? 1 : 0, max_cells), width,
                height);
  }
  // The same from the resident map of an ndt2d_occupancy_map's last update: nothing is uploaded.
  bool compute(ndt2d_occupancy_map * resident, bool unknown_is_obstacle = false, std::int64_t max_cells = 0,
               ndt2d_occupancy_info * info_out = nullptr)
  {
    if (c_ == nullptr) return false;
    const signed char * d_map = nullptr;
    ndt2d_occupancy_info info;
    const int rc = ndt2d_occmap_device_map(resident, &d_map, &info);
    if (rc != NDT2D_OK)
    {
      error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_occmap_last_error(resident);
      return false;
    }
    if (info_out != nullptr) *info_out = info;
    return computeDevice(d_map, info.width, info.height, unknown_is_obstacle, max_cells);
  }

  std::uint32_t width() const { return width_; }
  std::uint32_t height() const { return height_; }

  // d2 of the whole map, row-major
  bool d2(std::vector<std::uint32_t> & out)
  {
    out.assign(static_cast<std::size_t>(width_) * height_, 0);
    return c_ != nullptr && ok(ndt2d_clearance_read(c_, 0, 0, width_, height_, out.data(), width_));
  }
  // a rectangle of it into out[h][row_stride]
  bool d2(std::uint32_t x0, std::uint32_t y0, std::uint32_t w, std::uint32_t h, std::uint32_t * out,
          std::size_t row_stride)
  {
    return c_ != nullptr && ok(ndt2d_clearance_read(c_, x0, y0, w, h, out, row_stride));
  }
  // the resident d2 (DEVICE, read-only)
  const std::uint32_t * deviceD2()
  {
    const std::uint32_t * p = nullptr;
    std::uint32_t w = 0, h = 0;
    return c_ != nullptr && ok(ndt2d_clearance_device(c_, &p, &w, &h)) ? p : nullptr;
  }

  // The object's own DEVICE map in which every free cell with d2 < min_d2 is 99; nullptr on failure.
  const signed char * mask(std::uint32_t min_d2)
  {
    const signed char * p = nullptr;
    return c_ != nullptr && ok(ndt2d_clearance_mask(c_, min_d2, &p)) ? p : nullptr;
  }
  // The host copy of the last mask: the inflated map.
  bool inflated(std::vector<signed char> & out)
  {
    out.assign(static_cast<std::size_t>(width_) * height_, 0);
    return c_ != nullptr && ok(ndt2d_clearance_read_mask(c_, 0, 0, width_, height_, out.data(), width_));
  }

  bool setTiming(bool enabled) { return c_ != nullptr && ok(ndt2d_clearance_set_timing(c_, enabled ? 1 : 0)); }
  bool lastMs(float * transform_ms, float * mask_ms)
  {
    return c_ != nullptr && ok(ndt2d_clearance_last_ms(c_, transform_ms, mask_ms));
  }

  const std::string & last_error() const { return error_; }

private:
  bool ok(int rc)
  {
    if (rc == NDT2D_OK) return true;
    error_ = std::string("ndt2d error ") + std::to_string(rc) + ": " + ndt2d_clearance_last_error(c_);
    return false;
  }
  bool took(int rc, std::uint32_t width, std::uint32_t height)
  {
    if (!ok(rc)) return false;
    width_ = width;
    height_ = height;
    return true;
  }

  ndt2d_clearance * c_ = nullptr;
  std::uint32_t width_ = 0, height_ = 0;
  std::string error_;
};

}  // namespace ndt_2d_hip

#endif  // NDT_2D_HIP__CLEARANCE_HIP_HPP_
