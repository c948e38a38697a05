// C++ consumer of ClearanceMapHip (ndt_2d_amd/plugin/clearance_hip.hpp) and of
// ParticleFilterHip::initGlobal(..., min_clearance) (particle_filter_hip.hpp): no Python and no torch
// in this process.  Reads a map and the call's parameters from argv[1], runs the transform capped and
// uncapped, the mask, initGlobal with the clearance on the host map and on the resident map of an
// ndt2d_occupancy_map holding one scan, and writes what it saw to argv[2];
// tests/test_gpu_clearance_mirror.py compares it with the yardsticks and with the Python path.
//   in:  u64 width, height, n, seed, cap; f64 origin_x, origin_y, resolution, clearance;
//        i8 map[height * width]
//   out: u32 min_d2
//        u32 d2[height * width]              uncapped
//        u32 d2[height * width]              capped at `cap`
//        i8 mask[height * width]             of the uncapped transform at min_d2
//        u64 n; f64 particles[n][3]          after initGlobal(map, ..., clearance)
//        u64 step
//        u64 w, h; f64 origin_x, origin_y, resolution; u64 n; f64 particles[n][3]; i8 map[h * w]   the resident map's
#include <cstdint>
#include <cstdio>
#include <vector>

#include "clearance_hip.hpp"
#include "particle_filter_hip.hpp"

namespace
{

bool read(std::FILE * f, void * p, std::size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

void dump(std::FILE * f, ndt_2d_hip::ParticleFilterHip & pf)
{
  const std::vector<double> p = pf.particles();
  std::fwrite(p.data(), sizeof(double), p.size(), f);
}

}  // namespace

int main(int argc, char ** argv)
{
  if (argc != 3) return 2;
  std::FILE * in = std::fopen(argv[1], "rb");
  if (in == nullptr) return 2;
  std::uint64_t head[5];
  double geo[4];
  if (!read(in, head, sizeof(head)) || !read(in, geo, sizeof(geo))) return 2;
  std::vector<signed char> map(head[0] * head[1]);
  if (!read(in, map.data(), map.size())) return 2;
  std::fclose(in);
  const std::uint32_t width = static_cast<std::uint32_t>(head[0]), height = static_cast<std::uint32_t>(head[1]);
  const std::size_t n = head[2];
  const double clearance = geo[3];

  ndt2d_matcher * matcher = nullptr;
  if (ndt2d_matcher_create(&matcher, 0) != NDT2D_OK) return 3;
  if (ndt2d_matcher_initialize(matcher, 0.25, 0.0025, 0.1, 0.005, 0.05, 100, 30.0) != NDT2D_OK) return 3;
  int status = 0;
  std::FILE * out = std::fopen(argv[2], "wb");
  if (out == nullptr) return 2;
  {
    ndt_2d_hip::ClearanceMapHip cm(ndt2d_matcher_device(matcher));
    std::uint32_t min_d2 = 0;
    std::vector<std::uint32_t> d2;
    std::vector<signed char> inflated;
    if (!cm.valid() || !ndt_2d_hip::ClearanceMapHip::minD2(clearance, geo[2], 0, &min_d2)) status = 6;
    std::fwrite(&min_d2, 4, 1, out);
    if (status == 0 && !(cm.compute(map.data(), width, height) && cm.d2(d2))) status = 6;
    std::fwrite(d2.data(), 4, d2.size(), out);
    const bool masked = status == 0 && cm.mask(min_d2) != nullptr && cm.inflated(inflated);
    if (status == 0 && !(cm.compute(map.data(), width, height, false, static_cast<std::int64_t>(head[4])) && cm.d2(d2))) status = 6;
    std::fwrite(d2.data(), 4, d2.size(), out);
    if (!masked) status = 6;
    std::fwrite(inflated.data(), 1, inflated.size(), out);
    // the refusals arrive as false with a message, and the object goes on
    if (cm.compute(nullptr, width, height) || cm.last_error().find("null map") == std::string::npos) status = 7;
    if (cm.width() != width || cm.height() != height || cm.deviceD2() == nullptr) status = 7;
    if (status != 0) std::fprintf(stderr, "clearance: %s\n", cm.last_error().c_str());
  }
  {
    const double alphas[5] = {0.1, 0.1, 0.1, 0.1, 0.05};
    ndt_2d_hip::ParticleFilterHip pf(10, n, alphas, matcher, head[3]);
    pf.initGlobal(map.data(), width, height, geo[0], geo[1], geo[2], 0, nullptr, clearance);
    std::uint64_t count = pf.size();
    std::fwrite(&count, 8, 1, out);
    dump(out, pf);
    const std::uint64_t step = pf.step();
    std::fwrite(&step, 8, 1, out);

    // a resident map: one scan of four points round the origin
    ndt2d_occupancy_map * resident = nullptr;
    ndt2d_occmap_result result;
    const double points[8] = {1.0, 0.0, 0.0, 1.2, -0.9, 0.0, 0.0, -1.1}, pose[3] = {0.1, -0.2, 0.3};
    if (ndt2d_occmap_create(ndt2d_matcher_device(matcher), 0.05, 0.25, &resident) != NDT2D_OK ||
        ndt2d_occmap_append_scan(resident, points, 4, nullptr) != NDT2D_OK ||
        ndt2d_occmap_update(resident, pose, 1, &result) != NDT2D_OK)
    {
      status = 4;
    }
    else
    {
      pf.initGlobal(resident, 300, nullptr, clearance);
      const std::uint64_t dims[2] = {result.info.width, result.info.height};
      const double g[3] = {result.info.origin_x, result.info.origin_y, result.info.resolution};
      std::fwrite(dims, 8, 2, out);
      std::fwrite(g, 8, 3, out);
      count = pf.size();
      std::fwrite(&count, 8, 1, out);
      dump(out, pf);
      std::vector<signed char> data(static_cast<std::size_t>(dims[0]) * dims[1]);
      if (ndt2d_occmap_read(resident, 0, 0, result.info.width, result.info.height, data.data(), result.info.width) != NDT2D_OK) status = 4;
      std::fwrite(data.data(), 1, data.size(), out);
    }
    if (resident != nullptr) ndt2d_occmap_destroy(resident);
    if (!pf.ok())
    {
      std::fprintf(stderr, "filter: %s\n", pf.last_error().c_str());
      status = 5;
    }
  }
  std::fclose(out);
  ndt2d_matcher_destroy(matcher);
  return status;
}
