// C++ consumer of ParticleFilterHip::initGlobal / inject (ndt_2d_amd/plugin/particle_filter_hip.hpp):
// no Python and no torch in this process.  Reads a map and the call's parameters from argv[1], runs
// initGlobal on the host map, inject, and initGlobal on the resident map of an ndt2d_occupancy_map
// holding one scan, and writes every set it saw to argv[2]; tests/test_gpu_seed_mirror.py compares
// them with the restatement bit for bit.
//   in:  u64 width, height, n, seed; f64 origin_x, origin_y, resolution, probability;
//        i8 map[height * width]
//   out: u64 n; f64 particles[n][3]      after initGlobal(map)
//        u64 replaced; f64 particles[n][3]   after inject(probability)
//        u64 step
//        u64 w, h; f64 origin_x, origin_y, resolution; u64 n; f64 particles[n][3]   the resident map's
#include <cstdint>
#include <cstdio>
#include <vector>

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
  std::uint64_t head[4];
  double geo[4];
  if (!read(in, head, sizeof(head)) || !read(in, geo, sizeof(geo))) return 2;
  std::vector<signed char> map(head[0] * head[1]);
  if (!read(in, map.data(), map.size())) return 2;
  std::fclose(in);
  const std::uint32_t width = static_cast<std::uint32_t>(head[0]), height = static_cast<std::uint32_t>(head[1]);
  const std::size_t n = head[2];

  ndt2d_matcher * matcher = nullptr;
  if (ndt2d_matcher_create(&matcher, 0) != NDT2D_OK) return 3;
  if (ndt2d_matcher_initialize(matcher, 0.25, 0.0025, 0.1, 0.005, 0.05, 100, 30.0) != NDT2D_OK) return 3;
  int status = 0;
  std::FILE * out = std::fopen(argv[2], "wb");
  if (out == nullptr) return 2;
  {
    const double alphas[5] = {0.1, 0.1, 0.1, 0.1, 0.05};
    ndt_2d_hip::ParticleFilterHip pf(10, n, alphas, matcher, head[3]);
    pf.initGlobal(map.data(), width, height, geo[0], geo[1], geo[2]);
    std::uint64_t count = pf.size();
    std::fwrite(&count, 8, 1, out);
    dump(out, pf);
    const std::uint64_t replaced = pf.inject(geo[3]);
    std::fwrite(&replaced, 8, 1, out);
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
      pf.initGlobal(resident, 300);
      const std::uint64_t dims[2] = {result.info.width, result.info.height};
      const double g[3] = {result.info.origin_x, result.info.origin_y, result.info.resolution};
      std::fwrite(dims, 8, 2, out);
      std::fwrite(g, 8, 3, out);
      count = pf.size();
      std::fwrite(&count, 8, 1, out);
      dump(out, pf);
      // the map those particles must lie in, as the host reads it
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
