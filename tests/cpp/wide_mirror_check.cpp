// WideSearchHip::matchWide (ndt_2d_amd/plugin/wide_search_hip.hpp) driven from a plain C++ program
// (built and run by tests/test_gpu_wide.py): a matcher of its own, the map scans and the query of
// the input file, two calls (the second keeps the bound image), the results to the output file.
//   in:  u64 n_scans, n_points (all scans), n_query | f64 ndt_resolution, range_max, linear_size,
//        linear_res, angular_size, angular_res, query pose[3] | u64 offsets[n_scans + 1] |
//        f64 poses[n_scans][3] | f64 points[n_points][2] | f64 query[n_query][2]
//   out: per call  f64 score, correction[3], pose[3] | u64 best_index, near_tie, has_winner,
//        tiles_scored, tiles_total
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wide_search_hip.hpp"

int main(int argc, char ** argv)
{
  if (argc != 3) return 2;
  std::FILE * in = std::fopen(argv[1], "rb");
  if (in == nullptr) return 3;
  uint64_t counts[3];
  double params[9];
  if (std::fread(counts, sizeof(uint64_t), 3, in) != 3 || std::fread(params, sizeof(double), 9, in) != 9) return 4;
  std::vector<uint64_t> offsets64(counts[0] + 1);
  std::vector<double> poses(3 * counts[0]), points(2 * counts[1]), query(2 * counts[2]);
  if (std::fread(offsets64.data(), sizeof(uint64_t), offsets64.size(), in) != offsets64.size()) return 4;
  if (std::fread(poses.data(), sizeof(double), poses.size(), in) != poses.size()) return 4;
  if (std::fread(points.data(), sizeof(double), points.size(), in) != points.size()) return 4;
  if (std::fread(query.data(), sizeof(double), query.size(), in) != query.size()) return 4;
  std::fclose(in);
  const std::vector<size_t> offsets(offsets64.begin(), offsets64.end());

  ndt2d_matcher * m = nullptr;
  if (ndt2d_matcher_create(&m, 0) != NDT2D_OK) return 5;
  int status = 0;
  std::FILE * out = std::fopen(argv[2], "wb");
  if (out == nullptr) status = 6;
  // (the matcher's own lattice is the plugin's default: the wide search brings its own)
  if (status == 0 && ndt2d_matcher_initialize(m, params[0], 0.0025, 0.1, 0.005, 0.05, 100, params[1]) != NDT2D_OK) status = 7;
  if (status == 0 && ndt2d_matcher_add_scans(m, poses.data(), points.data(), offsets.data(), counts[0]) != NDT2D_OK) status = 8;
  ndt_2d_hip::WideSearchHip wide(m);
  for (int call = 0; call < 2 && status == 0; ++call)
  {
    ndt_2d_hip::WideMatch r;
    if (!wide.matchWide(params + 6, query.data(), counts[2], params[2], params[3], params[4], params[5], r, 2))
    {
      std::fprintf(stderr, "%s\n", wide.last_error().c_str());
      status = 9;
      break;
    }
    const double d[7] = {r.score, r.correction[0], r.correction[1], r.correction[2], r.pose[0], r.pose[1], r.pose[2]};
    const uint64_t u[5] = {r.best_index, r.near_tie ? 1u : 0u, r.has_winner ? 1u : 0u, r.tiles_scored, r.tiles_total};
    std::fwrite(d, sizeof(double), 7, out);
    std::fwrite(u, sizeof(uint64_t), 5, out);
  }
  if (out != nullptr) std::fclose(out);
  ndt2d_matcher_destroy(m);
  return status;
}
