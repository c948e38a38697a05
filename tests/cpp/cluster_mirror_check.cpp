// C++ consumer of ParticleFilterHip::clusters / bestCluster (ndt_2d_amd/plugin/particle_filter_hip.hpp):
// no Python and no torch in this process.  Reads a map and the call's parameters from argv[1], runs
// initGlobal on the host map (a seeded set: many clusters) and init round a pose (one blob), and
// writes the particles, the weights and what clusters() and bestCluster() reported for each set to
// argv[2]; tests/test_gpu_cluster_mirror.py compares them with the restatement.
//   in:  u64 width, height, n, seed; f64 origin_x, origin_y, resolution, unused; i8 map[height * width]
//   out: twice (the seeded set with clusters(4), the blob with clusters()):
//        u64 n; f64 particles[n][3]; f64 weights[n]
//        u64 header n, n_left_out, n_bins, n_clusters, rounds; f64 w_total
//        u64 n_records; per record: u64 label, count; f64 mass, weight, mean_x, mean_y, mean_theta,
//                                   cxx, cxy, cyy, var_theta
//        u64 have_best; f64 mean[3], covariance[9], share; u64 label, count
//        f64 getMean[3]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "particle_filter_hip.hpp"

namespace
{

bool read(std::FILE * f, void * p, std::size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

void u64(std::FILE * f, std::uint64_t v) { std::fwrite(&v, 8, 1, f); }
void f64(std::FILE * f, const double * v, std::size_t n) { std::fwrite(v, 8, n, f); }

void dump(std::FILE * f, ndt_2d_hip::ParticleFilterHip & pf, int max_clusters)
{
  const std::vector<double> p = pf.particles(), w = pf.weights();
  u64(f, pf.size());
  f64(f, p.data(), p.size());
  f64(f, w.data(), w.size());
  // (a copy: bestCluster's own call replaces the records)
  const std::vector<ndt2d_cluster_record> found = max_clusters > 0 ? pf.clusters(max_clusters) : pf.clusters();
  const ndt2d_cluster_header h = pf.clusterHeader();
  u64(f, h.n);
  u64(f, h.n_left_out);
  u64(f, h.n_bins);
  u64(f, h.n_clusters);
  u64(f, h.rounds);
  f64(f, &h.w_total, 1);
  u64(f, found.size());
  for (const ndt2d_cluster_record & r : found)
  {
    u64(f, r.label);
    u64(f, r.count);
    const double v[9] = {r.mass, r.weight, r.mean_x, r.mean_y, r.mean_theta, r.cxx, r.cxy, r.cyy, r.var_theta};
    f64(f, v, 9);
  }
  ndt_2d_hip::PoseClusterHip best;
  u64(f, pf.bestCluster(&best) ? 1 : 0);
  f64(f, best.mean, 3);
  f64(f, best.covariance, 9);
  f64(f, &best.share, 1);
  u64(f, best.label);
  u64(f, best.count);
  double mean[3];
  pf.getMean(mean);
  f64(f, mean, 3);
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
    dump(out, pf, 4);
    pf.init(1.3, -0.4, 3.1, 0.1, 0.1, 0.05);
    dump(out, pf, 0);
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
