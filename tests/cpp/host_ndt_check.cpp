// The host NDT build in REUSED storage (ndt_2d_amd/csrc/host/ndt2d_host_ndt.h), as a matcher drives it:
// one HostNdt object taken through a sequence of maps of different geometry -- build_ndt(...,
// reuse = the NDT before) -- and then reset_cells + load6 of a packed grid, the way a grid built on
// the device is fetched back.  Built from ndt2d_host_ndt.cpp alone with the address and
// undefined-behaviour sanitizers (tests/test_host_logic.py): a stale size, stamp or touched list in
// the reused pool is a memory error here.  Every build's inputs and cells are written to argv[1];
// the test rebuilds the same inputs in fresh storage (ndt2d_host_build_grid_ex) and compares bytes.
//
// The file, little endian, a sequence of records:
//   "BUILD": u64 1, u64 sequential, f64 resolution, f64 range_max, u64 n_scans, f64 poses[3 n_scans],
//            u64 offsets[n_scans + 1], f64 points[2 offsets[n_scans]], u64 sx, u64 sy, f64 ox, f64 oy,
//            f64 cells6[6 sx sy]
//   "LOAD":  u64 2, u64 sx, u64 sy, u64 n_touched, u64 index[n_touched], f64 sparse6[6 n_touched],
//            f64 packed6[6 sx sy]      (the grid loaded: the cells6 of the BUILD record before it)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "host/ndt2d_host_ndt.h"

using ndt2d::host::HostNdt;

namespace
{

// SplitMix64: a fixed integer generator, the same values on every machine
struct Rng
{
  uint64_t s;
  uint64_t next()
  {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uniform() { return static_cast<double>(next() >> 11) * (1.0 / 9007199254740992.0); }
  double between(double lo, double hi) { return lo + (hi - lo) * uniform(); }
};

struct Map
{
  double resolution, range_max;
  std::vector<double> poses, points;
  std::vector<size_t> offsets{0};
  void add(double x, double y, double theta, const std::vector<double> & pts)
  {
    poses.insert(poses.end(), {x, y, theta});
    points.insert(points.end(), pts.begin(), pts.end());
    offsets.push_back(points.size() / 2);
  }
};

// n beams around the full circle, ranges up to `reach`
std::vector<double> ring(Rng & rng, size_t n, double reach)
{
  std::vector<double> pts(2 * n);
  for (size_t k = 0; k < n; ++k)
  {
    const double ang = -M_PI + 2.0 * M_PI * static_cast<double>(k) / static_cast<double>(n);
    const double r = rng.between(0.0, reach);
    pts[2 * k] = r * std::cos(ang);
    pts[2 * k + 1] = r * std::sin(ang);
  }
  return pts;
}

// points off the grid -- NaN, +-inf, 1e300 -- at the first beam, the last, about every quarter
// boundary and where the n % 4 tail begins
void put_off_grid(std::vector<double> & pts)
{
  const size_t n = pts.size() / 2, q = n / 4;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double bad[8][2] = {{nan, 0.5}, {inf, 0.0}, {0.25, -inf}, {1e300, 1e300}, {-1e300, 0.0}, {nan, nan}, {-inf, inf}, {0.0, 1e300}};
  const size_t at[8] = {0, n - 1, q - 1, q, 2 * q, 3 * q - 1, 3 * q, 4 * q < n ? 4 * q : n - 1};
  for (size_t i = 0; i < 8; ++i)
  {
    pts[2 * at[i]] = bad[i][0];
    pts[2 * at[i] + 1] = bad[i][1];
  }
}

// A map whose scan poses span +-spread_x, +-spread_y exactly: empty scans, scans of 1, 5, 31, 33 and
// 719 beams (below the quarter cut, just above it, with and without a tail), off-grid points in
// two of them, and one scan whose beams all fall in one cell.
Map make_map(Rng & rng, double resolution, double range_max, double spread_x, double spread_y, double reach)
{
  Map m;
  m.resolution = resolution;
  m.range_max = range_max;
  const size_t beams[] = {0, 719, 1, 33, 5, 0, 31, 719, 33};
  size_t i = 0;
  for (const size_t n : beams)
  {
    std::vector<double> pts = ring(rng, n, reach);
    if (i == 7 || i == 8) put_off_grid(pts);
    // (the first two poses pin the extent)
    const double x = i == 0 ? -spread_x : (i == 1 ? spread_x : rng.between(-spread_x, spread_x));
    const double y = i == 0 ? -spread_y : (i == 1 ? spread_y : rng.between(-spread_y, spread_y));
    m.add(x, y, rng.between(-M_PI, M_PI), pts);
    ++i;
  }
  std::vector<double> one_cell(2 * 64);
  for (size_t j = 0; j < 64; ++j)
  {
    one_cell[2 * j] = resolution * (0.3 + 1e-4 * static_cast<double>(j));
    one_cell[2 * j + 1] = resolution * (0.4 - 1e-4 * static_cast<double>(j));
  }
  m.add(0.0, 0.0, 0.0, one_cell);
  return m;
}

void put(std::FILE * f, const void * p, size_t bytes)
{
  if (bytes > 0 && std::fwrite(p, 1, bytes, f) != bytes) std::abort();
}
void put_u64(std::FILE * f, uint64_t v) { put(f, &v, sizeof(v)); }
void put_f64(std::FILE * f, double v) { put(f, &v, sizeof(v)); }

}  // namespace

int main(int argc, char ** argv)
{
  if (argc != 2) return 2;
  std::FILE * f = std::fopen(argv[1], "wb");
  if (f == nullptr) return 2;
  Rng rng{2024};
  // 41 x 41; larger (81 x 81); smaller, a cell size that is no power of two (the true divide of
  // getIndex); a 1 x 11 sliver; the first geometry again
  const Map maps[] = {make_map(rng, 0.25, 4.75, 0.25, 0.25, 6.0), make_map(rng, 0.25, 9.0, 1.0, 1.0, 12.0),
                      make_map(rng, 0.3, 2.4, 0.6, 0.6, 3.0), make_map(rng, 4.0, 1.0, 0.0, 20.0, 3.0),
                      make_map(rng, 0.25, 4.75, 0.25, 0.25, 0.3)};
  std::unique_ptr<HostNdt> ndt;   // the ONE object every build below fills
  std::vector<double> cells, grid;   // grid: the third map's cells, loaded back at the end
  double grid_cs = 0.0, grid_ox = 0.0, grid_oy = 0.0;
  size_t grid_sx = 0, grid_sy = 0;
  size_t n_builds = 0;
  for (const Map & m : maps)
  {
    for (int sequential = 0; sequential < 2; ++sequential)
    {
      const size_t n_scans = m.offsets.size() - 1;
      ndt = ndt2d::host::build_ndt(m.resolution, m.range_max, m.poses.data(), m.points.data(), m.offsets.data(), n_scans,
                                   std::move(ndt), ndt2d::kEigenFormSchur, sequential == 0);
      if (!ndt) return 3;
      cells.assign(6 * ndt->ncell(), -1.0);
      ndt->pack6(cells.data());
      put_u64(f, 1);
      put_u64(f, static_cast<uint64_t>(sequential));
      put_f64(f, m.resolution);
      put_f64(f, m.range_max);
      put_u64(f, n_scans);
      put(f, m.poses.data(), m.poses.size() * sizeof(double));
      for (const size_t o : m.offsets) put_u64(f, o);
      put(f, m.points.data(), m.points.size() * sizeof(double));
      put_u64(f, ndt->size_x());
      put_u64(f, ndt->size_y());
      put_f64(f, ndt->origin_x());
      put_f64(f, ndt->origin_y());
      put(f, cells.data(), cells.size() * sizeof(double));
      ++n_builds;
      if (&m == &maps[2])
      {
        grid = cells;
        grid_cs = ndt->cell_size(), grid_ox = ndt->origin_x(), grid_oy = ndt->origin_y();
        grid_sx = ndt->size_x(), grid_sy = ndt->size_y();
      }
    }
  }
  // a packed grid loaded into the same object (host_ndt() of the matcher: reset_cells + load6), of
  // another size than the build before it left: the third map's over what the fifth touched
  {
    const size_t sx = grid_sx, sy = grid_sy;
    ndt->reset_cells(grid_cs, sx, sy, grid_ox, grid_oy);
    ndt->load6(grid.data());
    std::vector<uint32_t> index(ndt->n_touched());
    std::vector<double> sparse(6 * ndt->n_touched()), packed(6 * ndt->ncell(), -1.0);
    ndt->sparse6(index.data(), sparse.data());
    ndt->pack6(packed.data());
    put_u64(f, 2);
    put_u64(f, sx);
    put_u64(f, sy);
    put_u64(f, index.size());
    for (const uint32_t i : index) put_u64(f, i);
    put(f, sparse.data(), sparse.size() * sizeof(double));
    put(f, packed.data(), packed.size() * sizeof(double));
  }
  if (std::fclose(f) != 0) return 2;
  std::printf("host ndt ok: %zu builds in one object\n", n_builds);
  return 0;
}
