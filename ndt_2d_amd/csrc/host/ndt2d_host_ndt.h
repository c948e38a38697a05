// The host NDT of libndt2d_hip.so: HostNdt, the NDT build of ScanMatcherNDT::addScans on the host
// with the reference's incremental formulas and point order (it produces the kernels' input and
// must be bit-faithful), the visited offsets of the search lattice and the
// subsampling of a scan.  Knows nothing of the matcher and calls no device function: ndt2d_host_ndt.cpp
// compiles into a stand-alone program (tests/cpp/host_ndt_check.cpp).
#ifndef NDT2D_HOST_NDT_H_
#define NDT2D_HOST_NDT_H_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "ndt2d_eigen2.h"

// (what crosses the library's translation units stays out of its dynamic symbol table)
#pragma GCC visibility push(hidden)
namespace ndt2d
{
namespace host
{

// cos(t) and sin(t) of one argument, as a GCC-built reference gets them: wherever
// the reference writes the pair, GCC merges the two calls into one glibc sincos(),
// whose sine can differ from sin()'s in the last ulp (t = 0.4710119964311561).
// (Same helper as in ndt2d_kernels.h; this file stays free of HIP headers.)
inline void ndt2d_cos_sin(double t, double * c, double * s)
{
  sincos(t, s, c);
}

// One NDT cell; fields as ndt_2d::Cell (reference include/ndt_2d/ndt_model.hpp:43-65).
// Symmetric 2x2 matrices keep {xx, xy, yy}; correlation(1,0) is never written
// by the reference and never read.
struct HostCell
{
  bool valid = false;
  double n = 0.0;
  double mean_x = 0.0, mean_y = 0.0;
  double corr_xx = 0.0, corr_xy = 0.0, corr_yy = 0.0;
  double cov_xx = 0.0, cov_xy = 0.0, cov_yy = 0.0;
  double info_xx = 0.0, info_xy = 0.0, info_yy = 0.0;

  // Cell::addPoint, reference src/ndt_model.cpp:50-63.  The five running values are
  // consecutive doubles updated by one expression shape, (v * n + t) / n1: the AVX2
  // clone of NDT::addScan below does them as packed operations (each lane the same
  // IEEE operation as the scalar code, so the results are bit-identical).
  __attribute__((always_inline)) void add(double x, double y)
  {
    typedef double v4d __attribute__((vector_size(32)));
    const double n1 = n + 1;
    v4d v;
    std::memcpy(&v, &mean_x, sizeof(v));             // mean_x, mean_y, corr_xx, corr_xy
    const v4d t = {x, y, x * x, x * y};
    v = (v * n + t) / n1;
    std::memcpy(&mean_x, &v, sizeof(v));
    corr_yy = (corr_yy * n + y * y) / n1;
    n += 1;
    valid = false;
  }

  // Cell::compute, reference src/ndt_model.cpp:65-103.  eigen_form: how the eigenvalues of
  // :84-85 are formed (ndt2d_eigen2.h: Eigen 3.4.0's EigenSolver transcribed, or the closed form).
  void compute(int eigen_form);
};

// class NDT (reference include/ndt_2d/ndt_model.hpp:67-134), build side only.
class HostNdt
{
public:
  // NDT::NDT, reference src/ndt_model.cpp:118-126
  HostNdt(double cell_size, double size_x, double size_y, double origin_x, double origin_y)
  {
    reset(cell_size, size_x, size_y, origin_x, origin_y);
  }

  // A new, empty NDT in this object's storage: the mapper rebuilds its local NDT for
  // every scan (src/ndt_mapper.cpp:508-509) with the same geometry more often than not,
  // and of its cells only the few hundred that received points need clearing.
  void reset(double cell_size, double size_x, double size_y, double origin_x, double origin_y)
  {
    reset_cells(cell_size, static_cast<size_t>((size_x / cell_size) + 1), static_cast<size_t>((size_y / cell_size) + 1),
                origin_x, origin_y);
  }

  // ... given its size in cells
  void reset_cells(double cell_size, size_t sx, size_t sy, double origin_x, double origin_y);

  // NDT::getIndex, reference src/ndt_model.cpp:203-218, with the off-grid rule of
  // include/ndt2d_hip.h: the four comparisons on the double quotients, before any integer cast
  // (for f >= 0, trunc(f) < size <=> f < size; NaN, +-inf and points 2^32 cells away are outside)
  __attribute__((always_inline)) long index(double x, double y) const
  {
    // (written with ordered compares only, `a < b`: a NaN falls through the first test and fails
    // the second -- no extra branch on the unordered flag)
    if (x < origin_x_ || y < origin_y_) return -1;
    // (a power-of-two cell size: multiplying by its exact reciprocal is the correctly
    // rounded quotient, bit-identical to the reference's divide)
    const double fx = pow2_ ? (x - origin_x_) * inv_cell_size_ : (x - origin_x_) / cell_size_;
    const double fy = pow2_ ? (y - origin_y_) * inv_cell_size_ : (y - origin_y_) / cell_size_;
    if (fx < fsize_x_ && fy < fsize_y_)
      return static_cast<long>(static_cast<unsigned int>(fy) * size_x_ + static_cast<unsigned int>(fx));
    return -1;
  }

  // NDT::addScan, reference src/ndt_model.cpp:132-152.
  //
  // Cell::addPoint is a recurrence -- v = (v * n + t) / (n + 1) on five running values -- and
  // consecutive beams of a scan fall into the same cell more often than not: one dependent chain
  // of multiply, add, DIVIDE and a store-to-load round trip per point (~20 cycles; the whole of
  // addScans' host time, 4.3 ns per point on the GPU box's EPYC 9575F).  Round 6: a scan is cut
  // into four quarters of consecutive beams and the quarters advance side by side -- four chains
  // in flight, and the four corr_yy updates of a step share ONE packed divide (five 256-bit
  // divides per four points instead of eight divide operations).  A cell's values depend on the
  // ORDER of its points (the reference's: scan after scan, beam after beam): pass 1 transforms the
  // points and looks their cells up (branch-free, vectorised by the compiler), then stamps every
  // cell with the first quarter of the scan that reaches it; the points of a LATER quarter in
  // such a cell (the cell a quarter boundary falls into; a robot boxed in closer than a cell) are
  // taken out of their quarter and added behind the quarters, in beam order.  So every cell
  // still receives its points in the reference's order, and every lane of a packed operation is
  // the IEEE operation of the scalar code: bit-identical cells (tests/test_host_logic.py, and
  // every host-build == oracle test).  Points outside the grid go to a scratch cell behind it.
  // (defined in ndt2d_host_ndt.cpp: the AVX2 clone of the loop exists once)
  void add_scan(double pose_x, double pose_y, double pose_theta, const double * pts, size_t n);

  // (tests: the sequential order for every scan -- the two must agree bit for bit)
  void set_interleave(bool on) { interleave_ = on; }
  void set_side_by_side_max_bytes(size_t bytes) { side_by_side_max_bytes_ = bytes; }   // (experiments)

  // NDT::likelihood(Vector2d) (reference src/ndt_model.cpp:162-170) with Cell::score (:105-116)
  // inlined: exp(((-0.5 * q^T) * information) * q) in that order, libm's exp.  Used by the
  // single-pose calls (scorePoints once per particle, src/particle_filter.cpp:81-87) and by the
  // adjudication of near-ties -- never by a search or a batch.
  __attribute__((always_inline)) double likelihood(double x, double y) const
  {
    const long i = index(x, y);
    if (i < 0) return 0.0;
    const HostCell & c = cells_[static_cast<size_t>(i)];
    if (c.n < 5) return 0.0;
    const double q0 = x - c.mean_x, q1 = y - c.mean_y;
    const double a0 = -0.5 * q0, a1 = -0.5 * q1;
    const double r0 = a0 * c.info_xx + a1 * c.info_xy;
    const double r1 = a0 * c.info_xy + a1 * c.info_yy;
    return std::exp(r0 * q0 + r1 * q1);
  }

  // A grid from its packed records (a grid that was built on the device, fetched back once).
  void load6(const double * cells6);

  // NDT::compute, reference src/ndt_model.cpp:154-160 (a cell without points returns
  // at once there: only the cells that received points are visited here)
  void compute(int eigen_form);

  // The cells that hold points, as ndt2d_set_grid_sparse takes them.
  size_t n_touched() const { return touched_.size(); }
  void sparse6(uint32_t * index, double * cells6) const;

  void pack6(double * out) const;

  double cell_size() const { return cell_size_; }
  size_t size_x() const { return size_x_; }
  size_t size_y() const { return size_y_; }
  double origin_x() const { return origin_x_; }
  double origin_y() const { return origin_y_; }
  size_t ncell() const { return n_cells_; }

private:
  // add_scan's body, and the copy of it compiled for AVX2 (x86-64: taken where the processor has it)
  __attribute__((always_inline)) void add_scan_body(double pose_x, double pose_y, double pose_theta, const double * pts, size_t n);
  void add_scan_avx2(double pose_x, double pose_y, double pose_theta, const double * pts, size_t n);

  double cell_size_ = 0.0, inv_cell_size_ = 0.0;
  bool pow2_ = false;
  size_t size_x_ = 0, size_y_ = 0;
  double fsize_x_ = 0.0, fsize_y_ = 0.0;   // (the sizes as index() compares them)
  double origin_x_ = 0.0, origin_y_ = 0.0;
  std::vector<HostCell> cells_;     // a pool: the first n_cells_ are the grid
  size_t n_cells_ = 0;
  std::vector<uint32_t> touched_;   // cells that hold at least one point
  // add_scan: world points and cell indices of the scan being added; per-cell stamp = the
  // (scan, quarter) that last reached the cell (ids from a running counter: never cleared)
  std::vector<double> scan_xy_;
  std::vector<int32_t> scan_idx_;
  std::vector<uint32_t> stamp_;
  std::vector<uint32_t> late_;      // beams of the scan that are added after the quarters ...
  std::vector<int32_t> late_cell_;  // ... and their cells
  uint32_t epoch_ = 0;
  bool interleave_ = true;
  size_t side_by_side_max_bytes_ = 1u << 20;
};

// ScanMatcherNDT::addScans' extent + NDT build, reference src/scan_matcher_ndt.cpp:49-74.
// max_x_/max_y_ start at numeric_limits<double>::min(), as the reference has it.
std::unique_ptr<HostNdt> build_ndt(double resolution, double range_max, const double * poses,
                                   const double * pts, const size_t * offsets, size_t n_scans,
                                   std::unique_ptr<HostNdt> reuse = nullptr, int eigen_form = ndt2d::kEigenFormSchur,
                                   bool side_by_side = true);

// The reference's `for (v = -size; v < size; v += res)` (src/scan_matcher_ndt.cpp:103,117,119):
// the visited values come from repeated floating-point addition.
std::vector<double> search_offsets(double size, double res);

// Whether search_offsets(size, res) ends and stays within `limit` values.
bool offsets_fit(double size, double res, size_t limit);

// The off-grid rule (include/ndt2d_hip.h) for matchLaserScan's ranges: `ranges` itself, or a copy in
// `scratch` with the kept infinities made finite (ndt2d_host_ndt.cpp).
const float * off_grid_ranges(std::vector<float> & scratch, const float * ranges, size_t n_ranges,
                              double range_max);

// Subsampling of matchScan / scorePoints, reference src/scan_matcher_ndt.cpp:95-96,110.
// (a beam the off-grid rule covers leaves as (-1e300, -1e300): ndt2d_host_ndt.cpp)
void subsample_into(std::vector<double> & out, const double * pts, size_t n_points,
                    size_t laser_max_beams);

}  // namespace host
}  // namespace ndt2d
#pragma GCC visibility pop

#endif  // NDT2D_HOST_NDT_H_
