// ndt2d_host_ndt.h: the host NDT build, the search lattice's offsets, the subsampling -- and the three
// entry points that need nothing else (ndt2d_host_build_grid, _ex, ndt2d_search_offsets).
#include "host/ndt2d_host_ndt.h"

#include <algorithm>
#include <cfloat>
#include <limits>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"

namespace ndt2d
{
namespace host
{

// Cell::compute, reference src/ndt_model.cpp:65-103
void HostCell::compute(int eigen_form)
{
  if (valid || n < 3) return;
  const double scale = n / (n - 1);
  cov_xx = (corr_xx - (mean_x * mean_x)) * scale;
  cov_xy = (corr_xy - (mean_x * mean_y)) * scale;
  cov_yy = (corr_yy - (mean_y * mean_y)) * scale;

  // (the eigenvalues decide the branch and feed the clamp's determinant: a covariance far from
  // the threshold does not need them, ndt2d_eigen2.h clamp_test_surely_false)
  double small = 1.0, large = 1.0;
  if (!ndt2d::clamp_test_surely_false(cov_xx, cov_xy, cov_yy))
  {
    ndt2d::covariance_eigenvalues(eigen_form, cov_xx, cov_xy, cov_yy, &small, &large);
    if (small > large) std::swap(small, large);
  }
  if (small < 0.001 * large)
  {
    // eigenvalue clamp (:88-96)
    const double determinant = (0.001 * large) * large;
    info_xx = cov_yy / determinant;
    info_xy = -cov_xy / determinant;
    info_yy = cov_xx / determinant;
  }
  else
  {
    // Matrix2d::inverse() (:99): adjugate times 1/det
    const double det = cov_xx * cov_yy - cov_xy * cov_xy;
    const double invdet = 1.0 / det;
    info_xx = cov_yy * invdet;
    info_xy = -cov_xy * invdet;
    info_yy = cov_xx * invdet;
  }
  valid = true;
}

void HostNdt::reset_cells(double cell_size, size_t sx, size_t sy, double origin_x, double origin_y)
{
  // The storage is a pool of cells of which only the touched ones are not in their initial
  // state: clearing those makes it an empty grid of ANY geometry that fits (the extent
  // follows the scan poses, so its size changes by a cell now and then; a real lidar's
  // grid is tens of thousands of cells, 6 MB, of which a scan touches a thousand).
  for (const uint32_t i : touched_) cells_[i] = HostCell();
  if (cells_.size() < sx * sy + 1) cells_.resize(sx * sy + 1);   // (+ 1: add_scan's scratch cell)
  n_cells_ = sx * sy;
  touched_.clear();
  {
    int e = 0;
    pow2_ = cell_size > 0.0 && std::isfinite(cell_size) && std::frexp(cell_size, &e) == 0.5 &&
            std::fpclassify(cell_size) == FP_NORMAL && std::fpclassify(1.0 / cell_size) == FP_NORMAL;
    inv_cell_size_ = 1.0 / cell_size;
  }
  cell_size_ = cell_size;
  size_x_ = sx;
  size_y_ = sy;
  fsize_x_ = static_cast<double>(sx);
  fsize_y_ = static_cast<double>(sy);
  origin_x_ = origin_x;
  origin_y_ = origin_y;
}

// NDT::addScan, reference src/ndt_model.cpp:132-152 (the order of the points: ndt2d_host_ndt.h)
inline void HostNdt::add_scan_body(double pose_x, double pose_y, double pose_theta, const double * pts, size_t n)
{
  typedef double v4d __attribute__((vector_size(32)));
  double cos_th, sin_th;
  ndt2d_cos_sin(pose_theta, &cos_th, &sin_th);  // :135-136
  const size_t quarter = n / 4;
  // (shorter scans: nothing to gain.  Nor on a grid whose cells do not stay in the host's L2:
  // there the sequential loop's cache misses overlap by themselves and the stamps only add
  // to them -- GPU box's EPYC 9575F, nine 720-beam scans: 41 x 41 cells 24.3 -> 20.8 us side by
  // side, 245 x 245 cells 17.3 -> 20.5 us)
  const bool side_by_side = quarter >= 8 && interleave_ && n_cells_ * sizeof(HostCell) <= side_by_side_max_bytes_;
  if (!side_by_side)
  {
    // the reference's loop as it stands
    for (size_t k = 0; k < n; ++k)
    {
      const double px = pts[2 * k], py = pts[2 * k + 1];
      double wx = pose_x;
      double wy = pose_y;
      wx += px * cos_th - py * sin_th;
      wy += px * sin_th + py * cos_th;
      const long i = index(wx, wy);
      if (i >= 0)
      {
        HostCell & c = cells_[static_cast<size_t>(i)];
        if (c.n == 0.0) touched_.push_back(static_cast<uint32_t>(i));
        c.add(wx, wy);
      }
    }
    return;
  }
  if (scan_idx_.size() < n)
  {
    scan_idx_.resize(n);
    scan_xy_.resize(2 * n);
  }
  if (cells_.size() < n_cells_ + 1) cells_.resize(n_cells_ + 1);
  if (stamp_.size() < cells_.size()) stamp_.resize(cells_.size(), 0u);
  if (epoch_ > 0xfffffff0u)
  {
    std::fill(stamp_.begin(), stamp_.end(), 0u);
    epoch_ = 0;
  }
  const uint32_t scan_first = epoch_ + 1;
  epoch_ += 4;
  int32_t * const idx = scan_idx_.data();
  double * const xy = scan_xy_.data();
  const int32_t outside = static_cast<int32_t>(n_cells_);   // the scratch cell
  // pass 1a: points_world (:138-143) and NDT::getIndex (:203-218).  For a point that passed
  // `x >= origin`, trunc(f) < size  <=>  f < size, so the four comparisons are getIndex's.
  // (Everything the loop reads of *this is copied out first: its stores could alias members.)
  {
    const double ox = origin_x_, oy = origin_y_, inv = inv_cell_size_, cs = cell_size_;
    const double fsx = static_cast<double>(size_x_), fsy = static_cast<double>(size_y_);
    const int32_t sx = static_cast<int32_t>(size_x_);
    if (pow2_)
    {
      for (size_t k = 0; k < n; ++k)
      {
        const double px = pts[2 * k], py = pts[2 * k + 1];
        double wx = pose_x;
        double wy = pose_y;
        wx += px * cos_th - py * sin_th;
        wy += px * sin_th + py * cos_th;
        xy[2 * k] = wx;
        xy[2 * k + 1] = wy;
        const double fx = (wx - ox) * inv, fy = (wy - oy) * inv;   // (exact reciprocal: == the divide)
        const bool in = (wx >= ox) & (wy >= oy) & (fx < fsx) & (fy < fsy);
        const int32_t gx = static_cast<int32_t>(in ? fx : 0.0), gy = static_cast<int32_t>(in ? fy : 0.0);
        idx[k] = in ? gy * sx + gx : outside;
      }
    }
    else
    {
      for (size_t k = 0; k < n; ++k)
      {
        const double px = pts[2 * k], py = pts[2 * k + 1];
        double wx = pose_x;
        double wy = pose_y;
        wx += px * cos_th - py * sin_th;
        wy += px * sin_th + py * cos_th;
        xy[2 * k] = wx;
        xy[2 * k + 1] = wy;
        const double fx = (wx - ox) / cs, fy = (wy - oy) / cs;
        const bool in = (wx >= ox) & (wy >= oy) & (fx < fsx) & (fy < fsy);
        const int32_t gx = static_cast<int32_t>(in ? fx : 0.0), gy = static_cast<int32_t>(in ? fy : 0.0);
        idx[k] = in ? gy * sx + gx : outside;
      }
    }
  }
  // pass 1b: first touches (in beam order: `touched_` keeps the order the sequential loop gave
  // it) and the quarter stamps.  A point whose cell an EARLIER quarter of this scan has reached
  // (the cell a quarter boundary falls into, mostly) leaves its quarter: it is added after the
  // quarters, in beam order -- every point of that cell from the later quarter does, so the
  // cell still sees its points in the reference's order.  The n % 4 beams behind the fourth
  // quarter go the same way.
  // (Written with selects instead of branches -- stamp, first touch and late list stored for every
  // point -- the loop is SLOWER: EPYC 9575F, toy map 19.4 -> 26.8 us per addScans; consecutive beams
  // share cells, and a stamp stored for every point is a store-to-load chain through that cell.)
  size_t n_late = 0;
  {
    const size_t n_touched_before = touched_.size();
    touched_.resize(n_touched_before + n);
    if (late_.size() < n) late_.resize(n);
    uint32_t * touched_out = touched_.data() + n_touched_before;
    uint32_t * const stamp = stamp_.data();
    uint32_t * const late = late_.data();
    const HostCell * const cells = cells_.data();
    for (size_t part = 0; part < 4; ++part)
    {
      const size_t k_end = part == 3 ? n : (part + 1) * quarter;
      const uint32_t mine = scan_first + static_cast<uint32_t>(part);
      for (size_t k = part * quarter; k < k_end; ++k)
      {
        const int32_t i = idx[k];
        if (i == outside) continue;
        const uint32_t seen = stamp[i];
        if (seen < scan_first)
        {
          stamp[i] = mine;
          *touched_out = static_cast<uint32_t>(i);
          touched_out += cells[i].n == 0.0 ? 1 : 0;
        }
        if ((seen >= scan_first && seen != mine) || k >= 4 * quarter)
        {
          late[n_late++] = static_cast<uint32_t>(k);
        }
      }
    }
    touched_.resize(static_cast<size_t>(touched_out - touched_.data()));
  }
  // pass 2: Cell::addPoint (:50-63)
  HostCell * const cells = cells_.data();
  {
    const size_t q = quarter;
    // (the late points step aside: their quarter adds to the scratch cell in their place)
    if (late_cell_.size() < n_late) late_cell_.resize(n_late);
    for (size_t l = 0; l < n_late; ++l)
    {
      const uint32_t k = late_[l];
      late_cell_[l] = idx[k];
      idx[k] = outside;
    }
    for (size_t j = 0; j < q; ++j)
    {
      HostCell & c0 = cells[idx[j]];
      HostCell & c1 = cells[idx[j + q]];
      HostCell & c2 = cells[idx[j + 2 * q]];
      HostCell & c3 = cells[idx[j + 3 * q]];
      const double x0 = xy[2 * j], y0 = xy[2 * j + 1];
      const double x1 = xy[2 * (j + q)], y1 = xy[2 * (j + q) + 1];
      const double x2 = xy[2 * (j + 2 * q)], y2 = xy[2 * (j + 2 * q) + 1];
      const double x3 = xy[2 * (j + 3 * q)], y3 = xy[2 * (j + 3 * q) + 1];
      const v4d nn = {c0.n, c1.n, c2.n, c3.n};
      const v4d n1 = nn + 1.0;
      v4d yy = {c0.corr_yy, c1.corr_yy, c2.corr_yy, c3.corr_yy};
      const v4d ty = {y0 * y0, y1 * y1, y2 * y2, y3 * y3};
      yy = (yy * nn + ty) / n1;
      v4d v0, v1, v2, v3;
      std::memcpy(&v0, &c0.mean_x, sizeof(v4d));     // mean_x, mean_y, corr_xx, corr_xy
      std::memcpy(&v1, &c1.mean_x, sizeof(v4d));
      std::memcpy(&v2, &c2.mean_x, sizeof(v4d));
      std::memcpy(&v3, &c3.mean_x, sizeof(v4d));
      const v4d t0 = {x0, y0, x0 * x0, x0 * y0}, t1 = {x1, y1, x1 * x1, x1 * y1};
      const v4d t2 = {x2, y2, x2 * x2, x2 * y2}, t3 = {x3, y3, x3 * x3, x3 * y3};
      v0 = (v0 * nn[0] + t0) / n1[0];
      v1 = (v1 * nn[1] + t1) / n1[1];
      v2 = (v2 * nn[2] + t2) / n1[2];
      v3 = (v3 * nn[3] + t3) / n1[3];
      std::memcpy(&c0.mean_x, &v0, sizeof(v4d));
      std::memcpy(&c1.mean_x, &v1, sizeof(v4d));
      std::memcpy(&c2.mean_x, &v2, sizeof(v4d));
      std::memcpy(&c3.mean_x, &v3, sizeof(v4d));
      c0.corr_yy = yy[0];
      c1.corr_yy = yy[1];
      c2.corr_yy = yy[2];
      c3.corr_yy = yy[3];
      c0.n = n1[0];
      c1.n = n1[1];
      c2.n = n1[2];
      c3.n = n1[3];
      c0.valid = c1.valid = c2.valid = c3.valid = false;
    }
    for (size_t l = 0; l < n_late; ++l)
    {
      const uint32_t k = late_[l];
      cells[late_cell_[l]].add(xy[2 * k], xy[2 * k + 1]);
    }
  }
  cells[outside] = HostCell();
}

// The body twice, as target_clones("avx2", "default") would make it -- written out, because that
// attribute's dispatcher is a global symbol whatever the function's visibility, and the library exports
// nothing of its host side but the C-ABI.
#if defined(__x86_64__) && defined(__GNUC__) && !defined(__clang__)
__attribute__((target("avx2"))) void HostNdt::add_scan_avx2(double pose_x, double pose_y, double pose_theta, const double * pts,
                                                            size_t n)
{
  add_scan_body(pose_x, pose_y, pose_theta, pts, n);
}
static const bool kHaveAvx2 = __builtin_cpu_supports("avx2") != 0;
#else
void HostNdt::add_scan_avx2(double pose_x, double pose_y, double pose_theta, const double * pts, size_t n)
{
  add_scan_body(pose_x, pose_y, pose_theta, pts, n);
}
static const bool kHaveAvx2 = false;
#endif

void HostNdt::add_scan(double pose_x, double pose_y, double pose_theta, const double * pts, size_t n)
{
  if (kHaveAvx2) return add_scan_avx2(pose_x, pose_y, pose_theta, pts, n);
  add_scan_body(pose_x, pose_y, pose_theta, pts, n);
}

void HostNdt::load6(const double * cells6)
{
  for (size_t i = 0; i < n_cells_; ++i)
  {
    const double * r = cells6 + 6 * i;
    HostCell & c = cells_[i];
    if (r[5] == 0.0) continue;
    c.mean_x = r[0];
    c.mean_y = r[1];
    c.info_xx = r[2];
    c.info_xy = r[3];
    c.info_yy = r[4];
    c.n = r[5];
    touched_.push_back(static_cast<uint32_t>(i));
  }
}

void HostNdt::compute(int eigen_form)
{
  for (const uint32_t i : touched_) cells_[i].compute(eigen_form);
}

void HostNdt::sparse6(uint32_t * index, double * cells6) const
{
  for (size_t k = 0; k < touched_.size(); ++k)
  {
    index[k] = touched_[k];
    const HostCell & c = cells_[touched_[k]];
    double * out = cells6 + 6 * k;
    out[0] = c.mean_x;
    out[1] = c.mean_y;
    out[2] = c.info_xx;
    out[3] = c.info_xy;
    out[4] = c.info_yy;
    out[5] = c.n;
  }
}

void HostNdt::pack6(double * out) const
{
  for (size_t i = 0; i < n_cells_; ++i)
  {
    const HostCell & c = cells_[i];
    out[6 * i + 0] = c.mean_x;
    out[6 * i + 1] = c.mean_y;
    out[6 * i + 2] = c.info_xx;
    out[6 * i + 3] = c.info_xy;
    out[6 * i + 4] = c.info_yy;
    out[6 * i + 5] = c.n;
  }
}

// ScanMatcherNDT::addScans' extent + NDT build, reference src/scan_matcher_ndt.cpp:49-74.
// max_x_/max_y_ start at numeric_limits<double>::min(), as the reference has it.
std::unique_ptr<HostNdt> build_ndt(double resolution, double range_max, const double * poses,
                                   const double * pts, const size_t * offsets, size_t n_scans,
                                   std::unique_ptr<HostNdt> reuse, int eigen_form, bool side_by_side)
{
  double min_x = std::numeric_limits<double>::max();
  double max_x = std::numeric_limits<double>::min();
  double min_y = std::numeric_limits<double>::max();
  double max_y = std::numeric_limits<double>::min();
  for (size_t k = 0; k < n_scans; ++k)
  {
    min_x = std::min(poses[3 * k] - range_max, min_x);
    max_x = std::max(poses[3 * k] + range_max, max_x);
    min_y = std::min(poses[3 * k + 1] - range_max, min_y);
    max_y = std::max(poses[3 * k + 1] + range_max, max_y);
  }
  // NDT::NDT (src/ndt_model.cpp:118-126) sizes the grid (size_t)(extent / cell_size + 1) per axis:
  // a pose of 1e15 or a NaN makes that a count no allocation can serve (or, cast from NaN, undefined
  // behaviour).  Refused here, before any storage is asked for: nullptr.
  {
    const double fsx = ((max_x - min_x) / resolution) + 1, fsy = ((max_y - min_y) / resolution) + 1;
    if (!(fsx >= 1.0) || !(fsy >= 1.0) || !(fsx * fsy < 2147483648.0)) return nullptr;
  }
  std::unique_ptr<HostNdt> ndt = std::move(reuse);
  if (ndt)
  {
    ndt->reset(resolution, (max_x - min_x), (max_y - min_y), min_x, min_y);
  }
  else
  {
    ndt.reset(new HostNdt(resolution, (max_x - min_x), (max_y - min_y), min_x, min_y));
  }
  ndt->set_interleave(side_by_side);
  for (size_t k = 0; k < n_scans; ++k)
  {
    ndt->add_scan(poses[3 * k], poses[3 * k + 1], poses[3 * k + 2], pts + 2 * offsets[k],
                  offsets[k + 1] - offsets[k]);
  }
  ndt->compute(eigen_form);
  return ndt;
}

// The reference's `for (v = -size; v < size; v += res)` (src/scan_matcher_ndt.cpp:103,117,119):
// the visited values come from repeated floating-point addition.
std::vector<double> search_offsets(double size, double res)
{
  std::vector<double> out;
  if (!(res > 0.0))
  {
    if (-size < size) out.push_back(-size);  // the reference would never terminate
    return out;
  }
  for (double v = -size; v < size; v += res) out.push_back(v);
  return out;
}

// Whether search_offsets(size, res) ends and stays within `limit` values.
bool offsets_fit(double size, double res, size_t limit)
{
  if (!std::isfinite(size) || !std::isfinite(res)) return false;
  if (!(res > 0.0)) return true;                  // (search_offsets: at most one value)
  if (!(size > 0.0)) return true;                 // (-size < size fails at once: no value)
  return 2.0 * size / res <= static_cast<double>(limit) - 2.0;
}

// The off-grid rule (include/ndt2d_hip.h) for the beams the device scores.  A beam with a NaN or
// infinite coordinate is off the grid for every pose, but the device scorers send a point off the
// grid to a sentinel record (mean (1e300, 0), information -1) whose arithmetic turns it into exp(NaN);
// and a beam near 1e300 lands near that mean and scores exp(-q^2) > 0.  A beam with a coordinate
// outside +-1e200 m (off any grid a scan reaches) is therefore handed on as (-1e300, -1e300): 1.4e300
// from every pose and at least 4e299 from the sentinel's mean -- exponent -inf, term +0.0, what the
// reference adds for a point off the grid.  (The host scorers give it the same +0.0.)
constexpr double kOffGridBeamBound = 1.0e200;
constexpr double kOffGridBeam = -1.0e300;

// The same rule for matchLaserScan, whose conversion and subsampling run on the device: a range the
// conversion keeps (reference src/ndt_mapper.cpp:413,436 drop NaN and range > range_max only) and that is
// infinite -- -inf, REP-117 "too close", or +inf under an infinite range_max -- converts to a point
// with an infinite or NaN coordinate, which the device would score as NaN.  Such a range goes to the
// device as +-FLT_MAX, which the conversion keeps as well: a finite point 3.4e38 m out, off the grid
// and scored +0.0 like the original.  (Every other kept range converts to a finite point within
// FLT_MAX of the laser; the laser and motion transforms are taken as finite.)  Returns the ranges to
// upload: `ranges` itself unless one needed changing.  One pass over the ranges on the host.
const float * off_grid_ranges(std::vector<float> & scratch, const float * ranges, size_t n_ranges,
                              double range_max)
{
  size_t first = n_ranges;
  for (size_t i = 0; i < n_ranges; ++i)
  {
    if (std::isinf(ranges[i]) && !(ranges[i] > range_max))
    {
      first = i;
      break;
    }
  }
  if (first == n_ranges) return ranges;
  scratch.assign(ranges, ranges + n_ranges);
  for (size_t i = first; i < n_ranges; ++i)
  {
    const float r = scratch[i];
    const float f = std::copysign(FLT_MAX, r);
    if (std::isinf(r) && !(r > range_max) && !(f > range_max)) scratch[i] = f;
  }
  return scratch.data();
}

// Subsampling of matchScan / scorePoints, reference src/scan_matcher_ndt.cpp:95-96,110.
void subsample_into(std::vector<double> & out, const double * pts, size_t n_points,
                    size_t laser_max_beams)
{
  const size_t use = std::min(laser_max_beams, n_points);
  out.resize(2 * use);
  if (use == 0) return;
  const double scan_step = static_cast<double>(n_points) / use;
  // (the copy as it stands with one branch-free flag, and the far beams replaced in a second pass
  // only when there are any)
  bool far = false;
  for (size_t i = 0; i < use; ++i)
  {
    const size_t idx = static_cast<size_t>(i * scan_step);
    const double x = pts[2 * idx], y = pts[2 * idx + 1];
    out[2 * i] = x;
    out[2 * i + 1] = y;
    far |= !(std::fabs(x) <= kOffGridBeamBound) | !(std::fabs(y) <= kOffGridBeamBound);
  }
  if (!far) return;
  for (size_t i = 0; i < use; ++i)
  {
    const bool near = std::fabs(out[2 * i]) <= kOffGridBeamBound && std::fabs(out[2 * i + 1]) <= kOffGridBeamBound;
    if (!near) out[2 * i] = out[2 * i + 1] = kOffGridBeam;
  }
}

}  // namespace host
}  // namespace ndt2d

namespace
{
void guard_note(std::nullptr_t, const char *) noexcept {}   // (ndt2d_guard.h: these calls have no handle)
}  // namespace

using namespace ndt2d::host;

extern "C" {

int ndt2d_search_offsets(double size, double res, double * out, size_t cap, size_t * n_out)
{
  NDT2D_C_TRY
  if (!offsets_fit(size, res, 1u << 24)) return NDT2D_ERR_INVALID;   // (a loop that would not end, or only fill memory)
  const std::vector<double> v = search_offsets(size, res);
  if (n_out != nullptr) *n_out = v.size();
  if (out != nullptr)
  {
    for (size_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_host_build_grid(double ndt_resolution, double range_max, const double * poses_xyt,
                          const double * points_xy, const size_t * offsets, size_t n_scans,
                          double * cells6_out, size_t capacity_cells, uint32_t * size_x,
                          uint32_t * size_y, double * origin_x, double * origin_y)
{
  NDT2D_C_TRY
  return ndt2d_host_build_grid_ex(ndt_resolution, range_max, poses_xyt, points_xy, offsets, n_scans, 0u, cells6_out,
                                  capacity_cells, size_x, size_y, origin_x, origin_y);
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_host_build_grid_ex(double ndt_resolution, double range_max, const double * poses_xyt,
                             const double * points_xy, const size_t * offsets, size_t n_scans, unsigned flags,
                             double * cells6_out, size_t capacity_cells, uint32_t * size_x,
                             uint32_t * size_y, double * origin_x, double * origin_y)
{
  NDT2D_C_TRY
  if (!(ndt_resolution > 0.0) || (n_scans > 0 && (poses_xyt == nullptr || offsets == nullptr)))
  {
    return NDT2D_ERR_INVALID;
  }
  static const double no_points[2] = {0.0, 0.0};
  static const size_t no_offsets[1] = {0};
  std::unique_ptr<HostNdt> ndt = build_ndt(ndt_resolution, range_max, poses_xyt,
                                           points_xy ? points_xy : no_points,
                                           offsets ? offsets : no_offsets, n_scans, nullptr,
                                           (flags & NDT2D_BUILD_CLOSED_FORM) ? ndt2d::kEigenFormClosed
                                                                             : ndt2d::kEigenFormSchur,
                                           (flags & NDT2D_BUILD_SEQUENTIAL) == 0);
  if (!ndt) return NDT2D_ERR_INVALID;   // (degenerate extent: non-finite poses / range_max, >= 2^31 cells)
  if (size_x) *size_x = static_cast<uint32_t>(ndt->size_x());
  if (size_y) *size_y = static_cast<uint32_t>(ndt->size_y());
  if (origin_x) *origin_x = ndt->origin_x();
  if (origin_y) *origin_y = ndt->origin_y();
  if (cells6_out != nullptr)
  {
    if (capacity_cells < ndt->ncell()) return NDT2D_ERR_INVALID;
    ndt->pack6(cells6_out);
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

}  // extern "C"
