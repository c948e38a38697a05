// Cell::addPoint's recurrence and Cell::compute for the fused small-map build
// (ndt2d_build_small.hip): the arithmetic of cell_sums_kernel / cells_kernel (../ndt2d_build.hip),
// operation by operation -- restated here because that file, like every kernel source at the top
// of csrc/, is pinned by the hash the committed counter profiles carry.  IEEE double with the
// reference's operation order; compiled with -ffp-contract=off.
#ifndef NDT2D_BUILD_FN_H_
#define NDT2D_BUILD_FN_H_

#include <hip/hip_runtime.h>

#include "ndt2d_eigen2.h"

namespace ndt2d
{

// One of Cell::addPoint's five recurrences (src/ndt_model.cpp:50-63): quantity q of the cell
// (0, 1: the mean's components; 2, 3, 4: the upper triangle of the second moment) takes point p
// as the (n + 1)-th.  The caller advances n.
__device__ __forceinline__ double add_point_quantity(uint32_t q, double2 p, double v, double n)
{
  const double term = q == 0u ? p.x : q == 1u ? p.y : q == 2u ? p.x * p.x : q == 3u ? p.x * p.y : p.y * p.y;
  return (v * n + term) / (n + 1);
}

// Cell::compute (src/ndt_model.cpp:65-103) from the sums addPoint left: the information matrix
// of a cell with n >= 3 points, zeros otherwise.
__device__ __forceinline__ void cell_compute(int eigen_form, double n, double mean_x, double mean_y, double cxx,
                                             double cxy, double cyy, double * ixx_out, double * ixy_out,
                                             double * iyy_out)
{
  double ixx = 0.0, ixy = 0.0, iyy = 0.0;
  if (!(n < 3))
  {
    const double scale = n / (n - 1);
    const double vxx = (cxx - (mean_x * mean_x)) * scale;
    const double vxy = (cxy - (mean_x * mean_y)) * scale;
    const double vyy = (cyy - (mean_y * mean_y)) * scale;
    double small = 1.0, large = 1.0;
    if (!clamp_test_surely_false(vxx, vxy, vyy))   // (else: the branch of :99 whatever their last bits)
    {
      covariance_eigenvalues(eigen_form, vxx, vxy, vyy, &small, &large);   // (:84-85, ndt2d_eigen2.h)
      if (small > large)
      {
        const double t = small;
        small = large;
        large = t;
      }
    }
    if (small < 0.001 * large)
    {
      const double determinant = (0.001 * large) * large;
      ixx = vyy / determinant;
      ixy = -vxy / determinant;
      iyy = vxx / determinant;
    }
    else
    {
      const double det = vxx * vyy - vxy * vxy;
      const double invdet = 1.0 / det;
      ixx = vyy * invdet;
      ixy = -vxy * invdet;
      iyy = vxx * invdet;
    }
  }
  *ixx_out = ixx;
  *ixy_out = ixy;
  *iyy_out = iyy;
}

}  // namespace ndt2d

#endif  // NDT2D_BUILD_FN_H_
