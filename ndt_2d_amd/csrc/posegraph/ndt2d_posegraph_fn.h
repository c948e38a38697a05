// The arithmetic of the pose graph (posegraph/ndt2d_posegraph_kernel.h): the residual of one constraint,
// its analytic Jacobians, the products the matrix-free solver needs, the 3 x 3 symmetric inverse of
// the block-Jacobi preconditioner and the host's Cholesky of an information matrix -- the contract
// of include/ndt2d_hip.h ("Pose graph").  Plain C++ without HIP types, host and device: every
// thread of the kernels runs it, and a stand-alone host program checks it
// (tests/cpp/posegraph_fn_check.cpp).  Every operation is written out in the order a restatement
// has to follow; the translation units are compiled with -ffp-contract=off.
#ifndef NDT2D_POSEGRAPH_FN_H_
#define NDT2D_POSEGRAPH_FN_H_

#include <math.h>

#if defined(__HIPCC__)
#define NDT2D_PG_HD __host__ __device__
#else
#define NDT2D_PG_HD
#endif

namespace ndt2d
{
namespace posegraph
{

constexpr double kPi = 3.141592653589793238462643383279502884;

// Into [-pi, pi): IEEE + - x / and floor only, 2 pi formed as 2.0 * pi
// (include/ndt_2d/ceres_solver_pose.hpp:60-65).
NDT2D_PG_HD inline double normalize(double v)
{
  const double two_pi = 2.0 * kPi;
  return v - two_pi * floor((v + kPi) / two_pi);
}

// What the residual and both Jacobians of a constraint a -> b are made of: cos and sin of pose a's
// heading, and p_b - p_a rotated into a's frame.
struct Frame
{
  double c, s;     // cos, sin of theta_a
  double ex, ey;   // R(theta_a)^T (p_b - p_a)
};

NDT2D_PG_HD inline Frame frame(double c, double s, const double * pa, const double * pb)
{
  const double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
  Frame f;
  f.c = c;
  f.s = s;
  f.ex = c * dx + s * dy;
  f.ey = c * dy - s * dx;
  return f;
}

// e = (R_a^T (p_b - p_a) - t_xy, Normalize((theta_b - theta_a) - t_theta)).
NDT2D_PG_HD inline void error(const Frame & f, double theta_a, double theta_b, const double * t, double * e)
{
  e[0] = f.ex - t[0];
  e[1] = f.ey - t[1];
  e[2] = normalize((theta_b - theta_a) - t[2]);
}

// y = M v, y = M^T v of a row-major 3 x 3.
NDT2D_PG_HD inline void mul(const double * M, const double * v, double * y)
{
  y[0] = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
  y[1] = M[3] * v[0] + M[4] * v[1] + M[5] * v[2];
  y[2] = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
}

NDT2D_PG_HD inline void mul_t(const double * M, const double * v, double * y)
{
  y[0] = M[0] * v[0] + M[3] * v[1] + M[6] * v[2];
  y[1] = M[1] * v[0] + M[4] * v[1] + M[7] * v[2];
  y[2] = M[2] * v[0] + M[5] * v[1] + M[8] * v[2];
}

// The unweighted Jacobians, row-major: A = de / d(pose a), B = de / d(pose b).
//   A = [ -c  -s   ey ]      B = [  c  s  0 ]
//       [  s  -c  -ex ]          [ -s  c  0 ]
//       [  0   0  -1  ]          [  0  0  1 ]
NDT2D_PG_HD inline void jacobian_a(const Frame & f, double * A)
{
  A[0] = -f.c; A[1] = -f.s; A[2] = f.ey;
  A[3] = f.s;  A[4] = -f.c; A[5] = -f.ex;
  A[6] = 0.0;  A[7] = 0.0;  A[8] = -1.0;
}

NDT2D_PG_HD inline void jacobian_b(const Frame & f, double * B)
{
  B[0] = f.c;  B[1] = f.s;  B[2] = 0.0;
  B[3] = -f.s; B[4] = f.c;  B[5] = 0.0;
  B[6] = 0.0;  B[7] = 0.0;  B[8] = 1.0;
}

// y = A v, B v, A^T v, B^T v without forming the blocks.
NDT2D_PG_HD inline void apply_a(const Frame & f, const double * v, double * y)
{
  y[0] = (f.ey * v[2] - f.c * v[0]) - f.s * v[1];
  y[1] = (f.s * v[0] - f.c * v[1]) - f.ex * v[2];
  y[2] = -v[2];
}

NDT2D_PG_HD inline void apply_b(const Frame & f, const double * v, double * y)
{
  y[0] = f.c * v[0] + f.s * v[1];
  y[1] = f.c * v[1] - f.s * v[0];
  y[2] = v[2];
}

NDT2D_PG_HD inline void apply_at(const Frame & f, const double * v, double * y)
{
  y[0] = f.s * v[1] - f.c * v[0];
  y[1] = -(f.s * v[0] + f.c * v[1]);
  y[2] = (f.ey * v[0] - f.ex * v[1]) - v[2];
}

NDT2D_PG_HD inline void apply_bt(const Frame & f, const double * v, double * y)
{
  y[0] = f.c * v[0] - f.s * v[1];
  y[1] = f.s * v[0] + f.c * v[1];
  y[2] = v[2];
}

// S += J^T J of the weighted block J = W E (E: A or B), the symmetric 3 x 3 as (00, 01, 02, 11, 12, 22).
NDT2D_PG_HD inline void add_jtj(const double * W, const double * E, double * S)
{
  double J[9];
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j) J[3 * i + j] = W[3 * i] * E[j] + W[3 * i + 1] * E[3 + j] + W[3 * i + 2] * E[6 + j];
  }
  S[0] += J[0] * J[0] + J[3] * J[3] + J[6] * J[6];
  S[1] += J[0] * J[1] + J[3] * J[4] + J[6] * J[7];
  S[2] += J[0] * J[2] + J[3] * J[5] + J[6] * J[8];
  S[3] += J[1] * J[1] + J[4] * J[4] + J[7] * J[7];
  S[4] += J[1] * J[2] + J[4] * J[5] + J[7] * J[8];
  S[5] += J[2] * J[2] + J[5] * J[5] + J[8] * J[8];
}

// y = S v of a symmetric 3 x 3 stored as above.
NDT2D_PG_HD inline void mul_sym(const double * S, const double * v, double * y)
{
  y[0] = S[0] * v[0] + S[1] * v[1] + S[2] * v[2];
  y[1] = S[1] * v[0] + S[3] * v[1] + S[4] * v[2];
  y[2] = S[2] * v[0] + S[4] * v[1] + S[5] * v[2];
}

// A symmetric positive definite 3 x 3 D (00, 01, 02, 11, 12, 22) factored: M = L^-1 of D = L L^T, the lower triangle
// as (00, 10, 11, 20, 21, 22).  D^-1 v is applied as M^T (M v), two triangular products (apply_pivot); D^-1 itself is
// M^T M (pivot_inverse).  false (M zeroed: every product with it is zero) unless the three Cholesky pivots are
// positive finite numbers and M is finite.
NDT2D_PG_HD inline bool factor_spd(const double * S, double * M)
{
  const double big = 1.7976931348623157e308;
  const double p0 = S[0];
  const double l00 = sqrt(p0);
  const double l10 = S[1] / l00;
  const double l20 = S[2] / l00;
  const double p1 = S[3] - l10 * l10;
  const double l11 = sqrt(p1);
  const double l21 = (S[4] - l20 * l10) / l11;
  const double p2 = (S[5] - l20 * l20) - l21 * l21;
  const double l22 = sqrt(p2);
  const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
  const double m10 = -(l10 * m00) / l11;
  const double m21 = -(l21 * m11) / l22;
  const double m20 = -(l20 * m00 + l21 * m10) / l22;
  const double c[6] = {m00, m10, m11, m20, m21, m22};
  bool ok = p0 > 0.0 && p0 <= big && p1 > 0.0 && p1 <= big && p2 > 0.0 && p2 <= big;
  for (int i = 0; i < 6; ++i) ok = ok && fabs(c[i]) <= big;
  for (int i = 0; i < 6; ++i) M[i] = ok ? c[i] : 0.0;
  return ok;
}

// y = D^-1 v = M^T (M v).
NDT2D_PG_HD inline void apply_pivot(const double * M, const double * v, double * y)
{
  const double t0 = M[0] * v[0];
  const double t1 = M[1] * v[0] + M[2] * v[1];
  const double t2 = (M[3] * v[0] + M[4] * v[1]) + M[5] * v[2];
  y[0] = (M[0] * t0 + M[1] * t1) + M[3] * t2;
  y[1] = M[2] * t1 + M[4] * t2;
  y[2] = M[5] * t2;
}

// D^-1 = M^T M itself, symmetric storage (00, 01, 02, 11, 12, 22).
NDT2D_PG_HD inline void pivot_inverse(const double * M, double * P)
{
  P[0] = (M[0] * M[0] + M[1] * M[1]) + M[3] * M[3];
  P[1] = M[1] * M[2] + M[3] * M[4];
  P[2] = M[3] * M[5];
  P[3] = M[2] * M[2] + M[4] * M[4];
  P[4] = M[4] * M[5];
  P[5] = M[5] * M[5];
}

// The inverse of a symmetric positive definite 3 x 3, in the same storage: M^T M of factor_spd (the form of refine's
// covariance).  false (out zeroed) when a pivot is not a positive finite number or an entry of the inverse is not
// finite.  Its error grows with kappa(S), where the cofactor form's grew with kappa^1.5 (the determinant is summed
// from products kappa^1.5 times its size).
NDT2D_PG_HD inline bool invert_sym(const double * S, double * out)
{
  double M[6];
  bool ok = factor_spd(S, M);
  pivot_inverse(M, out);
  for (int i = 0; i < 6; ++i) ok = ok && fabs(out[i]) <= 1.7976931348623157e308;
  if (!ok)
  {
    for (int i = 0; i < 6; ++i) out[i] = 0.0;
  }
  return ok;
}

// The lower Cholesky factor L (row-major, zeros above the diagonal) of the lower triangle of a
// row-major 3 x 3; false when a pivot is <= 0 or not finite (the matrix is not symmetric positive
// definite as far as the factorisation can tell: Eigen's llt() goes on silently there).
NDT2D_PG_HD inline bool cholesky_lower(const double * I, double * L)
{
  for (int i = 0; i < 9; ++i) L[i] = 0.0;
  for (int j = 0; j < 3; ++j)
  {
    double d = I[3 * j + j];
    for (int k = 0; k < j; ++k) d -= L[3 * j + k] * L[3 * j + k];
    if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return false;
    const double root = sqrt(d);
    L[3 * j + j] = root;
    for (int i = j + 1; i < 3; ++i)
    {
      double v = I[3 * i + j];
      for (int k = 0; k < j; ++k) v -= L[3 * i + k] * L[3 * j + k];
      L[3 * i + j] = v / root;
    }
  }
  return true;
}

}  // namespace posegraph
}  // namespace ndt2d

#endif  // NDT2D_POSEGRAPH_FN_H_
