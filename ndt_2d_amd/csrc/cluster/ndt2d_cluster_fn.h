// The arithmetic of the particle clusterer (cluster/ndt2d_cluster.hip) that the kernels and a
// restatement must agree on bit for bit -- the contract of include/ndt2d_hip.h ("Pose clusters"):
// the bin key of a pose, the normalisation of its heading, the left-out predicate, the integer mass
// q of a weight, the hash of a key, the 26 neighbour keys with the heading's wrap, and the order
// clusters are ranked by.  Plain C++ without HIP types, host and device: every thread of the kernels
// runs it, and a stand-alone host program checks it (tests/cpp/cluster_fn_check.cpp).  A quotient and
// a product that must round separately are separate statements under a contraction-off pragma,
// whatever the flags of the translation unit.
#ifndef NDT2D_CLUSTER_FN_H_
#define NDT2D_CLUSTER_FN_H_

#include <math.h>
#include <stdint.h>

#include "../particles/ndt2d_key_table.h"   // (relative: a stand-alone check needs this directory alone on its path)

#if defined(__HIPCC__)
#define NDT2D_CLUSTER_HD __host__ __device__
#else
#define NDT2D_CLUSTER_HD
#endif

// (g++ has no such pragma in C++: a GNU build passes -ffp-contract=off, as build.py and the tests do)
#if defined(__clang__)
#define NDT2D_CLUSTER_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define NDT2D_CLUSTER_NO_CONTRACT
#endif

namespace ndt2d
{
namespace cluster
{

constexpr double kPi = 3.14159265358979323846;   // the double M_PI
constexpr double kTwoPi = 2.0 * kPi;             // exact: a power of two times M_PI
constexpr double kKeyLimit = 1073741824.0;       // 2^30: |x / cell| at and above it is left out
constexpr double kTwo40 = 1099511627776.0;       // 2^40
constexpr double kInv40 = 1.0 / kTwo40;          // exact
constexpr uint32_t kLeftOut = 0xffffffffu;       // the label of a particle that is left out
constexpr int kNeighbours = 26;

struct Bins
{
  double cell_x, cell_y;
  int32_t n_theta;   // >= 1
};

// The key of a bin, its hash and the size of the table over it: particles/ndt2d_key_table.h.
using Key = particles::Key3;   // kt < 0: left out
using particles::key_hash;
using particles::same_key;
using particles::table_size;

// theta into [-pi, pi): the remainder of theta / 2 pi (fmod is exact), then at most one turn either
// way.  pi itself goes to -pi; a remainder that the added turn rounds up to pi goes there too.
NDT2D_CLUSTER_HD inline double normalise_angle(double theta)
{
  NDT2D_CLUSTER_NO_CONTRACT
  double r = fmod(theta, kTwoPi);
  if (r < -kPi) r = r + kTwoPi;
  if (r >= kPi) r = r - kTwoPi;
  return r;
}

// min(n_theta - 1, (int) ((t + pi) / (2 pi) * n_theta)) for t in [-pi, pi): an add, a quotient and a
// product, each rounded on its own, then truncation.  (The clamp: t + pi can round up to 2 pi.)
NDT2D_CLUSTER_HD inline int32_t theta_bin(double t, int32_t n_theta)
{
  NDT2D_CLUSTER_NO_CONTRACT
  const double shifted = t + kPi;
  const double turn = shifted / kTwoPi;
  const double scaled = turn * static_cast<double>(n_theta);
  const int32_t k = static_cast<int32_t>(scaled);   // 0 <= scaled <= n_theta
  return k < n_theta - 1 ? k : n_theta - 1;
}

// A weight counts when it lies in [0, 1]; a NaN fails both comparisons.
NDT2D_CLUSTER_HD inline bool weight_counts(double w) { return w >= 0.0 && w <= 1.0; }

// q = (uint64) (w 2^40) for w in [0, 1]: the product is exact, the conversion truncates.  A weight
// below 2^-40 has q = 0: it does not count towards the rank (it does towards W and the statistics).
NDT2D_CLUSTER_HD inline uint64_t mass_q(double w) { return static_cast<uint64_t>(w * kTwo40); }

// The key of a pose, or kt = -1 where the particle is left out: a pose that is not finite, a
// quotient x / cell or y / cell of magnitude 2^30 and above, a weight that does not count.
// floor, not truncation: the bins either side of 0 are as wide as every other.
NDT2D_CLUSTER_HD inline Key key_of(double x, double y, double theta, double w, const Bins & b)
{
  NDT2D_CLUSTER_NO_CONTRACT
  Key k;
  k.kx = 0;
  k.ky = 0;
  k.kt = -1;
  if (!(isfinite(x) && isfinite(y) && isfinite(theta))) return k;
  if (!weight_counts(w)) return k;
  const double qx = x / b.cell_x;
  const double qy = y / b.cell_y;
  if (!(fabs(qx) < kKeyLimit && fabs(qy) < kKeyLimit)) return k;
  k.kx = static_cast<int32_t>(floor(qx));
  k.ky = static_cast<int32_t>(floor(qy));
  k.kt = theta_bin(normalise_angle(theta), b.n_theta);
  return k;
}

// Neighbour j (0 .. 25) of a key: the offsets (dx, dy, dt) in {-1, 0, 1}^3 without (0, 0, 0), dt
// slowest and dx fastest, the heading bin taken modulo n_theta.  With n_theta of 1 or 2 some
// entries name the key itself or one twin more than once; a reader takes them as they come.
NDT2D_CLUSTER_HD inline Key neighbour(const Key & k, int j, int32_t n_theta)
{
  const int cell = j < 13 ? j : j + 1;   // the 27 offsets without the middle one
  const int dx = cell % 3 - 1, dy = (cell / 3) % 3 - 1, dt = cell / 9 - 1;
  Key out;
  out.kx = k.kx + dx;   // |kx| <= 2^30: no overflow
  out.ky = k.ky + dy;
  int32_t t = (k.kt + dt) % n_theta;
  if (t < 0) t += n_theta;
  out.kt = t;
  return out;
}

// The total order clusters are ranked by: mass descending, then label ascending.
NDT2D_CLUSTER_HD inline bool ranks_before(uint64_t q_a, uint32_t label_a, uint64_t q_b, uint32_t label_b)
{
  return q_a > q_b || (q_a == q_b && label_a < label_b);
}

}  // namespace cluster
}  // namespace ndt2d

#endif  // NDT2D_CLUSTER_FN_H_
