// The plan of the dense covariance (covariance/ndt2d_covariance.hip): how a matrix of dimension
// d = 3 n is cut into panels and tiles, where an unknown lies, how many jobs a byte budget holds and
// which launches a factorisation and an inversion are made of.  Plain C++ without HIP types, host and
// device: the kernels index with it, the host sizes and launches with it, and a stand-alone host
// program walks it exhaustively (tests/cpp/covariance_plan_check.cpp).
//
// The matrices are row-major with the leading dimension padded(d): d rounded up to whole panels of
// kPanel = 48 columns, so that neither a node's 3 x 3 block nor a 16 x 16 tile of the matrix cores
// straddles a panel and every panel and tile is whole.  The rows and columns from d on are those of
// the identity.
#ifndef NDT2D_COVARIANCE_PLAN_H_
#define NDT2D_COVARIANCE_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NDT2D_COV_HD __host__ __device__
#else
#define NDT2D_COV_HD
#endif

namespace ndt2d
{
namespace covariance
{

constexpr uint32_t kPanel = 48;     // columns of a panel, rows and columns of a workgroup's block
constexpr uint32_t kTile = 16;      // rows and columns of a tile of v_mfma_f64_16x16x4_f64
constexpr uint32_t kRows = 64;      // rows (or columns) of a workgroup of the two substitutions
// the largest dimension: a row a block of the fill kernel's grid (65,535), whole panels
constexpr size_t kMaxDim = 65520;

// The scalar unknown j = 0, 1, 2 (x, y, heading) of a node: its row and its column.
NDT2D_COV_HD inline size_t unknown(size_t node, size_t j) { return 3 * node + j; }

NDT2D_COV_HD inline size_t panels(size_t d) { return (d + kPanel - 1) / kPanel; }
NDT2D_COV_HD inline size_t padded(size_t d) { return panels(d) * kPanel; }

// The doubles of a job on the device: the matrix A (then its factor L) and T (the identity, then
// L^-1), padded(d)^2 each; A's diagonal as assembled, padded(d); cos, sin and the free flag of
// each node, 3 n.
NDT2D_COV_HD inline size_t job_doubles(size_t n)
{
  const size_t ld = padded(3 * n);
  return 2 * ld * ld + ld + 3 * n;
}

// The jobs of a chunk: what the budget holds, at most max_jobs; 0 where not even one fits.
NDT2D_COV_HD inline size_t chunk_jobs(size_t max_jobs, size_t workspace_bytes, size_t job_bytes)
{
  const size_t fit = job_bytes == 0 ? max_jobs : workspace_bytes / job_bytes;
  return fit < max_jobs ? fit : max_jobs;
}

// The lower triangle of t x t blocks, row by row: q = r (r + 1) / 2 + c, c <= r.
NDT2D_COV_HD inline uint64_t lower_tiles(uint64_t t) { return t * (t + 1) / 2; }

NDT2D_COV_HD inline void lower_tile(uint64_t q, uint32_t * r, uint32_t * c)
{
  // the root of 8 q + 1 in doubles is exact to a unit here (q < 2^32); two bounded corrections
  uint64_t row = static_cast<uint64_t>((__builtin_sqrt(8.0 * static_cast<double>(q) + 1.0) - 1.0) * 0.5);
  for (int k = 0; k < 2 && lower_tiles(row) > q; ++k) --row;
  for (int k = 0; k < 2 && lower_tiles(row + 1) <= q; ++k) ++row;
  *r = static_cast<uint32_t>(row);
  *c = static_cast<uint32_t>(q - lower_tiles(row));
}

// A launch of the factorisation A = L L^T or of the inversion T = L^-1, all on panel p.
//   kFactor      the diagonal block (p, p) in one workgroup
//   kSolveBelow  the block rows below it, L[i, p] = A[i, p] L[p, p]^-T: kRows rows a workgroup
//   kUpdate      A[i, j] -= L[i, p] L[j, p]^T over the lower blocks p < j <= i: a block a workgroup
//   kSolveRow    T[p, 0 .. p] = L[p, p]^-1 T[p, 0 .. p]: kRows columns a workgroup
//   kUpdateRect  T[i, q] -= L[i, p] T[p, q] over the blocks i > p, q <= p (the others are zero)
enum Kind
{
  kFactor = 0,
  kSolveBelow = 1,
  kUpdate = 2,
  kSolveRow = 3,
  kUpdateRect = 4
};

struct Launch
{
  int kind;
  uint32_t panel;
  uint32_t groups;   // workgroups per job, never 0
};

// The launches in stream order: 3 per panel but the last for the factor, then 2 per panel but the
// last for the inverse.  out: room for what launch_list(d, NULL) counts, or NULL to count.  (Host.)
inline size_t launch_list(size_t d, Launch * out)
{
  const uint32_t np = static_cast<uint32_t>(panels(d));
  size_t count = 0;
  const auto put = [&](int kind, uint32_t p, uint64_t groups) {
    if (groups == 0) return;
    if (out != nullptr) out[count] = Launch{kind, p, static_cast<uint32_t>(groups)};
    ++count;
  };
  for (uint32_t p = 0; p < np; ++p)
  {
    const uint64_t below = np - p - 1;
    put(kFactor, p, 1);
    put(kSolveBelow, p, (below * kPanel + kRows - 1) / kRows);
    put(kUpdate, p, lower_tiles(below));
  }
  for (uint32_t p = 0; p < np; ++p)
  {
    const uint64_t below = np - p - 1, left = p + 1;
    put(kSolveRow, p, (left * kPanel + kRows - 1) / kRows);
    put(kUpdateRect, p, below * left);
  }
  return count;
}

// The block (row, column) a workgroup of kUpdate / kUpdateRect on panel p works on.
NDT2D_COV_HD inline void update_block(int kind, uint32_t p, uint32_t group, uint32_t * bi, uint32_t * bj)
{
  if (kind == kUpdate)
  {
    lower_tile(group, bi, bj);
    *bi += p + 1;
    *bj += p + 1;
  }
  else
  {
    *bi = p + 1 + group / (p + 1);
    *bj = group % (p + 1);
  }
}

}  // namespace covariance
}  // namespace ndt2d

#endif  // NDT2D_COVARIANCE_PLAN_H_
