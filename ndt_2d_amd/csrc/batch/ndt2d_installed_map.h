// The grid installed in the context as a kernel reads it, once: the map policy of the lane's walk
// (MAP, ndt2d_walk_fn.h) for the searches of ndt2d_batch_search.h, and the SOURCE of the refine and
// verify kernels on the installed grid.  No kernel is defined here: refine/ and verify/ take this
// without the search kernels.
// Included by the .hip translation units only.
#ifndef NDT2D_INSTALLED_MAP_H_
#define NDT2D_INSTALLED_MAP_H_

#include "ndt2d_device_fn.h"

namespace ndt2d
{

namespace
{

// The installed grid as the lane's walk reads it: a cell is its own record.
struct InstalledMap
{
  const uint32_t * occ_bits;
  const double * cells_global;
  __device__ __forceinline__ bool find(uint32_t cell, uint32_t & rank) const
  {
    rank = cell;   // (<= ncell: bit ncell is 0)
    return ((occ_bits[cell >> 5] >> (cell & 31u)) & 1u) != 0u;
  }
  __device__ __forceinline__ const double2 * record(uint32_t rank) const
  {
    return reinterpret_cast<const double2 *>(cells_global + static_cast<size_t>(rank) * kCellStrideGlobal);
  }
};

// SOURCE (refine/ndt2d_refine_kernel.h, verify/ndt2d_verify_kernel.h) of the grid installed in the
// context: one grid for all jobs, a cell is its own record.
struct InstalledSource
{
  GridDesc g;   // geometry, cells_global, occ_bits
  __device__ __forceinline__ const GridDesc & grid(uint32_t) const { return g; }
  __device__ __forceinline__ InstalledMap map(uint32_t) const { return InstalledMap{g.occ_bits, g.cells_global}; }
};

}  // namespace

}  // namespace ndt2d

#endif  // NDT2D_INSTALLED_MAP_H_
