// The device layer's translation unit -- ../ndt2d_device.hip, included whole and unchanged -- plus
// one read-only accessor to the grid installed in the context, for kernels that live beside the
// context (../batch/ndt2d_batch_host.h installed_grid: starts/, scans/).  The context struct is private to ndt2d_device.hip and stays there;
// the accessor has to be compiled with it to see it.  It is kept out of that file because the
// committed profiles (profiles/r06_pmc.json, r06_valu_mix.json) carry the hash of the top-level
// kernel sources they were taken with (bench.py source_hash): an accessor is no kernel edit and
// must not make them read as stale.  build.py compiles THIS file in place of ndt2d_device.hip.
#include "../ndt2d_device.hip"

extern "C" {

int ndt2d_grid_view_get(ndt2d_handle h, ndt2d_grid_view * out)
{
  NDT2D_C_TRY
  if (h == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  if (!h->has_grid) return fail(h, NDT2D_ERR_NO_GRID, "ndt2d_grid_view_get: no grid");
  const GridDesc & g = h->grid;
  out->cells_global = g.cells_global;
  out->occ_bits = g.occ_bits;
  out->size_x = g.size_x;
  out->size_y = g.size_y;
  out->ncell = g.ncell;
  out->pow2 = g.pow2;
  out->cell_size = g.cell_size;
  out->inv_cell_size = g.inv_cell_size;
  out->origin_x = g.origin_x;
  out->origin_y = g.origin_y;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

}  // extern "C"
