// NDT build of a mapper-size map in ONE workgroup: NDT::addScan for every scan in order plus
// NDT::compute (reference src/ndt_model.cpp:50-103,132-160), for maps of at most kFusedMaxPoints
// points on a grid of fewer than 65,535 cells (the mapper's local map and a loop closure's
// candidate map: ten scans, ~6,500 points, 41 x 41 to 245 x 245 cells) -- and the scan store that
// keeps scans on the device for it.  The device build of ndt2d_build.hip is a dozen stream
// operations (points, library radix sort, segments, sums, cells, bytes, compact, read-back) and
// the host build a divide chain on the CPU while the GPU idles; here everything order-dependent is
// one launch:
//
//   build_small_kernel   one workgroup of 1,024 threads:
//     1. a thread per point: transform by its scan's pose (cos / sin from the host libm),
//        cell_index (ndt2d_device_fn.h: the function and off-grid rules of points_kernel) ->
//        16-bit key in LDS, world-frame point to a global scratch array
//     2. stable LSD radix sort of the point indices by key in LDS, 4 bits a pass
//     3. segment heads -> the touched cells, in cell order
//     4. a lane per (touched cell, quantity), eight lanes to a cell of which five work, walks
//        the cell's points in the reference's order (cell_sums_kernel's recurrences); lane 0 of
//        the eight then does Cell::compute and writes the cell's raw record {mean, information,
//        n} and its index into the list the context's list install takes
//   grid_install_kernel + grid_bytes_sparse_kernel   (ndt2d_grid_stage_commit, unchanged): every
//        layout the scorers read, from that list
//
// Three launches and the read-back of the list's length.  The list is written straight into the
// pinned staging buffer ndt2d_grid_stage_begin hands out, where the install kernel reads it in
// place: the records cross PCIe once each way and no copy command is queued.  Stream order is the
// only ordering between the launches; inside the workgroup the only barrier is __syncthreads.
//
// Why through the list install and not by writing the scorers' layouts from the workgroup: the
// context's buffers are private to csrc/device/, and the kernel sources at the top of csrc/
// are pinned by the hash the committed counter profiles carry (profiles/r06_pmc.json,
// tests/test_bench_artefacts.py) -- this directory stands beside them, like resample/ and
// occupancy_map/, and goes through the public boundary.  For the same reason Cell::compute is
// restated in ndt2d_build_fn.h here instead of being shared with cells_kernel.
//
// Everything is IEEE double with the reference's operation order (file compiled with
// -ffp-contract=off; '/' and sqrt are correctly rounded): the grid is bit-identical to the host
// build's and to ndt2d_build.hip's.
//
// LDS (all dynamic: the launcher asks for it through prepare_absolute_lds_kernel), N = kFusedMaxPoints:
//   keys    u16[N]        32,768 B   cell of point i (ncell = off the grid)
//   val_a   u16[N]        32,768 B   point indices, ping
//   val_b   u16[N]        32,768 B   point indices, pong; ahead of the sort: the scans' first points
//   cnt     u16[N + 16]   32,800 B   16 digits x 1,024 threads of radix counters; behind the sort: segment starts
//   waves   u32[32]          128 B   block scan partials
//   total                131,232 B of the CU's 163,840.  A point costs 6 bytes and the counters' size
//   does not depend on N, so 21,000 points would fit as well; 16,384 is ten scans of a
//   1,440-beam lidar with room to spare, and keeps every count and index a 16-bit value with
//   headroom (prefixes reach N, which must stay below 65,536).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "ndt2d_build_small_fn.h"
#include "ndt2d_guard.h"
#include "ndt2d_hip.h"

namespace ndt2d
{

using namespace fused;   // ndt2d_build_small_fn.h: the workgroup, its LDS layout, the geometry

namespace
{

__global__ void __launch_bounds__(kThreads) build_small_kernel(const SmallBuildArgs a)
{
  extern __shared__ __align__(16) unsigned char lds[];
  (void)build_small_workgroup(a, lds);
}

hipError_t launch_build_small(const SmallBuildArgs & args, hipStream_t stream)
{
  const uint32_t ncell = args.grid.ncell;
  if (args.n_points > kFusedMaxPoints || ncell >= 65535u || ncell == 0u || args.n_scans == 0u)
  {
    return hipErrorInvalidValue;
  }
  SmallBuildArgs a = args;
  a.sort_passes = sort_passes_for(ncell);
  // (no static LDS in front of the arrays: prepare_absolute_lds_kernel, ndt2d_kernels.h)
  const hipError_t e = prepare_absolute_lds_kernel(reinterpret_cast<const void *>(build_small_kernel), kLdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(build_small_kernel, dim3(1), dim3(kThreads), kLdsBytes, stream, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace ndt2d

// ---- the scan store (struct ndt2d_scanstore: ndt2d_build_small_fn.h) and the C entry points ----


namespace
{

using ndt2d::GridDesc;
using ndt2d::kFusedMaxPoints;

void guard_note(ndt2d_scanstore * s, const char * what) noexcept
{
  if (s == nullptr) return;
  try
  {
    s->err = what;
  }
  catch (...)
  {
  }
}
void guard_note(std::nullptr_t, const char *) noexcept {}

int sfail(ndt2d_scanstore * s, int code, const std::string & msg)
{
  if (s != nullptr) s->err = msg;
  return code;
}

int sfail_hip(ndt2d_scanstore * s, hipError_t e, const char * what)
{
  (void)hipGetLastError();  // clear sticky state
  return sfail(s, NDT2D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define NDT2D_STORE_HIP(s, call)                            \
  do                                                        \
  {                                                         \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return sfail_hip(s, e__, #call); \
  } while (0)

int parse_form(const char * form)
{
  if (form == nullptr) return -1;
  if (std::strcmp(form, "eigen") == 0) return 0;
  if (std::strcmp(form, "closed") == 0) return 1;
  return -1;
}

void free_store(ndt2d_scanstore * s)
{
  (void)hipSetDevice(s->device);
  if (s->pool != nullptr) (void)hipFree(s->pool);
  if (s->world != nullptr) (void)hipFree(s->world);
  if (s->table != nullptr) (void)hipFree(s->table);
  if (s->list != nullptr) (void)hipFree(s->list);
  if (s->pinned != nullptr) (void)hipHostFree(s->pinned);
  if (s->n_touched != nullptr) (void)hipHostFree(s->n_touched);
  delete s;
}

int make_store(ndt2d_handle h, size_t capacity_points, size_t capacity_scans, ndt2d_scanstore ** out)
{
  ndt2d_scanstore * s = new ndt2d_scanstore();
  s->h = h;
  s->device = ndt2d_device_id(h);
  s->capacity_points = capacity_points;
  s->capacity_scans = capacity_scans;
  hipError_t e = hipSetDevice(s->device);
  if (e == hipSuccess)
  {
    e = hipMalloc(reinterpret_cast<void **>(&s->pool), (capacity_points + kFusedMaxPoints) * 2 * sizeof(double));
  }
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->world), kFusedMaxPoints * 2 * sizeof(double));
  if (e == hipSuccess)
  {
    e = hipHostMalloc(reinterpret_cast<void **>(&s->n_touched), 64, hipHostMallocDefault);
  }
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&s->n_touched_dev), s->n_touched, 0);
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    free_store(s);
    return NDT2D_ERR_HIP;
  }
  *out = s;
  return NDT2D_OK;
}

// The whole of addScans through the fused kernel and the context's list install.  Scan k has pose
// poses_xyt[3k..] and count[k] points at pool_offset[k] (in points) of the store's pool, or --
// host_points != nullptr -- of host_points, which then travel into the pool's scratch region.
// Arguments are checked by the callers; nothing is launched and the installed grid stays unless
// the map fits.
int build_small(ndt2d_scanstore * s, const char * who, double ndt_resolution, double range_max,
                const double * poses_xyt, size_t n_scans, const uint32_t * pool_offset, const uint32_t * count,
                size_t n_points, const double * host_points, bool clear_when_too_large)
{
  ndt2d_handle h = s->h;
  GridDesc g{};
  if (!ndt2d::addscans_geometry(ndt_resolution, range_max, poses_xyt, n_scans, &g))
  {
    return sfail(s, NDT2D_ERR_INVALID, std::string(who) + ": degenerate grid extent");
  }
  if (!ndt2d::small_map_fits(g, n_points))
  {
    if (clear_when_too_large) (void)ndt2d_clear_grid(h);
    return sfail(s, NDT2D_ERR_INVALID, std::string(who) + ": the map exceeds the fused build's limits (" +
                                         std::to_string(n_points) + " points of at most " +
                                         std::to_string(kFusedMaxPoints) + ", " + std::to_string(g.ncell) +
                                         " cells of fewer than 65535)");
  }
  NDT2D_STORE_HIP(s, hipSetDevice(s->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(h));

  // [scan table | host points] in pinned staging (free again: every build ends with a synchronisation)
  const size_t n_table = (5 * n_scans + 1) & ~size_t(1);
  const size_t n_pinned = n_table + (host_points != nullptr ? 2 * n_points : 0);
  if (n_pinned > s->pinned_cap)
  {
    if (s->pinned != nullptr) NDT2D_STORE_HIP(s, hipHostFree(s->pinned));
    s->pinned = nullptr;
    s->pinned_cap = 0;
    const size_t cap = n_pinned < 4096 ? 4096 : n_pinned + n_pinned / 8;
    NDT2D_STORE_HIP(s, hipHostMalloc(reinterpret_cast<void **>(&s->pinned), cap * sizeof(double), hipHostMallocDefault));
    s->pinned_cap = cap;
  }
  if (n_table > s->table_cap)
  {
    if (s->table != nullptr) NDT2D_STORE_HIP(s, hipFree(s->table));
    s->table = nullptr;
    s->table_cap = 0;
    const size_t cap = n_table < 512 ? 512 : n_table + n_table / 8;
    NDT2D_STORE_HIP(s, hipMalloc(reinterpret_cast<void **>(&s->table), cap * sizeof(double)));
    s->table_cap = cap;
  }
  ndt2d::SmallScan * table = reinterpret_cast<ndt2d::SmallScan *>(s->pinned);
  uint32_t first = 0;
  for (size_t k = 0; k < n_scans; ++k)
  {
    table[k].x = poses_xyt[3 * k];
    table[k].y = poses_xyt[3 * k + 1];
    ndt2d_cos_sin(poses_xyt[3 * k + 2], &table[k].c, &table[k].s);   // (src/ndt_model.cpp:135-136, host libm)
    table[k].pool_offset = pool_offset[k] + (host_points != nullptr ? static_cast<uint32_t>(s->capacity_points) : 0u);
    table[k].first = first;
    first += count[k];
  }
  if (host_points != nullptr && n_points > 0)
  {
    std::memcpy(s->pinned + n_table, host_points, 2 * n_points * sizeof(double));
  }

  // The context opens a list install (no grid from here on, as in ndt2d_build_grid): the workgroup
  // writes the touched cells where the host would, the commit installs them.
  const size_t list_cap = std::max<size_t>(1, std::min<size_t>(n_points, g.ncell));
  uint32_t * list_index = nullptr;
  double * list_cells6 = nullptr;
  int rc = ndt2d_grid_stage_begin(h, g.size_x, g.size_y, list_cap, &list_index, &list_cells6);
  if (rc != NDT2D_OK) return sfail(s, rc, std::string(who) + ": ndt2d_grid_stage_begin: " + ndt2d_last_error(h));
  double * d_cells6 = nullptr;
  uint32_t * d_index = nullptr;
  const bool in_place =
    hipHostGetDevicePointer(reinterpret_cast<void **>(&d_cells6), list_cells6, 0) == hipSuccess &&
    hipHostGetDevicePointer(reinterpret_cast<void **>(&d_index), list_index, 0) == hipSuccess;
  if (!in_place)
  {
    (void)hipGetLastError();
    if (list_cap > s->list_cap)
    {
      if (s->list != nullptr) (void)hipFree(s->list);
      s->list = nullptr;
      s->list_cap = 0;
      const hipError_t e = hipMalloc(reinterpret_cast<void **>(&s->list), list_cap * 7 * sizeof(double));
      if (e != hipSuccess)
      {
        (void)ndt2d_clear_grid(h);
        return sfail_hip(s, e, "hipMalloc");
      }
      s->list_cap = list_cap;
    }
    d_cells6 = s->list;
    d_index = reinterpret_cast<uint32_t *>(s->list + list_cap * 6);
  }

  ndt2d::SmallBuildArgs a{};
  a.grid = g;
  a.pool_xy = s->pool;
  a.scans = reinterpret_cast<const ndt2d::SmallScan *>(s->table);
  a.n_scans = static_cast<uint32_t>(n_scans);
  a.n_points = static_cast<uint32_t>(n_points);
  a.world_xy = s->world;
  a.list_cells6 = d_cells6;
  a.list_index = d_index;
  a.n_touched_out = s->n_touched_dev;
  a.eigen_form = s->eigen_form;
  hipError_t e = hipMemcpyAsync(s->table, s->pinned, n_table * sizeof(double), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess && host_points != nullptr && n_points > 0)
  {
    e = hipMemcpyAsync(s->pool + 2 * s->capacity_points, s->pinned + n_table, 2 * n_points * sizeof(double),
                       hipMemcpyHostToDevice, stream);
  }
  if (e == hipSuccess) e = ndt2d::launch_build_small(a, stream);
  // the list's length comes back to the host: the one read-back of the build
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  uint32_t n_touched = 0;
  if (e == hipSuccess)
  {
    n_touched = *static_cast<volatile uint32_t *>(s->n_touched);
    if (n_touched > list_cap) e = hipErrorUnknown;
  }
  if (e == hipSuccess && !in_place && n_touched > 0)
  {
    e = hipMemcpy(list_cells6, d_cells6, static_cast<size_t>(n_touched) * 6 * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(list_index, d_index, static_cast<size_t>(n_touched) * sizeof(uint32_t), hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess)
  {
    (void)ndt2d_clear_grid(h);   // (the open list is dropped with it)
    return sfail_hip(s, e, who);
  }
  rc = ndt2d_grid_stage_commit(h, n_touched, g.cell_size, g.origin_x, g.origin_y);
  if (rc != NDT2D_OK) return sfail(s, rc, std::string(who) + ": ndt2d_grid_stage_commit: " + ndt2d_last_error(h));
  return NDT2D_OK;
}

// ndt2d_build_grid_small(h, ...) has no object to keep its device memory in: a store without
// resident scans per context, found by the handle (ndt2d_build_small_release frees it).
std::mutex g_scratch_mutex;
std::unordered_map<ndt2d_handle, ndt2d_scanstore *> g_scratch;

ndt2d_scanstore * scratch_store(ndt2d_handle h, bool create)
{
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  auto it = g_scratch.find(h);
  if (it != g_scratch.end())
  {
    // (a handle's address can come back after ndt2d_destroy without a release in between: a store
    // made for another device is not this context's)
    if (it->second->device == ndt2d_device_id(h)) return it->second;
    free_store(it->second);
    g_scratch.erase(it);
  }
  if (!create) return nullptr;
  ndt2d_scanstore * s = nullptr;
  if (make_store(h, 0, 0, &s) != NDT2D_OK) return nullptr;
  g_scratch[h] = s;
  return s;
}

}  // namespace

extern "C" {

size_t ndt2d_build_small_max_points(void) { return kFusedMaxPoints; }

int ndt2d_build_grid_small_fits(double ndt_resolution, double range_max, const double * poses_xyt, size_t n_scans,
                                size_t n_points)
{
  if (!(ndt_resolution > 0.0) || n_scans == 0 || poses_xyt == nullptr) return 0;
  GridDesc g{};
  return (ndt2d::addscans_geometry(ndt_resolution, range_max, poses_xyt, n_scans, &g) &&
          ndt2d::small_map_fits(g, n_points)) ? 1 : 0;
}

int ndt2d_build_grid_small(ndt2d_handle h, double ndt_resolution, double range_max, const double * poses_xyt,
                           const double * points_xy, const size_t * offsets, size_t n_scans)
{
  ndt2d_scanstore * s = nullptr;
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  s = scratch_store(h, true);
  if (s == nullptr) return NDT2D_ERR_HIP;
  if (!(ndt_resolution > 0.0) || n_scans == 0 || poses_xyt == nullptr || offsets == nullptr ||
      n_scans > (1u << 30))
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_build_grid_small: bad argument");
  }
  const size_t n_points = offsets[n_scans];
  if (n_points >= (1ull << 31) || (n_points > 0 && points_xy == nullptr))
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_build_grid_small: bad points");
  }
  for (size_t k = 0; k < n_scans; ++k)
  {
    if (offsets[k + 1] < offsets[k] || offsets[k + 1] > n_points)
    {
      return sfail(s, NDT2D_ERR_INVALID, "ndt2d_build_grid_small: offsets must not decrease");
    }
  }
  s->job.resize(2 * n_scans);
  for (size_t k = 0; k < n_scans; ++k)
  {
    s->job[k] = static_cast<uint32_t>(offsets[k]);
    s->job[n_scans + k] = static_cast<uint32_t>(offsets[k + 1] - offsets[k]);
  }
  static const double no_points[2] = {0.0, 0.0};
  return build_small(s, "ndt2d_build_grid_small", ndt_resolution, range_max, poses_xyt, n_scans, s->job.data(),
                     s->job.data() + n_scans, n_points, points_xy != nullptr ? points_xy : no_points, true);
  NDT2D_C_CATCH(s)
}

int ndt2d_build_small_set_eigenvalue_form(ndt2d_handle h, const char * form)
{
  NDT2D_C_TRY
  const int f = parse_form(form);
  if (h == nullptr || f < 0) return NDT2D_ERR_INVALID;
  // (the default needs no store; any other form is kept in one)
  ndt2d_scanstore * s = scratch_store(h, f != 0);
  if (s == nullptr) return f == 0 ? NDT2D_OK : NDT2D_ERR_HIP;
  s->eigen_form = f;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_build_small_last_error(ndt2d_handle h)
{
  if (h == nullptr) return "null handle";
  try
  {
    ndt2d_scanstore * s = scratch_store(h, false);
    return s != nullptr ? s->err.c_str() : "";
  }
  catch (...)
  {
    return "";
  }
}

int ndt2d_build_small_release(ndt2d_handle h)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  auto it = g_scratch.find(h);
  if (it == g_scratch.end()) return NDT2D_OK;
  (void)hipSetDevice(it->second->device);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(h)));
  free_store(it->second);
  g_scratch.erase(it);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_scanstore_create(ndt2d_handle h, size_t capacity_points, size_t capacity_scans, ndt2d_scanstore ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (capacity_points == 0 || capacity_scans == 0 || capacity_points >= (1ull << 31) - kFusedMaxPoints ||
      capacity_scans >= (1ull << 31))
  {
    return NDT2D_ERR_INVALID;
  }
  return make_store(h, capacity_points, capacity_scans, out);
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_scanstore_destroy(ndt2d_scanstore * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(s->h)));
  free_store(s);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_scanstore_last_error(ndt2d_scanstore * s)
{
  return s != nullptr ? s->err.c_str() : "null scan store";
}

int ndt2d_scanstore_set_eigenvalue_form(ndt2d_scanstore * s, const char * form)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const int f = parse_form(form);
  if (f < 0) return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scanstore_set_eigenvalue_form: unknown form (eigen, closed)");
  s->eigen_form = f;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_scanstore_append(ndt2d_scanstore * s, const double * points_xy, size_t n_points, size_t * id_out)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_points > 0 && points_xy == nullptr) return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scanstore_append: null points");
  if (s->count.size() >= s->capacity_scans)
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scanstore_append: the store is full (scans)");
  }
  if (n_points > s->capacity_points - s->used_points)
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scanstore_append: the store is full (points)");
  }
  if (n_points > 0)
  {
    // (the caller's buffer is free on return: the copy is waited for)
    hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(s->h));
    NDT2D_STORE_HIP(s, hipSetDevice(s->device));
    NDT2D_STORE_HIP(s, hipMemcpyAsync(s->pool + 2 * s->used_points, points_xy, 2 * n_points * sizeof(double),
                                      hipMemcpyHostToDevice, stream));
    NDT2D_STORE_HIP(s, hipStreamSynchronize(stream));
  }
  s->offset.push_back(static_cast<uint32_t>(s->used_points));
  s->count.push_back(static_cast<uint32_t>(n_points));
  s->used_points += n_points;
  if (id_out != nullptr) *id_out = s->count.size() - 1;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_scanstore_count(ndt2d_scanstore * s, size_t * n_scans_out)
{
  if (s == nullptr || n_scans_out == nullptr) return NDT2D_ERR_INVALID;
  *n_scans_out = s->count.size();
  return NDT2D_OK;
}

int ndt2d_scanstore_reset(ndt2d_scanstore * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  s->offset.clear();
  s->count.clear();
  s->used_points = 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_scanstore_build(ndt2d_scanstore * s, const size_t * ids, const double * poses_xyt, size_t n_scans,
                          double ndt_resolution, double range_max)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (ids == nullptr || poses_xyt == nullptr || n_scans == 0 || n_scans > (1u << 30) || !(ndt_resolution > 0.0) ||
      !std::isfinite(ndt_resolution) || !std::isfinite(range_max))
  {
    return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scanstore_build: bad argument");
  }
  for (size_t k = 0; k < 3 * n_scans; ++k)
  {
    if (!std::isfinite(poses_xyt[k])) return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scanstore_build: a scan pose is not finite");
  }
  size_t n_points = 0;
  for (size_t k = 0; k < n_scans; ++k)
  {
    if (ids[k] >= s->count.size())
    {
      return sfail(s, NDT2D_ERR_INVALID, "ndt2d_scanstore_build: unknown scan id " + std::to_string(ids[k]));
    }
    n_points += s->count[ids[k]];
  }
  s->job.resize(2 * n_scans);
  for (size_t k = 0; k < n_scans; ++k)
  {
    s->job[k] = s->offset[ids[k]];
    s->job[n_scans + k] = s->count[ids[k]];
  }
  return build_small(s, "ndt2d_scanstore_build", ndt_resolution, range_max, poses_xyt, n_scans, s->job.data(),
                     s->job.data() + n_scans, n_points, nullptr, false);
  NDT2D_C_CATCH(s)
}

}  // extern "C"
