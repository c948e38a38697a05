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
// context's buffers are private to ndt2d_device.hip, and the kernel sources at the top of csrc/
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

#include "ndt2d_build_fn.h"
#include "ndt2d_device_fn.h"
#include "ndt2d_guard.h"
#include "ndt2d_hip.h"

namespace ndt2d
{

namespace
{

constexpr uint32_t kFusedMaxPoints = 16384;
constexpr uint32_t kThreads = 1024;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kDigits = 16;                          // 4 key bits a pass
constexpr uint32_t kFirstInLds = kFusedMaxPoints / 2;     // scans whose first points fit val_b as u32

// The scans' robot-frame points lie anywhere in one device pool; `first` is the running count of
// points in build order.
struct SmallScan
{
  double x, y, c, s;        // pose translation, cos / sin of pose theta (host libm)
  uint32_t pool_offset;     // the scan's first point in the pool (points, not doubles)
  uint32_t first;           // points of the scans before this one
};
static_assert(sizeof(SmallScan) == 5 * sizeof(double), "scan table record");

struct SmallBuildArgs
{
  GridDesc grid;              // geometry only
  const double * pool_xy;     // [..][2] robot-frame points
  const SmallScan * scans;    // [n_scans], device
  uint32_t n_scans;
  uint32_t n_points;          // of all scans together
  uint32_t sort_passes;
  double * world_xy;          // [n_points][2] scratch
  double * list_cells6;       // out: [touched][6] {mean_x, mean_y, i00, i01, i11, n}, in cell order
  uint32_t * list_index;      // out: [touched] cell of every record
  uint32_t * n_touched_out;   // out
  int eigen_form;
};

constexpr size_t kOffKeys = 0;
constexpr size_t kOffValA = kOffKeys + kFusedMaxPoints * sizeof(uint16_t);
constexpr size_t kOffValB = kOffValA + kFusedMaxPoints * sizeof(uint16_t);
constexpr size_t kOffCnt = kOffValB + kFusedMaxPoints * sizeof(uint16_t);
constexpr size_t kOffWaves = kOffCnt + (kFusedMaxPoints + 16) * sizeof(uint16_t);
constexpr size_t kLdsBytes = kOffWaves + 32 * sizeof(uint32_t);
static_assert(kDigits * kThreads == kFusedMaxPoints, "the counters alias the segment starts: N + 1 entries");
static_assert(kLdsBytes <= 160 * 1024, "one CU's LDS");
static_assert(kFusedMaxPoints < 65536, "indices and prefixes are 16-bit");

// Exclusive prefix of v over the block's threads (in thread order) and the block's total.
// Every thread of the block calls it; `waves` is free again on return.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t * waves, uint32_t * total)
{
  const uint32_t t = threadIdx.x;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1)
  {
    const uint32_t up = __shfl_up(incl, off, 64);
    if ((t & 63u) >= static_cast<uint32_t>(off)) incl += up;
  }
  if ((t & 63u) == 63u) waves[t >> 6] = incl;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w)
  {
    const uint32_t c = waves[w];
    if (w < (t >> 6)) base += c;
    all += c;
  }
  __syncthreads();
  *total = all;
  return base + incl - v;
}

__global__ void __launch_bounds__(kThreads) build_small_kernel(const SmallBuildArgs a)
{
  extern __shared__ __align__(16) unsigned char lds[];
  uint16_t * keys = reinterpret_cast<uint16_t *>(lds + kOffKeys);
  uint16_t * val_a = reinterpret_cast<uint16_t *>(lds + kOffValA);
  uint16_t * val_b = reinterpret_cast<uint16_t *>(lds + kOffValB);
  uint16_t * cnt = reinterpret_cast<uint16_t *>(lds + kOffCnt);
  uint32_t * waves = reinterpret_cast<uint32_t *>(lds + kOffWaves);

  const uint32_t t = threadIdx.x;
  const uint32_t n = a.n_points;
  const uint32_t ncell = a.grid.ncell;
  double2 * world = reinterpret_cast<double2 *>(a.world_xy);

  // ---- 1. keys ----
  uint32_t * first_lds = reinterpret_cast<uint32_t *>(val_b);
  const bool first_in_lds = a.n_scans <= kFirstInLds;
  if (first_in_lds)
  {
    for (uint32_t k = t; k < a.n_scans; k += kThreads) first_lds[k] = a.scans[k].first;
  }
  __syncthreads();
  for (uint32_t i = t; i < n; i += kThreads)
  {
    // which scan does point i belong to: last k with first[k] <= i
    uint32_t lo = 0, hi = a.n_scans;
    while (hi - lo > 1)
    {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t f = first_in_lds ? first_lds[mid] : a.scans[mid].first;
      if (f <= i) lo = mid; else hi = mid;
    }
    const SmallScan sc = a.scans[lo];
    const double2 p = reinterpret_cast<const double2 *>(a.pool_xy)[static_cast<size_t>(sc.pool_offset) + (i - sc.first)];
    // p(0) = pose.x; p(0) += point.x * cos_th - point.y * sin_th (src/ndt_model.cpp:139-141)
    const double wx = sc.x + (p.x * sc.c - p.y * sc.s);
    const double wy = sc.y + (p.x * sc.s + p.y * sc.c);
    world[i] = double2{wx, wy};
    const uint32_t key = a.grid.pow2 ? cell_index<true>(a.grid, wx, wy) : cell_index<false>(a.grid, wx, wy);
    keys[i] = static_cast<uint16_t>(key);
  }
  __syncthreads();

  // ---- 2. stable radix sort of the point indices by key ----
  // Thread t owns the positions [pb, pe) of every pass: a digit's counters are scanned in thread
  // order, a thread places its own items in position order, so equal keys keep their order.
  const uint32_t per_thread = (n + kThreads - 1) / kThreads;
  const uint32_t pb = min(n, t * per_thread), pe = min(n, pb + per_thread);
  uint16_t * src = val_b, * dst = val_a;
  for (uint32_t pass = 0; pass < a.sort_passes; ++pass)
  {
    const uint32_t shift = 4u * pass;
#pragma unroll
    for (uint32_t d = 0; d < kDigits; ++d) cnt[d * kThreads + t] = 0;
    for (uint32_t j = pb; j < pe; ++j)
    {
      const uint32_t idx = pass == 0u ? j : src[j];
      const uint32_t d = (keys[idx] >> shift) & (kDigits - 1u);
      cnt[d * kThreads + t] = static_cast<uint16_t>(cnt[d * kThreads + t] + 1u);
    }
    __syncthreads();
    // the counters in (digit, thread) order are one linear array: 16 consecutive ones per thread
    uint32_t c[kDigits], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kDigits; ++k)
    {
      c[k] = cnt[t * kDigits + k];
      sum += c[k];
    }
    uint32_t total;
    uint32_t run = block_exclusive_scan(sum, waves, &total);
#pragma unroll
    for (uint32_t k = 0; k < kDigits; ++k)
    {
      cnt[t * kDigits + k] = static_cast<uint16_t>(run);
      run += c[k];
    }
    __syncthreads();
    for (uint32_t j = pb; j < pe; ++j)
    {
      const uint32_t idx = pass == 0u ? j : src[j];
      const uint32_t d = (keys[idx] >> shift) & (kDigits - 1u);
      const uint32_t pos = cnt[d * kThreads + t];
      cnt[d * kThreads + t] = static_cast<uint16_t>(pos + 1u);
      dst[pos] = static_cast<uint16_t>(idx);
    }
    __syncthreads();
    uint16_t * const tmp = src;
    src = dst;
    dst = tmp;
  }
  const uint16_t * vals = src;     // sorted point indices (a.sort_passes >= 1)

  // ---- 3. segment heads: the touched cells ----
  uint16_t * seg = cnt;            // seg[k]: first sorted position of the k-th segment; seg[segments] = n
  uint32_t heads = 0;
  for (uint32_t j = pb; j < pe; ++j) heads += (j == 0u || keys[vals[j - 1]] != keys[vals[j]]) ? 1u : 0u;
  uint32_t n_seg;
  uint32_t h = block_exclusive_scan(heads, waves, &n_seg);
  for (uint32_t j = pb; j < pe; ++j)
  {
    if (j == 0u || keys[vals[j - 1]] != keys[vals[j]]) seg[h++] = static_cast<uint16_t>(j);
  }
  if (t == 0) seg[n_seg] = static_cast<uint16_t>(n);
  __syncthreads();
  // (the points off the grid, key ncell, are the last segment: not a cell)
  const uint32_t n_touched = (n_seg > 0u && keys[vals[n - 1]] == ncell) ? n_seg - 1u : n_seg;
  if (t == 0) *a.n_touched_out = n_touched;

  // ---- 4. addPoint in the reference's order, Cell::compute, the list ----
  const uint32_t q = t & 7u;
  const uint32_t lane_base = (t & 63u) & ~7u;
  for (uint32_t k = t >> 3; k < n_touched; k += kThreads / 8)
  {
    const uint32_t b = seg[k], e = seg[k + 1];
    double cnt_n = 0.0, v = 0.0;
    if (q < 5u)
    {
      // (the gather of the points eight ahead of the chain, as cell_sums_kernel has it)
      constexpr uint32_t kBatch = 8;
      uint32_t j = b;
      for (; j + kBatch <= e; j += kBatch)
      {
        double2 p[kBatch];
#pragma unroll
        for (uint32_t u = 0; u < kBatch; ++u) p[u] = world[vals[j + u]];
#pragma unroll
        for (uint32_t u = 0; u < kBatch; ++u)
        {
          v = add_point_quantity(q, p[u], v, cnt_n);
          cnt_n += 1;
        }
      }
      for (; j < e; ++j)
      {
        v = add_point_quantity(q, world[vals[j]], v, cnt_n);
        cnt_n += 1;
      }
    }
    const double mean_x = __shfl(v, static_cast<int>(lane_base + 0u), 64);
    const double mean_y = __shfl(v, static_cast<int>(lane_base + 1u), 64);
    const double cxx = __shfl(v, static_cast<int>(lane_base + 2u), 64);
    const double cxy = __shfl(v, static_cast<int>(lane_base + 3u), 64);
    const double cyy = __shfl(v, static_cast<int>(lane_base + 4u), 64);
    if (q == 0u)
    {
      double ixx, ixy, iyy;
      cell_compute(a.eigen_form, cnt_n, mean_x, mean_y, cxx, cxy, cyy, &ixx, &ixy, &iyy);
      double2 * c6 = reinterpret_cast<double2 *>(a.list_cells6 + static_cast<size_t>(k) * 6);
      c6[0] = double2{mean_x, mean_y};
      c6[1] = double2{ixx, ixy};
      c6[2] = double2{iyy, cnt_n};
      a.list_index[k] = keys[vals[b]];
    }
  }
}

hipError_t launch_build_small(const SmallBuildArgs & args, hipStream_t stream)
{
  const uint32_t ncell = args.grid.ncell;
  if (args.n_points > kFusedMaxPoints || ncell >= 65535u || ncell == 0u || args.n_scans == 0u)
  {
    return hipErrorInvalidValue;
  }
  SmallBuildArgs a = args;
  // passes over the bits of the largest key, ncell ("off the grid")
  uint32_t key_bits = 1;
  while ((1u << key_bits) <= ncell) ++key_bits;
  a.sort_passes = (key_bits + 3u) / 4u;
  // (no static LDS in front of the arrays: prepare_absolute_lds_kernel, ndt2d_kernels.h)
  const hipError_t e = prepare_absolute_lds_kernel(reinterpret_cast<const void *>(build_small_kernel), kLdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(build_small_kernel, dim3(1), dim3(kThreads), kLdsBytes, stream, a);
  return hipGetLastError();
}

// The grid ScanMatcherNDT::addScans gives a map (reference src/scan_matcher_ndt.cpp:52-66): the
// scan poses +- range_max; max_x_ / max_y_ start at numeric_limits<double>::min() as the reference
// has it.  NDT::NDT (src/ndt_model.cpp:118-126): size_x_ = (size_t)(size_x / cell_size + 1).  The
// arithmetic of ndt2d_build_grid.  Geometry fields of *g only; false: degenerate extent.
bool addscans_geometry(double ndt_resolution, double range_max, const double * poses_xyt, size_t n_scans,
                       GridDesc * g)
{
  double min_x = std::numeric_limits<double>::max(), max_x = std::numeric_limits<double>::min();
  double min_y = std::numeric_limits<double>::max(), max_y = std::numeric_limits<double>::min();
  for (size_t k = 0; k < n_scans; ++k)
  {
    min_x = std::min(poses_xyt[3 * k] - range_max, min_x);
    max_x = std::max(poses_xyt[3 * k] + range_max, max_x);
    min_y = std::min(poses_xyt[3 * k + 1] - range_max, min_y);
    max_y = std::max(poses_xyt[3 * k + 1] + range_max, max_y);
  }
  const double fsx = ((max_x - min_x) / ndt_resolution) + 1;
  const double fsy = ((max_y - min_y) / ndt_resolution) + 1;
  if (!(fsx >= 1.0) || !(fsy >= 1.0) || fsx * fsy >= 2147483648.0) return false;
  *g = GridDesc{};
  g->size_x = static_cast<uint32_t>(static_cast<size_t>(fsx));
  g->size_y = static_cast<uint32_t>(static_cast<size_t>(fsy));
  g->ncell = g->size_x * g->size_y;
  g->cell_size = ndt_resolution;
  int exponent = 0;
  // (a power of two whose reciprocal is a normal number, as the context's installs decide it)
  g->pow2 = (std::isfinite(ndt_resolution) && std::frexp(ndt_resolution, &exponent) == 0.5 &&
             std::fpclassify(ndt_resolution) == FP_NORMAL && std::fpclassify(1.0 / ndt_resolution) == FP_NORMAL) ? 1 : 0;
  g->inv_cell_size = 1.0 / ndt_resolution;
  g->origin_x = min_x;
  g->origin_y = min_y;
  return true;
}

bool small_map_fits(const GridDesc & g, size_t n_points)
{
  return n_points <= kFusedMaxPoints && g.ncell < 65535u;
}

}  // namespace

}  // namespace ndt2d

// ---- the scan store and the C entry points ----

// Scans kept on the device, and what a build needs beside them: an object of its own beside the
// context, which it reaches through the public boundary only.
struct ndt2d_scanstore
{
  ndt2d_handle h = nullptr;
  int device = 0;
  std::string err;
  // [capacity_points resident | kFusedMaxPoints scratch for a build from host points][2]
  double * pool = nullptr;
  size_t capacity_points = 0, capacity_scans = 0;
  size_t used_points = 0;
  std::vector<uint32_t> offset, count;   // of scan `id`, in points
  std::vector<uint32_t> job;             // a build's {offset | count} per scan
  int eigen_form = 0;                    // ndt2d_eigen2.h
  double * world = nullptr;              // [kFusedMaxPoints][2] scratch
  double * pinned = nullptr;             // staging of a build: [scan table | host points]
  size_t pinned_cap = 0;                 // doubles
  double * table = nullptr;              // device copy of the scan table
  size_t table_cap = 0;                  // doubles
  uint32_t * n_touched = nullptr;        // pinned word the kernel leaves the list's length in
  uint32_t * n_touched_dev = nullptr;    // ... as the device addresses it
  double * list = nullptr;               // the list on the device, when the context's staging buffer
  size_t list_cap = 0;                   // cannot be addressed by the device (cells)
};

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
