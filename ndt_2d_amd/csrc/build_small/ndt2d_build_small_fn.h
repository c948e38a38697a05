// The workgroup of the fused small-map NDT build (ndt2d_build_small.hip: the header comment there
// describes the steps and the LDS layout), the grid geometry of ScanMatcherNDT::addScans and the
// scan store's state -- in a header so that the batched loop-closure build
// (../closure/ndt2d_closure.hip: one such workgroup per candidate map) runs the same code on the
// same stored scans.  Included by .hip translation units only; compiled with -ffp-contract=off.
#ifndef NDT2D_BUILD_SMALL_FN_H_
#define NDT2D_BUILD_SMALL_FN_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "ndt2d_build_fn.h"
#include "ndt2d_device_fn.h"
#include "ndt2d_hip.h"

namespace ndt2d
{

namespace fused
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

// The whole build of one map by one workgroup of kThreads threads; lds: kLdsBytes at LDS offset 0.
// Returns the number of touched cells (to every thread); the list is in global memory, written by
// the threads that computed it (a caller that reads it in the same workgroup puts a barrier first).
__device__ __forceinline__ uint32_t build_small_workgroup(const SmallBuildArgs & a, unsigned char * lds)
{
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
  return n_touched;
}

// passes of the radix sort over the bits of the largest key, ncell ("off the grid")
inline uint32_t sort_passes_for(uint32_t ncell)
{
  uint32_t key_bits = 1;
  while ((1u << key_bits) <= ncell) ++key_bits;
  return (key_bits + 3u) / 4u;
}

// The grid ScanMatcherNDT::addScans gives a map (reference src/scan_matcher_ndt.cpp:52-66): the
// scan poses +- range_max; max_x_ / max_y_ start at numeric_limits<double>::min() as the reference
// has it.  NDT::NDT (src/ndt_model.cpp:118-126): size_x_ = (size_t)(size_x / cell_size + 1).  The
// arithmetic of ndt2d_build_grid.  Geometry fields of *g only; false: degenerate extent.
inline bool addscans_geometry(double ndt_resolution, double range_max, const double * poses_xyt, size_t n_scans,
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

inline bool small_map_fits(const GridDesc & g, size_t n_points)
{
  return n_points <= kFusedMaxPoints && g.ncell < 65535u;
}

}  // namespace fused

}  // namespace ndt2d

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

#endif  // NDT2D_BUILD_SMALL_FN_H_
