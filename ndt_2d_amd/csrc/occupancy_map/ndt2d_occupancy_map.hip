// OccupancyGrid with resident scans and counts (include/ndt2d_hip.h, "OccupancyGrid with
// resident scans and counts"; reference src/occupancy_grid.cpp:37-185).  The node publishes the
// map after every scan (src/ndt_mapper.cpp:545,691-703) with the whole scan vector; the counts
// are integers, so adding the new scans' rays to the counters of the last publish gives exactly
// the map a full re-trace gives.  This object keeps what that needs on the device:
//
//   points      every appended scan's robot-frame points, append-only, grown by doubling
//   offsets     first point of scan k, [n + 1]
//   scan table  {pose x, pose y, cos, sin} per scan, as of the last update
//   counts      hit << 32 | empty per cell, persistent between updates
//   data        the int8 map
//
//   map_bounds_kernel    updateBounds (:154-178) over the points of the scans [first, n): the
//                        transform expression of ndt2d_occupancy.hip's bounds_kernel; a launch of
//                        one block writes the pinned read-back block itself
//   map_bounds_fold_kernel   folds the per-block partials into the pinned block
//   map_trace_kernel     the ray loop (:73-131) of the points [first_point, n_points), ADDED to
//                        the counters; rays_kernel's rules (a cell outside the grid is skipped,
//                        ++empty and ++hit of one cell are one add)
//   map_finalize_kernel  (:134-150) -1 / 0 / 100 over a rectangle of the row-major map
//
// Beams to lanes: consecutive beams of a scan on consecutive lanes, as in rays_kernel.  A visit is
// one 8-byte no-return atomic executed at the L2 / memory side; what a wave instruction costs there
// grows with the number of distinct 64-byte lines it touches, and neighbouring beams leave the pose
// through the same or adjacent cells, so this mapping keeps the lines per instruction low where the
// sharing is densest (a strided mapping would touch up to 64 lines per instruction from the first
// step on).  One new scan is 720 rays: its trace is a few waves and is bounded by the longest ray,
// not by atomic throughput.
//
// The object is beside the device context, not in it (particles/ndt2d_device_object.h): it reaches
// the context through ndt2d_get_stream and ndt2d_device_id only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "ndt2d_kernels.h"
#include "particles/ndt2d_device_object.h"

using namespace ndt2d::object;

namespace
{

constexpr int kWave = 64;
constexpr uint32_t kMaxBoundsBlocks = 1024;
constexpr size_t kInitialPoints = 1u << 14;
constexpr size_t kInitialScans = 256;

struct ScanRec
{
  double x, y, c, s;  // pose translation, cos / sin of pose theta (host libm, :78-79,163-164)
};

struct MapArgs
{
  const double2 * points;     // [n_points] robot frame, scans concatenated
  const uint32_t * offsets;   // [n_scans + 1]
  const ScanRec * scans;      // [n_scans]
  uint32_t first_scan, n_scans;
  uint32_t first_point, n_points;
  double resolution, origin_x, origin_y;
  uint32_t width, height;
};

// last k in [first_scan, n_scans) with offsets[k] <= i
__device__ __forceinline__ uint32_t scan_of_point(const MapArgs & a, uint32_t i)
{
  uint32_t lo = a.first_scan, hi = a.n_scans;
  while (hi - lo > 1)
  {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void store_host(double * p, double v)
{
  // the pinned block, written through at system scope (a vector store)
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// {min_x, max_x, min_y, max_y} of the map-frame points [first_point, n_points): per block into
// partials[block][4], or, from a launch of one block, straight into out[4]
__global__ void __launch_bounds__(256) map_bounds_kernel(const MapArgs a, double * partials,
                                                         double * out)
{
  __shared__ double sh[4][4];
  double mn_x = HUGE_VAL, mx_x = -HUGE_VAL, mn_y = HUGE_VAL, mx_y = -HUGE_VAL;
  for (uint32_t i = a.first_point + blockIdx.x * 256 + threadIdx.x; i < a.n_points;
       i += gridDim.x * 256)
  {
    const ScanRec sc = a.scans[scan_of_point(a, i)];
    const double2 p = a.points[i];
    // Point p(x, y); p.x += point.x * cos_th - point.y * sin_th (:171-173)
    const double px = sc.x + (p.x * sc.c - p.y * sc.s);
    const double py = sc.y + (p.x * sc.s + p.y * sc.c);
    mn_x = fmin(mn_x, px);
    mx_x = fmax(mx_x, px);
    mn_y = fmin(mn_y, py);
    mx_y = fmax(mx_y, py);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
  {
    mn_x = fmin(mn_x, __shfl_xor(mn_x, off, kWave));
    mx_x = fmax(mx_x, __shfl_xor(mx_x, off, kWave));
    mn_y = fmin(mn_y, __shfl_xor(mn_y, off, kWave));
    mx_y = fmax(mx_y, __shfl_xor(mx_y, off, kWave));
  }
  if ((threadIdx.x & (kWave - 1)) == 0)
  {
    const int w = threadIdx.x >> 6;
    sh[w][0] = mn_x;
    sh[w][1] = mx_x;
    sh[w][2] = mn_y;
    sh[w][3] = mx_y;
  }
  __syncthreads();
  if (threadIdx.x < 4)
  {
    const int k = threadIdx.x;
    const double v = (k & 1) ? fmax(fmax(sh[0][k], sh[1][k]), fmax(sh[2][k], sh[3][k]))
                             : fmin(fmin(sh[0][k], sh[1][k]), fmin(sh[2][k], sh[3][k]));
    if (gridDim.x == 1)
    {
      store_host(out + k, v);
    }
    else
    {
      partials[static_cast<size_t>(blockIdx.x) * 4 + k] = v;
    }
  }
}

__global__ void __launch_bounds__(256) map_bounds_fold_kernel(const double * partials,
                                                              uint32_t n_blocks, double * out)
{
  __shared__ double sh[4][4];
  double v[4] = {HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL};
  for (uint32_t b = threadIdx.x; b < n_blocks; b += 256)
  {
    const double * p = partials + static_cast<size_t>(b) * 4;
    v[0] = fmin(v[0], p[0]);
    v[1] = fmax(v[1], p[1]);
    v[2] = fmin(v[2], p[2]);
    v[3] = fmax(v[3], p[3]);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1)
  {
    v[0] = fmin(v[0], __shfl_xor(v[0], off, kWave));
    v[1] = fmax(v[1], __shfl_xor(v[1], off, kWave));
    v[2] = fmin(v[2], __shfl_xor(v[2], off, kWave));
    v[3] = fmax(v[3], __shfl_xor(v[3], off, kWave));
  }
  if ((threadIdx.x & (kWave - 1)) == 0)
  {
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 4)
  {
    const int k = threadIdx.x;
    const double r = (k & 1) ? fmax(fmax(sh[0][k], sh[1][k]), fmax(sh[2][k], sh[3][k]))
                             : fmin(fmin(sh[0][k], sh[1][k]), fmin(sh[2][k], sh[3][k]));
    store_host(out + k, r);
  }
}

// One beam per thread; counts[cell] += hit << 32 | empty.  Nothing is cleared here.
__global__ void __launch_bounds__(256) map_trace_kernel(const MapArgs a, unsigned long long * counts)
{
  const uint32_t i = a.first_point + blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_points) return;
  const ScanRec sc = a.scans[scan_of_point(a, i)];
  const double2 p = a.points[i];
  // :82-83 (double -> int truncates toward zero)
  const int start_x = static_cast<int>((sc.x - a.origin_x) / a.resolution);
  const int start_y = static_cast<int>((sc.y - a.origin_y) / a.resolution);
  // :87-91
  const double point_x = p.x * sc.c - p.y * sc.s + sc.x;
  const double point_y = p.x * sc.s + p.y * sc.c + sc.y;
  const int end_x = static_cast<int>((point_x - a.origin_x) / a.resolution);
  const int end_y = static_cast<int>((point_y - a.origin_y) / a.resolution);
  // :93-98
  const int dx = abs(end_x - start_x);
  const int sx = (start_x < end_x) ? 1 : -1;
  const int dy = -abs(end_y - start_y);
  const int sy = (start_y < end_y) ? 1 : -1;
  int error = dx + dy;
  int x = start_x, y = start_y;
  const unsigned long long kHit = 1ull << 32, kEmpty = 1ull;
  while (true)
  {
    // a cell outside the grid is skipped (the reference would write out of bounds)
    const bool inside = x >= 0 && y >= 0 && static_cast<uint32_t>(x) < a.width &&
                        static_cast<uint32_t>(y) < a.height;
    unsigned long long * cell =
      counts + (inside ? static_cast<size_t>(x) + static_cast<size_t>(y) * a.width : 0);
    if (x == end_x && y == end_y)
    {
      if (inside) atomicAdd(cell, kHit);
      break;
    }
    unsigned long long add = kEmpty;
    bool done = false;
    if (2 * error >= dy)
    {
      if (x == end_x)
      {
        add += kHit;  // ++empty and ++hit of the same cell (:111,116)
        done = true;
      }
      else
      {
        error = error + dy;
        x += sx;
      }
    }
    if (!done && 2 * error <= dx)
    {
      if (y == end_y)
      {
        add += kHit;
        done = true;
      }
      else
      {
        error = error + dx;
        y += sy;
      }
    }
    if (inside) atomicAdd(cell, add);
    if (done) break;
  }
}

struct CellRect
{
  uint32_t x0, y0, w, h;
};

// the cells of `r` (inside the map: checked by the host) of the row-major map
__global__ void __launch_bounds__(256) map_finalize_kernel(const unsigned long long * counts,
                                                           uint32_t width, CellRect r,
                                                           double occ_thresh, signed char * data)
{
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<size_t>(r.w) * r.h) return;
  const uint32_t row = static_cast<uint32_t>(i / r.w);
  const uint32_t col = static_cast<uint32_t>(i - static_cast<size_t>(row) * r.w);
  const size_t cell = static_cast<size_t>(r.y0 + row) * width + r.x0 + col;
  const unsigned long long c = counts[cell];
  const int hit = static_cast<int>(c >> 32), empty = static_cast<int>(c & 0xffffffffull);
  // :136-149
  const double touches = hit + empty;
  signed char v = -1;
  if (touches > 0.5) v = (static_cast<double>(hit) / touches > occ_thresh) ? 100 : 0;
  data[cell] = v;
}

}  // namespace

struct ndt2d_occupancy_map : DeviceObject
{
  double resolution = 0.0, occ_thresh = 0.0;

  // resident scans
  double * d_points = nullptr;      // [points_cap][2]
  size_t points_cap = 0;
  uint32_t * d_offsets = nullptr;   // [scans_cap + 1]
  ScanRec * d_scans = nullptr;      // [scans_cap]
  size_t scans_cap = 0;
  std::vector<uint32_t> offsets{0};   // host copy, [appended + 1]
  bool nonfinite_points = false;    // some appended point is NaN / inf: no rectangle is derived
  std::vector<unsigned char> scan_nonfinite;

  // counters and map
  unsigned long long * d_counts = nullptr;
  signed char * d_data = nullptr;
  size_t cells_cap = 0;
  double * d_partials = nullptr;    // [kMaxBoundsBlocks][4]
  double * pinned = nullptr;        // [4] bounds read-back
  double * pinned_dev = nullptr;

  // the generator (:37-43)
  double bounds[4] = {0.0, 0.0, 0.0, 0.0};
  size_t num_scans = 0;

  // the last update
  bool counts_valid = false;        // counts == the rays of scans [0, num_scans) at `poses`, on `geo`
  bool have_map = false;            // d_data holds the map of `geo`
  ndt2d_occupancy_info geo{};
  std::vector<double> poses;        // [num_scans][3] of the last update
  bool table_stale = false;         // the device scan table is not the one made from `poses`
  std::vector<ScanRec> stage;

  StreamUse use;
};

namespace
{

// after a failed HIP call (DeviceObject::hip_failed): whatever was in flight may not have happened
void invalidate(DeviceObject * o)
{
  ndt2d_occupancy_map * m = static_cast<ndt2d_occupancy_map *>(o);
  m->counts_valid = false;
  m->have_map = false;
  m->table_stale = true;
}

void release(ndt2d_occupancy_map * m)
{
  (void)hipFree(m->d_points);
  (void)hipFree(m->d_offsets);
  (void)hipFree(m->d_scans);
  (void)hipFree(m->d_counts);
  (void)hipFree(m->d_data);
  (void)hipFree(m->d_partials);
  if (m->pinned != nullptr) (void)hipHostFree(m->pinned);
  (void)hipGetLastError();
  delete m;
}

// room for `need` points / scans: double, copy device to device, release the old block
template <typename T>
int grow(ndt2d_occupancy_map * m, T ** buf, size_t * cap, size_t need, size_t keep, size_t extra,
         hipStream_t stream)
{
  if (need <= *cap) return NDT2D_OK;
  size_t cap_new = *cap;
  while (cap_new < need) cap_new *= 2;
  T * fresh = nullptr;
  NDT2D_OBJ_HIP(m, hipMalloc(reinterpret_cast<void **>(&fresh), (cap_new + extra) * sizeof(T)));
  hipError_t e = hipSuccess;
  if (keep > 0) e = hipMemcpyAsync(fresh, *buf, keep * sizeof(T), hipMemcpyDeviceToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);   // nothing in flight reads the old block
  if (e != hipSuccess)
  {
    (void)hipFree(fresh);
    return fail_hip(m, e, "growing a resident buffer");
  }
  (void)hipFree(*buf);
  *buf = fresh;
  *cap = cap_new;
  return NDT2D_OK;
}

bool same_bits(const double * a, const double * b, size_t n)
{
  return n == 0 || std::memcmp(a, b, n * sizeof(double)) == 0;
}

// static_cast<int>((v - origin) / resolution) as the device converts it (saturating, NaN -> 0)
long long cell_of(double v, double origin, double resolution)
{
  const double q = (v - origin) / resolution;
  if (!(q == q)) return 0;
  if (q >= 2147483647.0) return 2147483647ll;
  if (q <= -2147483648.0) return -2147483648ll;
  return static_cast<long long>(static_cast<int>(q));
}

void launch_finalize(const ndt2d_occupancy_map * m, const CellRect & r, hipStream_t stream)
{
  const size_t n = static_cast<size_t>(r.w) * r.h;
  hipLaunchKernelGGL(map_finalize_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0,
                     stream, m->d_counts, m->geo.width, r, m->occ_thresh, m->d_data);
}

void forget(ndt2d_occupancy_map * m)
{
  m->offsets.assign(1, 0);
  m->scan_nonfinite.clear();
  m->nonfinite_points = false;
  for (double & b : m->bounds) b = 0.0;
  m->num_scans = 0;
  m->counts_valid = false;
  m->have_map = false;
  m->poses.clear();
  m->table_stale = false;
}

}  // namespace

extern "C" {

int ndt2d_occmap_create(ndt2d_handle h, double resolution, double occ_thresh,
                        ndt2d_occupancy_map ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr || !(resolution > 0.0) || !(resolution < HUGE_VAL)) return NDT2D_ERR_INVALID;
  ndt2d_occupancy_map * m = new ndt2d_occupancy_map();
  m->h = h;
  m->device = ndt2d_device_id(h);
  m->hip_failed = invalidate;
  m->resolution = resolution;
  m->occ_thresh = occ_thresh;
  hipError_t e = hipSetDevice(m->device);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->d_points), kInitialPoints * 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->d_offsets), (kInitialScans + 1) * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->d_scans), kInitialScans * sizeof(ScanRec));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->d_partials), kMaxBoundsBlocks * 4 * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&m->pinned), 4 * sizeof(double),
                                               hipHostMallocCoherent | hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&m->pinned_dev), m->pinned, 0);
  if (e == hipSuccess) e = hipMemset(m->d_offsets, 0, sizeof(uint32_t));
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    release(m);
    return NDT2D_ERR_HIP;
  }
  m->points_cap = kInitialPoints;
  m->scans_cap = kInitialScans;
  *out = m;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_occmap_destroy(ndt2d_occupancy_map * m)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(m->device);
  if (m->use.used) (void)hipStreamSynchronize(m->use.last_stream);
  release(m);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_occmap_last_error(ndt2d_occupancy_map * m) { return m != nullptr ? m->err.c_str() : ""; }

int ndt2d_occmap_append_scan(ndt2d_occupancy_map * m, const double * points_xy, size_t n_points,
                             size_t * scan_id_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_points > 0 && points_xy == nullptr) return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_append_scan: null points");
  const size_t n_scans = m->offsets.size() - 1;
  const size_t first = m->offsets.back();
  // point indices are 32-bit words on the device (as in ndt2d_occupancy_grid)
  if (n_points >= (1ull << 31) || first + n_points >= (1ull << 31) || n_scans >= (1u << 30))
  {
    return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_append_scan: too many points or scans");
  }
  hipStream_t stream;
  int rc = current_stream(m, &m->use, &stream);
  if (rc != NDT2D_OK) return rc;
  // (the doubled blocks hold [cap][2] doubles and [cap + 1] offsets)
  {
    size_t cap2 = 2 * m->points_cap;
    if ((rc = grow(m, &m->d_points, &cap2, 2 * (first + n_points), 2 * first, 0, stream)) != NDT2D_OK) return rc;
    m->points_cap = cap2 / 2;
    size_t cap_s = m->scans_cap;
    if ((rc = grow(m, &m->d_offsets, &cap_s, n_scans + 1, n_scans + 1, 1, stream)) != NDT2D_OK) return rc;
    size_t cap_r = m->scans_cap;
    const size_t in_table = std::min(m->poses.size() / 3, n_scans);
    if ((rc = grow(m, &m->d_scans, &cap_r, n_scans + 1, in_table, 0, stream)) != NDT2D_OK) return rc;
    m->scans_cap = cap_s;
  }
  bool nonfinite = false;
  for (size_t i = 0; i < 2 * n_points; ++i) nonfinite = nonfinite || !std::isfinite(points_xy[i]);
  const uint32_t end = static_cast<uint32_t>(first + n_points);
  if (n_points > 0)
  {
    NDT2D_OBJ_HIP(m, hipMemcpyAsync(m->d_points + 2 * first, points_xy, 2 * n_points * sizeof(double),
                                 hipMemcpyHostToDevice, stream));
  }
  NDT2D_OBJ_HIP(m, hipMemcpyAsync(m->d_offsets + n_scans + 1, &end, sizeof(uint32_t), hipMemcpyHostToDevice,
                               stream));
  NDT2D_OBJ_HIP(m, hipStreamSynchronize(stream));   // the caller's array is free again
  m->offsets.push_back(end);
  m->scan_nonfinite.push_back(nonfinite ? 1 : 0);
  m->nonfinite_points = m->nonfinite_points || nonfinite;
  if (scan_id_out != nullptr) *scan_id_out = n_scans;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_occmap_scan_count(ndt2d_occupancy_map * m, size_t * n_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (n_out == nullptr) return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_scan_count: null argument");
  *n_out = m->offsets.size() - 1;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_occmap_reset(ndt2d_occupancy_map * m)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (m->use.used)
  {
    NDT2D_OBJ_HIP(m, hipSetDevice(m->device));
    NDT2D_OBJ_HIP(m, hipStreamSynchronize(m->use.last_stream));
  }
  forget(m);
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_occmap_update(ndt2d_occupancy_map * m, const double * poses_xyt, size_t n_scans,
                        ndt2d_occmap_result * result)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (result == nullptr || (n_scans > 0 && poses_xyt == nullptr))
  {
    return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_update: null argument");
  }
  // 1.
  if (n_scans > m->offsets.size() - 1)
  {
    return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_update: more scans than were appended");
  }
  if (n_scans < m->num_scans)
  {
    return fail(m, NDT2D_ERR_INVALID,
                 "ndt2d_occmap_update: fewer scans than the last update rendered (ndt2d_occmap_reset drops scans)");
  }
  hipStream_t stream;
  int rc = current_stream(m, &m->use, &stream);
  if (rc != NDT2D_OK) return rc;

  const size_t n_old = m->num_scans;
  const bool old_poses_same = m->poses.size() >= 3 * n_old && same_bits(poses_xyt, m->poses.data(), 3 * n_old);
  const bool table_same = !m->table_stale && m->poses.size() == 3 * n_scans &&
                          same_bits(poses_xyt, m->poses.data(), 3 * n_scans);

  // the device scan table: every record whose pose differs from what it was made from (after an
  // INCREMENTAL or UNCHANGED update: the new scans' records only)
  bool uploaded = false;
  if (!table_same)
  {
    size_t first_rec = 0;
    if (old_poses_same && !m->table_stale) first_rec = n_old;
    m->stage.resize(n_scans - first_rec);
    for (size_t k = first_rec; k < n_scans; ++k)
    {
      ScanRec & r = m->stage[k - first_rec];
      r.x = poses_xyt[3 * k];
      r.y = poses_xyt[3 * k + 1];
      ndt2d_cos_sin(poses_xyt[3 * k + 2], &r.c, &r.s);   // :78-79,163-164, host libm
    }
    if (n_scans > first_rec)
    {
      NDT2D_OBJ_HIP(m, hipMemcpyAsync(m->d_scans + first_rec, m->stage.data(),
                                   (n_scans - first_rec) * sizeof(ScanRec), hipMemcpyHostToDevice, stream));
      uploaded = true;
    }
    // (`poses`, what the counters were made from, is kept until the update is accepted)
    m->table_stale = first_rec < n_old;
  }

  MapArgs args{};
  args.points = reinterpret_cast<const double2 *>(m->d_points);
  args.offsets = m->d_offsets;
  args.scans = m->d_scans;
  args.n_scans = static_cast<uint32_t>(n_scans);
  args.n_points = m->offsets[n_scans];
  args.resolution = m->resolution;

  // 2. updateBounds (:154-185), only when the scan count changed (:51-54)
  double bounds[4] = {m->bounds[0], m->bounds[1], m->bounds[2], m->bounds[3]};
  double found[4] = {HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL};
  const uint32_t first_new_point = m->offsets[n_old];
  const uint32_t n_new_points = args.n_points - first_new_point;
  int status = NDT2D_OK;
  const char * refusal = nullptr;
  if (n_scans != n_old)
  {
    if (n_new_points > 0)
    {
      args.first_scan = static_cast<uint32_t>(n_old);
      args.first_point = first_new_point;
      uint32_t blocks = (n_new_points + 255) / 256;
      if (blocks > kMaxBoundsBlocks) blocks = kMaxBoundsBlocks;
      hipLaunchKernelGGL(map_bounds_kernel, dim3(blocks), dim3(256), 0, stream, args, m->d_partials,
                         m->pinned_dev);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess && blocks > 1)
      {
        hipLaunchKernelGGL(map_bounds_fold_kernel, dim3(1), dim3(256), 0, stream, m->d_partials, blocks,
                           m->pinned_dev);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) return fail_hip(m, e, "ndt2d_occmap_update: bounds");
      uploaded = false;   // (the staged records have arrived)
      for (int k = 0; k < 4; ++k) found[k] = static_cast<const volatile double *>(m->pinned)[k];
    }
    const double resolution = m->resolution;
    const double min_x = std::min(found[0], bounds[0]);
    const double max_x = std::max(found[1], bounds[1]);
    const double min_y = std::min(found[2], bounds[2]);
    const double max_y = std::max(found[3], bounds[3]);
    // :181-184
    bounds[0] = std::floor(min_x / resolution) * resolution;
    bounds[1] = std::ceil(max_x / resolution) * resolution;
    bounds[2] = std::floor(min_y / resolution) * resolution;
    bounds[3] = std::ceil(max_y / resolution) * resolution;
  }

  // 3. :57-65 (info.width / height are uint32: the quotient is truncated)
  ndt2d_occupancy_info geo{};
  {
    const double resolution = m->resolution;
    const double pad = 5 * resolution;
    const double fw = (bounds[1] - bounds[0] + 2 * pad) / resolution;
    const double fh = (bounds[3] - bounds[2] + 2 * pad) / resolution;
    if (!(fw >= 0.0) || !(fh >= 0.0) || fw >= 2147483648.0 || fh >= 2147483648.0 ||
        fw * fh >= 2147483648.0)
    {
      status = NDT2D_ERR_INVALID;
      refusal = "ndt2d_occmap_update: degenerate map extent";
    }
    else
    {
      geo.resolution = resolution;
      geo.width = static_cast<uint32_t>(fw);
      geo.height = static_cast<uint32_t>(fh);
      geo.origin_x = bounds[0] - pad;
      geo.origin_y = bounds[2] - pad;
    }
  }
  if (status != NDT2D_OK)
  {
    // refused: bounds, count, poses, counters and map stay as they were (a scan table written
    // over with the refused poses is marked stale above)
    if (uploaded) (void)hipStreamSynchronize(stream);
    return fail(m, status, refusal);
  }

  // 4.
  const bool geo_same = m->have_map && same_bits(&geo.origin_x, &m->geo.origin_x, 1) &&
                        same_bits(&geo.origin_y, &m->geo.origin_y, 1) && geo.width == m->geo.width &&
                        geo.height == m->geo.height;
  const bool keep = m->counts_valid && geo_same && old_poses_same;
  const int mode = !keep ? NDT2D_OCCMAP_FULL
                         : (n_scans > n_old ? NDT2D_OCCMAP_INCREMENTAL : NDT2D_OCCMAP_UNCHANGED);

  const size_t n_cells = static_cast<size_t>(geo.width) * geo.height;
  CellRect rect{0, 0, 0, 0};
  uint64_t beams = 0;
  args.width = geo.width;
  args.height = geo.height;
  args.origin_x = geo.origin_x;
  args.origin_y = geo.origin_y;

  // from here on the object describes the new state; a failing launch invalidates it (invalidate)
  m->bounds[0] = bounds[0];
  m->bounds[1] = bounds[1];
  m->bounds[2] = bounds[2];
  m->bounds[3] = bounds[3];
  m->num_scans = n_scans;
  m->geo = geo;
  m->poses.assign(poses_xyt, poses_xyt + 3 * n_scans);
  m->table_stale = false;

  if (mode == NDT2D_OCCMAP_FULL)
  {
    m->counts_valid = false;
    m->have_map = false;
    if (n_cells > m->cells_cap)
    {
      NDT2D_OBJ_HIP(m, hipStreamSynchronize(stream));
      (void)hipFree(m->d_counts);
      (void)hipFree(m->d_data);
      m->d_counts = nullptr;
      m->d_data = nullptr;
      m->cells_cap = 0;
      const size_t cap = n_cells + n_cells / 4;   // some room for a map that keeps growing
      NDT2D_OBJ_HIP(m, hipMalloc(reinterpret_cast<void **>(&m->d_counts), cap * sizeof(unsigned long long)));
      NDT2D_OBJ_HIP(m, hipMalloc(reinterpret_cast<void **>(&m->d_data), cap));
      m->cells_cap = cap;
    }
    if (n_cells > 0)
    {
      NDT2D_OBJ_HIP(m, hipMemsetAsync(m->d_counts, 0, n_cells * sizeof(unsigned long long), stream));
      if (args.n_points > 0)
      {
        args.first_scan = 0;
        args.first_point = 0;
        hipLaunchKernelGGL(map_trace_kernel, dim3((args.n_points + 255) / 256), dim3(256), 0, stream, args,
                           m->d_counts);
        NDT2D_OBJ_HIP(m, hipGetLastError());
      }
      rect = CellRect{0, 0, geo.width, geo.height};
      launch_finalize(m, rect, stream);
      NDT2D_OBJ_HIP(m, hipGetLastError());
    }
    beams = args.n_points;
    // the staged scan records must have left the host before the next update writes them
    NDT2D_OBJ_HIP(m, hipStreamSynchronize(stream));
  }
  else if (mode == NDT2D_OCCMAP_INCREMENTAL && n_new_points > 0)
  {
    // 7. the cell bounding box of the new scans' start and end cells, clipped
    bool whole = false;
    long long lo_x = cell_of(found[0], geo.origin_x, geo.resolution);
    long long hi_x = cell_of(found[1], geo.origin_x, geo.resolution);
    long long lo_y = cell_of(found[2], geo.origin_y, geo.resolution);
    long long hi_y = cell_of(found[3], geo.origin_y, geo.resolution);
    for (size_t k = n_old; k < n_scans; ++k)
    {
      if (m->offsets[k + 1] == m->offsets[k]) continue;   // no ray starts here
      const double * p = poses_xyt + 3 * k;
      if (m->scan_nonfinite[k] || !std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
      {
        whole = true;   // fmin / fmax drop a NaN: the reduction does not bound such a scan
        break;
      }
      const long long cx = cell_of(p[0], geo.origin_x, geo.resolution);
      const long long cy = cell_of(p[1], geo.origin_y, geo.resolution);
      lo_x = std::min(lo_x, cx);
      hi_x = std::max(hi_x, cx);
      lo_y = std::min(lo_y, cy);
      hi_y = std::max(hi_y, cy);
    }
    if (whole)
    {
      rect = CellRect{0, 0, geo.width, geo.height};
    }
    else
    {
      lo_x = std::max(lo_x, 0ll);
      lo_y = std::max(lo_y, 0ll);
      hi_x = std::min(hi_x, static_cast<long long>(geo.width) - 1);
      hi_y = std::min(hi_y, static_cast<long long>(geo.height) - 1);
      if (lo_x <= hi_x && lo_y <= hi_y)
      {
        rect = CellRect{static_cast<uint32_t>(lo_x), static_cast<uint32_t>(lo_y),
                        static_cast<uint32_t>(hi_x - lo_x + 1), static_cast<uint32_t>(hi_y - lo_y + 1)};
      }
    }
    if (n_cells > 0)
    {
      args.first_scan = static_cast<uint32_t>(n_old);
      args.first_point = first_new_point;
      hipLaunchKernelGGL(map_trace_kernel, dim3((n_new_points + 255) / 256), dim3(256), 0, stream, args,
                         m->d_counts);
      NDT2D_OBJ_HIP(m, hipGetLastError());
      if (rect.w > 0 && rect.h > 0)
      {
        launch_finalize(m, rect, stream);
        NDT2D_OBJ_HIP(m, hipGetLastError());
      }
    }
    beams = n_new_points;
  }
  else if (uploaded)
  {
    // new scans without a point: their records were staged and nothing waited for them yet
    NDT2D_OBJ_HIP(m, hipStreamSynchronize(stream));
  }
  m->counts_valid = true;
  m->have_map = true;

  result->info = geo;
  result->mode = mode;
  result->beams_traced = beams;
  result->rect_x0 = rect.x0;
  result->rect_y0 = rect.y0;
  result->rect_w = rect.w;
  result->rect_h = rect.h;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_occmap_read(ndt2d_occupancy_map * m, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                      signed char * out, size_t out_row_stride)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (!m->have_map) return fail(m, NDT2D_ERR_STATE, "ndt2d_occmap_read: no map (no update yet, or the last one failed)");
  if (static_cast<uint64_t>(x0) + w > m->geo.width || static_cast<uint64_t>(y0) + h > m->geo.height)
  {
    return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_read: the rectangle leaves the map");
  }
  if (w == 0 || h == 0) return NDT2D_OK;
  if (out == nullptr || out_row_stride < w)
  {
    return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_read: null output or a row stride below w");
  }
  hipStream_t stream;
  int rc = current_stream(m, &m->use, &stream);
  if (rc != NDT2D_OK) return rc;
  const signed char * src = m->d_data + static_cast<size_t>(y0) * m->geo.width + x0;
  if (w == m->geo.width && out_row_stride == w)
  {
    NDT2D_OBJ_HIP(m, hipMemcpyAsync(out, src, static_cast<size_t>(w) * h, hipMemcpyDeviceToHost, stream));
  }
  else
  {
    NDT2D_OBJ_HIP(m, hipMemcpy2DAsync(out, out_row_stride, src, m->geo.width, w, h, hipMemcpyDeviceToHost,
                                   stream));
  }
  NDT2D_OBJ_HIP(m, hipStreamSynchronize(stream));
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_occmap_device_map(ndt2d_occupancy_map * m, const signed char ** d_map, ndt2d_occupancy_info * info)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (d_map == nullptr || info == nullptr) return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_device_map: null argument");
  *d_map = nullptr;
  if (!m->have_map) return fail(m, NDT2D_ERR_STATE, "ndt2d_occmap_device_map: no map (no update yet, or the last one failed)");
  hipStream_t stream;
  const int rc = current_stream(m, &m->use, &stream);
  if (rc != NDT2D_OK) return rc;
  NDT2D_OBJ_HIP(m, hipStreamSynchronize(stream));   // the last update's trace and finalize are complete
  *d_map = m->d_data;
  *info = m->geo;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

int ndt2d_occmap_bounds(ndt2d_occupancy_map * m, double * bounds4_out, size_t * num_scans_out)
{
  NDT2D_C_TRY
  if (m == nullptr) return NDT2D_ERR_INVALID;
  if (bounds4_out == nullptr || num_scans_out == nullptr)
  {
    return fail(m, NDT2D_ERR_INVALID, "ndt2d_occmap_bounds: null argument");
  }
  for (int k = 0; k < 4; ++k) bounds4_out[k] = m->bounds[k];
  *num_scans_out = m->num_scans;
  return NDT2D_OK;
  NDT2D_C_CATCH(m)
}

}  // extern "C"
