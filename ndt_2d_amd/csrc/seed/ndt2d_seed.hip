// Global localisation's seeder (include/ndt2d_hip.h, "Global localisation"): particles uniform over
// the free cells of an occupancy map with a uniform heading, and the replacement of a share of a set
// by fresh such particles.  The arithmetic of a sample is seed/ndt2d_seed_fn.h.
//
// The free table free_cells[F] (the row-major indices of the cells whose byte is 0, ascending) is the
// order-preserving compaction of particles/ndt2d_compact.h over the flags "cell i is free":
//
//   count_kernel    free cells per tile
//   scan_kernel     exclusive scan of the tile counts in one block; the total F goes to the
//                   seeder's pinned word by a system-scope vector store
//   scatter_kernel  a free cell to its rank
//
// The host reads F between the scan and the scatter, so the table is allocated at its size.
//
//   sample_kernel   one particle per thread, grid-stride from 4,096 blocks: two Philox blocks, one
//                   4-byte gather from the table, three 8-byte stores
//   inject_kernel   the same, stored only where the inject draw is below the probability; replaced
//                   particles are counted per block by ballots
//   fold_kernel     the block counts added by one block: a strided share per thread, fixed trees
//
// The seeder is an object of its own on the public device-layer calls
// (particles/ndt2d_device_object.h): the device context has no field for it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <string>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "particles/ndt2d_compact.h"
#include "particles/ndt2d_device_object.h"
#include "seed/ndt2d_seed_fn.h"

using namespace ndt2d::object;

namespace
{

namespace fn = ndt2d::seed;
namespace compact = ndt2d::particles;

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;

struct Region
{
  uint32_t x0, y0, w, h;
};

// the free flag of item i of the region (i < n: one item per thread of the grid)
__device__ __forceinline__ bool item_free(const signed char * __restrict__ map, uint32_t width,
                                          Region r, uint32_t n, uint32_t i, uint32_t * cell)
{
  if (i >= n) return false;
  *cell = fn::region_cell(i, r.x0, r.y0, r.w, width);
  return fn::is_free(map[*cell]);
}

__global__ void __launch_bounds__(kBlock) count_kernel(const signed char * __restrict__ map,
                                                       uint32_t width, Region r, uint32_t n,
                                                       uint32_t * __restrict__ sums)
{
  uint32_t cell = 0;
  compact::tile_count(item_free(map, width, r, n, blockIdx.x * kBlock + threadIdx.x, &cell), sums);
}

// sums[b] -> free cells in the tiles before b; the total to host_total (pinned)
__global__ void __launch_bounds__(kBlock) scan_kernel(uint32_t * sums, uint32_t n_tiles,
                                                      unsigned long long * host_total)
{
  const uint32_t total = compact::scan_tile_sums(sums, n_tiles);
  if (threadIdx.x == kBlock - 1)
  {
    // the pinned word, written through at system scope (a vector store)
    __hip_atomic_store(host_total, static_cast<unsigned long long>(total), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ void __launch_bounds__(kBlock) scatter_kernel(const signed char * __restrict__ map,
                                                         uint32_t width, Region r, uint32_t n,
                                                         const uint32_t * __restrict__ sums,
                                                         uint32_t n_free,
                                                         uint32_t * __restrict__ free_cells)
{
  uint32_t cell = 0;
  const bool flag = item_free(map, width, r, n, blockIdx.x * kBlock + threadIdx.x, &cell);
  const uint32_t rank = compact::tile_rank(flag, sums);
  if (!flag) return;
  // (the map the count saw is the map read here: rank < n_free; the test keeps a map that changed
  // in between from writing past the table)
  if (rank < n_free) free_cells[rank] = cell;
}

__global__ void __launch_bounds__(kBlock) sample_kernel(double * __restrict__ poses, uint64_t n,
                                                        uint64_t seed, uint64_t step,
                                                        uint64_t first_index,
                                                        const uint32_t * __restrict__ free_cells,
                                                        uint64_t n_free, fn::Geometry g)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n;
       i += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const fn::Sample s = fn::sample(seed, step, first_index + i, free_cells, n_free, g);
    poses[3 * i] = s.x;
    poses[3 * i + 1] = s.y;
    poses[3 * i + 2] = s.theta;
  }
}

// block_counts (or NULL: nobody asked for the count) receives this block's replaced particles
__global__ void __launch_bounds__(kBlock) inject_kernel(double * __restrict__ poses, uint64_t n,
                                                        double probability, uint64_t seed,
                                                        uint64_t step, uint64_t first_index,
                                                        const uint32_t * __restrict__ free_cells,
                                                        uint64_t n_free, fn::Geometry g,
                                                        unsigned long long * __restrict__ block_counts)
{
  __shared__ unsigned long long sh[kWaves];
  unsigned long long replaced = 0;   // of this wave (the same value in every lane)
  // the bound is uniform in a block, so every lane of a wave reaches the ballot
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock; base < n;
       base += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    const uint64_t i = base + threadIdx.x;
    bool take = false;
    if (i < n)
    {
      const fn::Sample s = fn::sample(seed, step, first_index + i, free_cells, n_free, g);
      take = s.inject < probability;
      if (take)
      {
        poses[3 * i] = s.x;
        poses[3 * i + 1] = s.y;
        poses[3 * i + 2] = s.theta;
      }
    }
    replaced += static_cast<unsigned long long>(__popcll(__ballot(take)));
  }
  if (block_counts == nullptr) return;
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = replaced;
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// the block counts into *out: a strided share per thread, then the waves' and the block's fixed trees
// (integer sums: any order gives the same count)
__global__ void __launch_bounds__(kBlock) fold_kernel(const unsigned long long * __restrict__ block_counts,
                                                      uint32_t n_blocks, unsigned long long * out)
{
  __shared__ unsigned long long sh[kWaves];
  unsigned long long total = 0;
  for (uint32_t b = threadIdx.x; b < n_blocks; b += kBlock) total += block_counts[b];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0) *out = sh[0] + sh[1] + sh[2] + sh[3];
}

}  // namespace

struct ndt2d_seeder : DeviceObject
{
  // the table and what it was made from
  bool have_table = false;
  uint64_t n_free = 0;
  fn::Geometry geo{0.0, 0.0, 0.0, 0};
  uint32_t * d_free = nullptr;     // [free_cap]
  size_t free_cap = 0;
  uint32_t * d_sums = nullptr;     // [sums_cap] tile counts, then tile offsets
  size_t sums_cap = 0;
  signed char * d_stage = nullptr; // [stage_cap] a host map's copy
  size_t stage_cap = 0;
  unsigned long long * d_blocks = nullptr;       // [kMaxBlocks] inject's block counts
  Pinned<unsigned long long> total;              // F, as the scan wrote it

  StreamUse use;

  bool timing = false;
  bool table_timed = false, sample_timed = false;
  hipEvent_t t0 = nullptr, t1 = nullptr, s0 = nullptr, s1 = nullptr;
};

namespace
{

void release(ndt2d_seeder * s)
{
  for (hipEvent_t e : {s->t0, s->t1, s->s0, s->s1})
  {
    if (e != nullptr) (void)hipEventDestroy(e);
  }
  if (s->d_free != nullptr) (void)ndt2d_device_free(s->h, s->d_free);
  if (s->d_sums != nullptr) (void)ndt2d_device_free(s->h, s->d_sums);
  if (s->d_stage != nullptr) (void)ndt2d_device_free(s->h, s->d_stage);
  if (s->d_blocks != nullptr) (void)ndt2d_device_free(s->h, s->d_blocks);
  pinned_free(s, &s->total);
  delete s;
}

constexpr const char * kNoRoom = "ndt2d_seed_set_map: device allocation failed";

// what both forms of set_map refuse, before anything runs
const char * refusal(const signed char * map, uint32_t width, uint32_t height, double origin_x,
                     double origin_y, double resolution, const uint32_t * region4)
{
  if (map == nullptr) return "ndt2d_seed_set_map: null map";
  const uint64_t cells = static_cast<uint64_t>(width) * height;
  if (cells == 0 || cells >= (1ull << 31)) return "ndt2d_seed_set_map: width * height is zero or 2^31 and above";
  if (!std::isfinite(resolution) || !(resolution > 0.0)) return "ndt2d_seed_set_map: the resolution is not finite and positive";
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) return "ndt2d_seed_set_map: the origin is not finite";
  if (region4 != nullptr)
  {
    if (static_cast<uint64_t>(region4[0]) + region4[2] > width ||
        static_cast<uint64_t>(region4[1]) + region4[3] > height)
    {
      return "ndt2d_seed_set_map: the region leaves the map";
    }
  }
  return nullptr;
}

// the three launches over a DEVICE map; `stream` is idle of this seeder's earlier work
int build_table(ndt2d_seeder * s, const signed char * d_map, uint32_t width, uint32_t height,
                double origin_x, double origin_y, double resolution, const uint32_t * region4,
                hipStream_t stream)
{
  const Region r = region4 != nullptr ? Region{region4[0], region4[1], region4[2], region4[3]}
                                      : Region{0, 0, width, height};
  const uint32_t n = r.w * r.h;   // < 2^31
  const uint32_t n_tiles = (n + kBlock - 1) / kBlock;
  s->have_table = false;
  s->table_timed = false;
  uint64_t n_free = 0;
  if (n > 0)
  {
    int rc = reserve(s, &s->d_sums, &s->sums_cap, n_tiles, kNoRoom);
    if (rc != NDT2D_OK) return rc;
    if (s->timing) NDT2D_OBJ_HIP(s, hipEventRecord(s->t0, stream));
    hipLaunchKernelGGL(count_kernel, dim3(n_tiles), dim3(kBlock), 0, stream, d_map, width, r, n, s->d_sums);
    NDT2D_OBJ_HIP(s, hipGetLastError());
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kBlock), 0, stream, s->d_sums, n_tiles, s->total.dev);
    NDT2D_OBJ_HIP(s, hipGetLastError());
    NDT2D_OBJ_HIP(s, hipStreamSynchronize(stream));
    n_free = static_cast<uint64_t>(__atomic_load_n(s->total.host, __ATOMIC_ACQUIRE));
    if (n_free > n) return fail(s, NDT2D_ERR_INTERNAL, "ndt2d_seed_set_map: a count above the region's cells");
    if (n_free > 0)
    {
      rc = reserve(s, &s->d_free, &s->free_cap, static_cast<size_t>(n_free), kNoRoom);
      if (rc != NDT2D_OK) return rc;
      hipLaunchKernelGGL(scatter_kernel, dim3(n_tiles), dim3(kBlock), 0, stream, d_map, width, r, n,
                         s->d_sums, static_cast<uint32_t>(n_free), s->d_free);
      NDT2D_OBJ_HIP(s, hipGetLastError());
    }
    if (s->timing) NDT2D_OBJ_HIP(s, hipEventRecord(s->t1, stream));
    // the caller's map (a staged copy or a resident one) is free again when this returns
    NDT2D_OBJ_HIP(s, hipStreamSynchronize(stream));
    s->table_timed = s->timing;
  }
  s->n_free = n_free;
  s->geo = fn::Geometry{origin_x, origin_y, resolution, width};
  s->have_table = true;
  return NDT2D_OK;
}

// what both sample calls refuse
int sample_prelude(ndt2d_seeder * s, const double * d_poses, size_t n, const char * null_text,
                   const char * state_text, const char * empty_text)
{
  if (n > 0 && d_poses == nullptr) return fail(s, NDT2D_ERR_INVALID, null_text);
  if (!s->have_table) return fail(s, NDT2D_ERR_STATE, state_text);
  if (s->n_free == 0) return fail(s, NDT2D_ERR_STATE, empty_text);
  return NDT2D_OK;
}

}  // namespace

extern "C" {

int ndt2d_seed_create(ndt2d_handle h, ndt2d_seeder ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr) return NDT2D_ERR_INVALID;
  ndt2d_seeder * s = new ndt2d_seeder();
  s->h = h;
  s->device = ndt2d_device_id(h);
  void * p = nullptr;
  int rc = ndt2d_device_alloc(h, kMaxBlocks * sizeof(unsigned long long), &p);
  s->d_blocks = static_cast<unsigned long long *>(p);
  if (rc == NDT2D_OK) rc = pinned_alloc(s, &s->total);
  if (rc != NDT2D_OK)
  {
    release(s);
    return rc;
  }
  *s->total.host = 0;
  hipError_t e = hipEventCreate(&s->t0);
  if (e == hipSuccess) e = hipEventCreate(&s->t1);
  if (e == hipSuccess) e = hipEventCreate(&s->s0);
  if (e == hipSuccess) e = hipEventCreate(&s->s1);
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    release(s);
    return NDT2D_ERR_HIP;
  }
  *out = s;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_seed_destroy(ndt2d_seeder * s)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(s->device);
  if (s->use.used) (void)hipStreamSynchronize(s->use.last_stream);
  release(s);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_seed_last_error(ndt2d_seeder * s) { return s != nullptr ? s->err.c_str() : ""; }

int ndt2d_seed_set_timing(ndt2d_seeder * s, int enabled)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  s->timing = enabled != 0;
  if (!s->timing) s->table_timed = s->sample_timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_seed_last_ms(ndt2d_seeder * s, float * table_ms, float * sample_ms)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (table_ms == nullptr || sample_ms == nullptr) return fail(s, NDT2D_ERR_INVALID, "ndt2d_seed_last_ms: null argument");
  if (!s->table_timed && !s->sample_timed) return fail(s, NDT2D_ERR_STATE, "ndt2d_seed_last_ms: no timed launch");
  *table_ms = 0.0f;
  *sample_ms = 0.0f;
  NDT2D_OBJ_HIP(s, hipSetDevice(s->device));
  if (s->table_timed) NDT2D_OBJ_HIP(s, hipEventElapsedTime(table_ms, s->t0, s->t1));
  if (s->sample_timed)
  {
    NDT2D_OBJ_HIP(s, hipEventSynchronize(s->s1));
    NDT2D_OBJ_HIP(s, hipEventElapsedTime(sample_ms, s->s0, s->s1));
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_seed_set_map(ndt2d_seeder * s, const signed char * map, uint32_t width, uint32_t height,
                       double origin_x, double origin_y, double resolution, const uint32_t * region4)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const char * why = refusal(map, width, height, origin_x, origin_y, resolution, region4);
  if (why != nullptr) return fail(s, NDT2D_ERR_INVALID, why);
  hipStream_t stream;
  int rc = current_stream(s, &s->use, &stream);
  if (rc != NDT2D_OK) return rc;
  NDT2D_OBJ_HIP(s, hipStreamSynchronize(stream));   // no sample in flight reads the table
  const size_t cells = static_cast<size_t>(width) * height;
  s->have_table = false;
  if ((rc = reserve(s, &s->d_stage, &s->stage_cap, cells, kNoRoom)) != NDT2D_OK) return rc;
  NDT2D_OBJ_HIP(s, hipMemcpyAsync(s->d_stage, map, cells, hipMemcpyHostToDevice, stream));
  return build_table(s, s->d_stage, width, height, origin_x, origin_y, resolution, region4, stream);
  NDT2D_C_CATCH(s)
}

int ndt2d_seed_set_map_device(ndt2d_seeder * s, const signed char * d_map, uint32_t width,
                              uint32_t height, double origin_x, double origin_y, double resolution,
                              const uint32_t * region4)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const char * why = refusal(d_map, width, height, origin_x, origin_y, resolution, region4);
  if (why != nullptr) return fail(s, NDT2D_ERR_INVALID, why);
  hipStream_t stream;
  const int rc = current_stream(s, &s->use, &stream);
  if (rc != NDT2D_OK) return rc;
  NDT2D_OBJ_HIP(s, hipStreamSynchronize(stream));
  return build_table(s, d_map, width, height, origin_x, origin_y, resolution, region4, stream);
  NDT2D_C_CATCH(s)
}

int ndt2d_seed_free_count(ndt2d_seeder * s, size_t * n_out)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_out == nullptr) return fail(s, NDT2D_ERR_INVALID, "ndt2d_seed_free_count: null argument");
  if (!s->have_table) return fail(s, NDT2D_ERR_STATE, "ndt2d_seed_free_count: no map (none set, or the last one failed)");
  *n_out = static_cast<size_t>(s->n_free);
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_seed_read_table(ndt2d_seeder * s, uint32_t * out, size_t capacity, size_t * n_out)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (n_out == nullptr) return fail(s, NDT2D_ERR_INVALID, "ndt2d_seed_read_table: null argument");
  *n_out = 0;
  if (!s->have_table) return fail(s, NDT2D_ERR_STATE, "ndt2d_seed_read_table: no map (none set, or the last one failed)");
  const size_t count = static_cast<size_t>(s->n_free);
  *n_out = count;
  if (count == 0) return NDT2D_OK;
  if (out == nullptr || capacity < count) return fail(s, NDT2D_ERR_INVALID, "ndt2d_seed_read_table: null output or a capacity below the count");
  return ndt2d_copy_to_host(s->h, out, s->d_free, count * sizeof(uint32_t));
  NDT2D_C_CATCH(s)
}

int ndt2d_seed_launch(ndt2d_seeder * s, double * d_poses_xyt, size_t n, uint64_t seed, uint64_t step,
                      uint64_t first_index)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  const int refused = sample_prelude(s, d_poses_xyt, n, "ndt2d_seed_launch: null poses",
                                     "ndt2d_seed_launch: no map (none set, or the last one failed)",
                                     "ndt2d_seed_launch: no free cell");
  if (refused != NDT2D_OK) return refused;
  if (n == 0) return NDT2D_OK;
  hipStream_t stream;
  const int rc = current_stream(s, &s->use, &stream);
  if (rc != NDT2D_OK) return rc;
  if (s->timing) NDT2D_OBJ_HIP(s, hipEventRecord(s->s0, stream));
  hipLaunchKernelGGL(sample_kernel, dim3(stride_blocks(n, kBlock)), dim3(kBlock), 0, stream, d_poses_xyt,
                     static_cast<uint64_t>(n), seed, step, first_index, s->d_free, s->n_free, s->geo);
  NDT2D_OBJ_HIP(s, hipGetLastError());
  if (s->timing)
  {
    NDT2D_OBJ_HIP(s, hipEventRecord(s->s1, stream));
    s->sample_timed = true;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

int ndt2d_seed_inject_launch(ndt2d_seeder * s, double * d_poses_xyt, size_t n, double probability,
                             uint64_t seed, uint64_t step, uint64_t first_index, uint64_t * d_count)
{
  NDT2D_C_TRY
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (!(probability >= 0.0 && probability <= 1.0))
  {
    return fail(s, NDT2D_ERR_INVALID, "ndt2d_seed_inject_launch: the probability is not in [0, 1]");
  }
  const int refused = sample_prelude(s, d_poses_xyt, n, "ndt2d_seed_inject_launch: null poses",
                                     "ndt2d_seed_inject_launch: no map (none set, or the last one failed)",
                                     "ndt2d_seed_inject_launch: no free cell");
  if (refused != NDT2D_OK) return refused;
  if (n == 0 && d_count == nullptr) return NDT2D_OK;
  hipStream_t stream;
  const int rc = current_stream(s, &s->use, &stream);
  if (rc != NDT2D_OK) return rc;
  if (n == 0 || probability == 0.0)
  {
    // no draw lies below 0: nothing is written
    if (d_count != nullptr) NDT2D_OBJ_HIP(s, hipMemsetAsync(d_count, 0, sizeof(uint64_t), stream));
    return NDT2D_OK;
  }
  const uint32_t blocks = stride_blocks(n, kBlock);
  if (s->timing) NDT2D_OBJ_HIP(s, hipEventRecord(s->s0, stream));
  hipLaunchKernelGGL(inject_kernel, dim3(blocks), dim3(kBlock), 0, stream, d_poses_xyt,
                     static_cast<uint64_t>(n), probability, seed, step, first_index, s->d_free,
                     s->n_free, s->geo, d_count != nullptr ? s->d_blocks : nullptr);
  NDT2D_OBJ_HIP(s, hipGetLastError());
  if (d_count != nullptr)
  {
    hipLaunchKernelGGL(fold_kernel, dim3(1), dim3(kBlock), 0, stream, s->d_blocks, blocks,
                       reinterpret_cast<unsigned long long *>(d_count));
    NDT2D_OBJ_HIP(s, hipGetLastError());
  }
  if (s->timing)
  {
    NDT2D_OBJ_HIP(s, hipEventRecord(s->s1, stream));
    s->sample_timed = true;
  }
  return NDT2D_OK;
  NDT2D_C_CATCH(s)
}

}  // extern "C"
