// ParticleFilter::resample on the device (reference src/particle_filter.cpp:91-137): the
// KLD draw-and-stop loop of ndt2d_kld_resample (ndt2d_host.cpp, the host form and the parity
// reference) restated as kernels, so that the particle set stays in HBM across a filter step.
//
// The loop is not inherently sequential: draw i uses uniforms[i] whatever happened before it,
// the KD-tree's leaf count after draw i is the number of distinct keys among draws 0..i, Mx is a
// pure function of that count, and the loop keeps the shortest prefix that passes the stop test.
// A launch is therefore
//
//   cdf_kernel      cdf[i] = w[0] + ... + w[i], ONE rounding per add in index order (the draws
//                   compare against these bits, so no reassociated scan): one wave, lane 0 walks
//                   the chain through LDS while all 64 lanes move the tiles in and out
//   draw_kernel     one draw per thread: libstdc++'s upper_bound bisection, the pinned key
//   insert_kernel   the key table of particles/ndt2d_key_table.h over the draws' 96-bit keys; a slot
//                   holds the SMALLEST draw index that has its key (claimed by CAS, lowered by
//                   atomicMin), so "draw i met a new leaf" == (slot owner == i), whatever the schedule
//   count_kernel, scan_sums_kernel, stop_kernel
//                   inclusive scan of the new-leaf flags (particles/ndt2d_compact.h), Mx, stop test,
//                   min-reduction
//   gather_kernel   out[j] = in[p_j] for j < count (count read from device memory), and the
//                   count to the resampler's pinned word with a system-scope vector store
//
// The resampler is an object of its own on the public device-layer calls
// (particles/ndt2d_device_object.h): the device context has no field for it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "particles/ndt2d_compact.h"
#include "particles/ndt2d_device_object.h"
#include "particles/ndt2d_key_table.h"
#include "particles/ndt2d_philox.h"

using namespace ndt2d::object;

namespace
{

namespace pt = ndt2d::particles;
using pt::kEmpty;

constexpr int kWave = 64;
constexpr int kTile = 1024;          // doubles per LDS tile of the cdf chain
constexpr int kTileRegs = kTile / kWave;

// the uniform of draw `index`: words 0 and 1 of its Philox block (key = seed, counter = {index, step})
__device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t index, uint64_t step)
{
  uint32_t w[4];
  pt::philox4x32_10(seed, index, step, w);
  return pt::uniform53(w[0], w[1]);
}

__global__ void __launch_bounds__(256) uniforms_kernel(double * out, uint64_t n, uint64_t seed,
                                                       uint64_t first_index, uint64_t step)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
       i += static_cast<uint64_t>(gridDim.x) * 256)
  {
    out[i] = philox_uniform(seed, first_index + i, step);
  }
}

// ---- 1. the cumulative weights ----
// One wave.  Tile t + 1 is on its way from HBM into registers while lane 0 runs tile t's adds in
// LDS (16 B reads one batch ahead of the dependent add chain), then all lanes write tile t out.
__global__ void __launch_bounds__(kWave) cdf_kernel(const double * __restrict__ weights, uint64_t n,
                                                    double * __restrict__ cdf)
{
  __shared__ double2 tile[2][kTile / 2];
  const int lane = threadIdx.x;
  const uint64_t n_tiles = (n + kTile - 1) / kTile;
  double reg[kTileRegs];
  double total = 0.0;

#pragma unroll
  for (int k = 0; k < kTileRegs; ++k)
  {
    const uint64_t idx = static_cast<uint64_t>(k * kWave + lane);
    reg[k] = idx < n ? weights[idx] : 0.0;
  }
  {
    double * t0 = reinterpret_cast<double *>(tile[0]);
#pragma unroll
    for (int k = 0; k < kTileRegs; ++k) t0[k * kWave + lane] = reg[k];
  }
  __syncthreads();

  for (uint64_t t = 0; t < n_tiles; ++t)
  {
    const int buf = static_cast<int>(t & 1);
    const uint64_t base = t * kTile;
    const bool more = t + 1 < n_tiles;
    if (more)
    {
#pragma unroll
      for (int k = 0; k < kTileRegs; ++k)
      {
        const uint64_t idx = base + kTile + static_cast<uint64_t>(k * kWave + lane);
        reg[k] = idx < n ? weights[idx] : 0.0;
      }
    }
    if (lane == 0)
    {
      const int count = static_cast<int>(n - base < static_cast<uint64_t>(kTile) ? n - base : kTile);
      const int n_batches = count >> 3;
      double2 * t2 = tile[buf];
      double2 c0 = make_double2(0.0, 0.0), c1 = c0, c2 = c0, c3 = c0;
      if (n_batches > 0)
      {
        c0 = t2[0];
        c1 = t2[1];
        c2 = t2[2];
        c3 = t2[3];
      }
      for (int b = 0; b < n_batches; ++b)
      {
        const int ahead = 4 * (b + 1 < n_batches ? b + 1 : b);
        const double2 d0 = t2[ahead], d1 = t2[ahead + 1], d2 = t2[ahead + 2], d3 = t2[ahead + 3];
        total += c0.x; c0.x = total;
        total += c0.y; c0.y = total;
        total += c1.x; c1.x = total;
        total += c1.y; c1.y = total;
        total += c2.x; c2.x = total;
        total += c2.y; c2.y = total;
        total += c3.x; c3.x = total;
        total += c3.y; c3.y = total;
        t2[4 * b] = c0;
        t2[4 * b + 1] = c1;
        t2[4 * b + 2] = c2;
        t2[4 * b + 3] = c3;
        c0 = d0;
        c1 = d1;
        c2 = d2;
        c3 = d3;
      }
      double * t1 = reinterpret_cast<double *>(t2);
      for (int j = n_batches << 3; j < count; ++j)
      {
        total += t1[j];
        t1[j] = total;
      }
    }
    __syncthreads();
    {
      const double * t1 = reinterpret_cast<const double *>(tile[buf]);
#pragma unroll
      for (int k = 0; k < kTileRegs; ++k)
      {
        const uint64_t idx = base + static_cast<uint64_t>(k * kWave + lane);
        if (idx < n) cdf[idx] = t1[k * kWave + lane];
      }
    }
    if (more)
    {
      double * tn = reinterpret_cast<double *>(tile[buf ^ 1]);
#pragma unroll
      for (int k = 0; k < kTileRegs; ++k) tn[k * kWave + lane] = reg[k];
    }
    __syncthreads();
  }
}

// ---- 2. the draws ----
// static_cast<int>(value / leaf) of the reference's KDTree::insert with the host form's pinning
__device__ __forceinline__ int32_t leaf_key(double value, double leaf)
{
  const double q = value / leaf;
  return q >= 2147483647.0 ? 2147483647
         : (q <= -2147483648.0 ? (-2147483647 - 1) : (q == q ? static_cast<int32_t>(q) : 0));
}

struct Leaf3
{
  double v[3];
};

__global__ void __launch_bounds__(256) draw_kernel(const double * __restrict__ particles,
                                                   const double * __restrict__ cdf, uint64_t n,
                                                   const double * __restrict__ uniforms,
                                                   uint64_t seed, uint64_t step, uint64_t max_particles,
                                                   Leaf3 leaf, uint32_t * __restrict__ draws,
                                                   int32_t * __restrict__ keys)
{
  const double total = cdf[n - 1];
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < max_particles;
       i += static_cast<uint64_t>(gridDim.x) * 256)
  {
    const double u = uniforms != nullptr ? uniforms[i] : philox_uniform(seed, i, step);
    const double val = u * total;
    // std::upper_bound as libstdc++ bisects it (with a NaN or negative weight the array is not
    // sorted, and only the same bisection gives the same answer)
    uint64_t first = 0, len = n;
    while (len > 0)
    {
      const uint64_t half = len >> 1;
      if (val < cdf[first + half])
      {
        len = half;
      }
      else
      {
        first += half + 1;
        len -= half + 1;
      }
    }
    const uint64_t p = first >= n ? n - 1 : first;
    draws[i] = static_cast<uint32_t>(p);
    keys[3 * i] = leaf_key(particles[3 * p], leaf.v[0]);
    keys[3 * i + 1] = leaf_key(particles[3 * p + 1], leaf.v[1]);
    keys[3 * i + 2] = leaf_key(particles[3 * p + 2], leaf.v[2]);
  }
}

// ---- 3. the leaf count ----
// The table (a power of two, at least 2 * max_particles) and the probe are
// particles/ndt2d_key_table.h; the keys were written by draw_kernel.
__global__ void __launch_bounds__(256) insert_kernel(const int32_t * __restrict__ keys,
                                                     uint64_t max_particles, uint32_t * table,
                                                     uint32_t mask, uint32_t * __restrict__ slots,
                                                     uint32_t * ctrl)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i < max_particles;
       i += static_cast<uint64_t>(gridDim.x) * 256)
  {
    const uint32_t me = static_cast<uint32_t>(i);
    uint32_t owner;
    const uint32_t found = pt::probe_claim(keys, table, mask, me, pt::load_key(keys, i), &owner);
    if (found == kEmpty)
    {
      atomicOr(ctrl + 2, 1u);   // (a table at most half full cannot run out)
    }
    else if (me < owner)
    {
      atomicMin(table + found, me);
    }
    slots[i] = found;
  }
}

__device__ __forceinline__ bool is_new_leaf(const uint32_t * table, const uint32_t * slots, uint64_t i)
{
  const uint32_t s = slots[i];
  return s != kEmpty && table[s] == static_cast<uint32_t>(i);
}

// new leaves per block of 256 draws
__global__ void __launch_bounds__(256) count_kernel(const uint32_t * __restrict__ table,
                                                    const uint32_t * __restrict__ slots,
                                                    uint64_t max_particles, uint32_t * __restrict__ sums)
{
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  pt::tile_count(i < max_particles && is_new_leaf(table, slots, i), sums);
}

// sums[b] -> new leaves in the blocks before b (one block)
__global__ void __launch_bounds__(256) scan_sums_kernel(uint32_t * sums, uint32_t n_blocks)
{
  (void)pt::scan_tile_sums(sums, n_blocks);
}

// Mx after each draw and the stop test (particle_filter.cpp:107,117-132); ctrl[0] = the smallest
// draw index that stops the loop
__global__ void __launch_bounds__(256) stop_kernel(const uint32_t * __restrict__ table,
                                                   const uint32_t * __restrict__ slots,
                                                   const uint32_t * __restrict__ sums,
                                                   uint64_t min_particles, uint64_t max_particles,
                                                   double kld_err, double kld_z, uint32_t * ctrl)
{
  __shared__ uint32_t block_min;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (threadIdx.x == 0) block_min = kEmpty;
  // the leaves after draw i (the rank's barrier orders block_min's store as well)
  const uint64_t k = pt::tile_rank_inclusive(i < max_particles && is_new_leaf(table, slots, i), sums);
  if (i < max_particles)
  {
    uint64_t mx_pinned = max_particles;
    if (k > 1)
    {
      const double a = static_cast<double>(k - 1) / (2.0 * kld_err);
      const double b = 2.0 / (9.0 * static_cast<double>(k - 1));
      const double c = 1.0 - b + sqrt(b) * kld_z;
      const double mx = a * c * c * c;
      mx_pinned = mx >= 1.8446744073709552e19 ? ~static_cast<uint64_t>(0)
                                              : (mx > 0.0 ? static_cast<uint64_t>(mx) : 0);
    }
    const uint64_t size = i + 1;
    const uint64_t want = min_particles > mx_pinned ? min_particles : mx_pinned;
    if (size >= want || size >= max_particles) atomicMin(&block_min, static_cast<uint32_t>(i));
  }
  __syncthreads();
  if (threadIdx.x == 0 && block_min != kEmpty) atomicMin(ctrl, block_min);
}

// ---- 4. the particles kept ----
__global__ void __launch_bounds__(256) gather_kernel(const double * __restrict__ particles,
                                                     const double * __restrict__ weights,
                                                     const uint32_t * __restrict__ draws,
                                                     const uint32_t * __restrict__ ctrl,
                                                     uint64_t max_particles,
                                                     double * __restrict__ particles_out,
                                                     double * __restrict__ weights_out,
                                                     uint32_t * __restrict__ indices_out,
                                                     unsigned long long * host_count)
{
  // (draw max_particles - 1 always passes the stop test, so the word is a draw index)
  const uint64_t stop = ctrl[0];
  const uint64_t count = stop < max_particles ? stop + 1 : max_particles;
  for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; j < count;
       j += static_cast<uint64_t>(gridDim.x) * 256)
  {
    const uint64_t p = draws[j];
    particles_out[3 * j] = particles[3 * p];
    particles_out[3 * j + 1] = particles[3 * p + 1];
    particles_out[3 * j + 2] = particles[3 * p + 2];
    weights_out[j] = weights[p];
    if (indices_out != nullptr) indices_out[j] = static_cast<uint32_t>(p);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    // the count for the host: the pinned word, written through at system scope as the context's
    // result block is (ndt2d_device_fn.h store_host)
    __hip_atomic_store(host_count, static_cast<unsigned long long>(count), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

struct ndt2d_resampler : DeviceObject
{
  size_t n_cap = 0;
  size_t max_cap = 0;

  void * workspace = nullptr;
  double * cdf = nullptr;        // [n_cap]
  uint32_t * draws = nullptr;    // [max_cap]
  int32_t * keys = nullptr;      // [max_cap][3]
  uint32_t * slots = nullptr;    // [max_cap]
  uint32_t * table = nullptr;    // [table_cap]
  uint32_t * sums = nullptr;     // [ceil(max_cap / 256)]
  uint32_t * ctrl = nullptr;     // {stop index, -, table-full flag, -}
  Pinned<unsigned long long> count;   // the particles kept, as the gather wrote it

  hipStream_t stream = nullptr;  // of the launch a fetch waits for
  bool launched = false;
  bool launched_empty = false;   // max_particles == 0: nothing ran, the count is 0

  bool timing = false;
  bool cdf_timed = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace
{

void release(ndt2d_resampler * r)
{
  if (r->ev0 != nullptr) (void)hipEventDestroy(r->ev0);
  if (r->ev1 != nullptr) (void)hipEventDestroy(r->ev1);
  if (r->workspace != nullptr) (void)ndt2d_device_free(r->h, r->workspace);
  pinned_free(r, &r->count);
  delete r;
}

}  // namespace

extern "C" {

int ndt2d_resampler_create(ndt2d_handle h, size_t n_capacity, size_t max_particles_capacity,
                           ndt2d_resampler ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  // draw indices and table slots are 32-bit words
  if (h == nullptr || n_capacity == 0 || n_capacity > 0xffffffffull ||
      max_particles_capacity > 0x40000000ull)
  {
    return NDT2D_ERR_INVALID;
  }
  ndt2d_resampler * r = new ndt2d_resampler();
  r->h = h;
  r->device = ndt2d_device_id(h);
  r->n_cap = n_capacity;
  r->max_cap = max_particles_capacity;
  const size_t m = max_particles_capacity > 0 ? max_particles_capacity : 1;
  const size_t b_cdf = align_up(n_capacity * sizeof(double));
  const size_t b_draws = align_up(m * sizeof(uint32_t));
  const size_t b_keys = align_up(3 * m * sizeof(int32_t));
  const size_t n_table = static_cast<size_t>(pt::table_size(m)), n_sums = (m + 255) / 256;
  const size_t b_table = align_up(n_table * sizeof(uint32_t));
  const size_t b_sums = align_up(n_sums * sizeof(uint32_t));
  const size_t b_ctrl = 256;
  int rc = ndt2d_device_alloc(h, b_cdf + 2 * b_draws + b_keys + b_table + b_sums + b_ctrl, &r->workspace);
  if (rc == NDT2D_OK) rc = pinned_alloc(r, &r->count);
  if (rc != NDT2D_OK)
  {
    release(r);
    return rc;
  }
  char * p = static_cast<char *>(r->workspace);
  r->cdf = carve<double>(&p, n_capacity);
  r->draws = carve<uint32_t>(&p, m);
  r->slots = carve<uint32_t>(&p, m);
  r->keys = carve<int32_t>(&p, 3 * m);
  r->table = carve<uint32_t>(&p, n_table);
  r->sums = carve<uint32_t>(&p, n_sums);
  r->ctrl = carve<uint32_t>(&p, 4);
  *r->count.host = 0;
  hipError_t e = hipEventCreate(&r->ev0);
  if (e == hipSuccess) e = hipEventCreate(&r->ev1);
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    release(r);
    return NDT2D_ERR_HIP;
  }
  *out = r;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_resampler_destroy(ndt2d_resampler * r)
{
  NDT2D_C_TRY
  if (r == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(r->device);
  if (r->launched && !r->launched_empty) (void)hipStreamSynchronize(r->stream);
  release(r);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_resampler_last_error(ndt2d_resampler * r) { return r != nullptr ? r->err.c_str() : ""; }

int ndt2d_resampler_set_timing(ndt2d_resampler * r, int enabled)
{
  NDT2D_C_TRY
  if (r == nullptr) return NDT2D_ERR_INVALID;
  r->timing = enabled != 0;
  if (!r->timing) r->cdf_timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

int ndt2d_resampler_cdf_ms(ndt2d_resampler * r, float * ms)
{
  NDT2D_C_TRY
  if (r == nullptr || ms == nullptr) return NDT2D_ERR_INVALID;
  if (!r->cdf_timed) return fail(r, NDT2D_ERR_STATE, "ndt2d_resampler_cdf_ms: no timed launch");
  NDT2D_OBJ_HIP(r, hipSetDevice(r->device));
  NDT2D_OBJ_HIP(r, hipEventSynchronize(r->ev1));
  NDT2D_OBJ_HIP(r, hipEventElapsedTime(ms, r->ev0, r->ev1));
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

int ndt2d_resample_uniforms_launch(ndt2d_resampler * r, uint64_t seed, uint64_t step,
                                   uint64_t first_index, size_t n, double * d_out)
{
  NDT2D_C_TRY
  if (r == nullptr) return NDT2D_ERR_INVALID;
  if (n == 0 || d_out == nullptr) return fail(r, NDT2D_ERR_INVALID, "ndt2d_resample_uniforms_launch: nothing to write");
  NDT2D_OBJ_HIP(r, hipSetDevice(r->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(r->h));
  hipLaunchKernelGGL(uniforms_kernel, dim3(stride_blocks(n, 256)), dim3(256), 0, stream, d_out,
                     static_cast<uint64_t>(n), seed, first_index, step);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

int ndt2d_resample_launch(ndt2d_resampler * r, const double * d_particles_xyt,
                          const double * d_weights, size_t n, size_t min_particles,
                          size_t max_particles, double kld_err, double kld_z,
                          const double * leaf_size3, const double * d_uniforms, uint64_t seed,
                          uint64_t step, double * d_particles_out, double * d_weights_out,
                          uint32_t * d_indices_out)
{
  NDT2D_C_TRY
  if (r == nullptr) return NDT2D_ERR_INVALID;
  if (max_particles == 0)
  {
    r->launched = true;
    r->launched_empty = true;
    return NDT2D_OK;
  }
  if (n == 0 || n > 0xffffffffull || d_particles_xyt == nullptr || d_weights == nullptr ||
      leaf_size3 == nullptr || d_particles_out == nullptr || d_weights_out == nullptr)
  {
    return fail(r, NDT2D_ERR_INVALID, "ndt2d_resample_launch: null pointer or bad particle count");
  }
  if (n > r->n_cap || max_particles > r->max_cap)
  {
    return fail(r, NDT2D_ERR_INVALID, "ndt2d_resample_launch: beyond the resampler's capacity");
  }
  if (d_particles_out == d_particles_xyt || d_weights_out == d_weights)
  {
    return fail(r, NDT2D_ERR_INVALID, "ndt2d_resample_launch: the gather cannot run in place");
  }
  NDT2D_OBJ_HIP(r, hipSetDevice(r->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(r->h));
  const uint64_t n64 = n, max64 = max_particles;
  const uint64_t tsize = pt::table_size(max64);
  const uint32_t item_blocks = static_cast<uint32_t>((max64 + 255) / 256);
  Leaf3 leaf;
  for (int d = 0; d < 3; ++d) leaf.v[d] = leaf_size3[d];

  NDT2D_OBJ_HIP(r, hipMemsetAsync(r->table, 0xff, tsize * sizeof(uint32_t), stream));
  NDT2D_OBJ_HIP(r, hipMemsetAsync(r->ctrl, 0xff, sizeof(uint32_t), stream));
  NDT2D_OBJ_HIP(r, hipMemsetAsync(r->ctrl + 1, 0, 3 * sizeof(uint32_t), stream));
  if (r->timing) NDT2D_OBJ_HIP(r, hipEventRecord(r->ev0, stream));
  hipLaunchKernelGGL(cdf_kernel, dim3(1), dim3(kWave), 0, stream, d_weights, n64, r->cdf);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  if (r->timing)
  {
    NDT2D_OBJ_HIP(r, hipEventRecord(r->ev1, stream));
    r->cdf_timed = true;
  }
  hipLaunchKernelGGL(draw_kernel, dim3(stride_blocks(max64, 256)), dim3(256), 0, stream, d_particles_xyt,
                     r->cdf, n64, d_uniforms, seed, step, max64, leaf, r->draws, r->keys);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(insert_kernel, dim3(stride_blocks(max64, 256)), dim3(256), 0, stream, r->keys, max64,
                     r->table, static_cast<uint32_t>(tsize - 1), r->slots, r->ctrl);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(count_kernel, dim3(item_blocks), dim3(256), 0, stream, r->table, r->slots, max64,
                     r->sums);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, r->sums, item_blocks);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(stop_kernel, dim3(item_blocks), dim3(256), 0, stream, r->table, r->slots, r->sums,
                     static_cast<uint64_t>(min_particles), max64, kld_err, kld_z, r->ctrl);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(gather_kernel, dim3(stride_blocks(max64, 256)), dim3(256), 0, stream, d_particles_xyt,
                     d_weights, r->draws, r->ctrl, max64, d_particles_out, d_weights_out, d_indices_out,
                     r->count.dev);
  NDT2D_OBJ_HIP(r, hipGetLastError());
  r->stream = stream;
  r->launched = true;
  r->launched_empty = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

int ndt2d_resample_fetch(ndt2d_resampler * r, size_t * n_out)
{
  NDT2D_C_TRY
  if (r == nullptr || n_out == nullptr) return NDT2D_ERR_INVALID;
  *n_out = 0;
  if (!r->launched) return fail(r, NDT2D_ERR_STATE, "ndt2d_resample_fetch: nothing launched");
  r->launched = false;
  if (r->launched_empty) return NDT2D_OK;
  NDT2D_OBJ_HIP(r, hipSetDevice(r->device));
  NDT2D_OBJ_HIP(r, hipStreamSynchronize(r->stream));
  *n_out = static_cast<size_t>(__atomic_load_n(r->count.host, __ATOMIC_ACQUIRE));
  return NDT2D_OK;
  NDT2D_C_CATCH(r)
}

int ndt2d_pf_resample(ndt2d_handle h, const double * particles_xyt, const double * weights, size_t n,
                      size_t min_particles, size_t max_particles, double kld_err, double kld_z,
                      const double * leaf_size3, const double * uniforms, size_t n_uniforms,
                      uint32_t * indices_out, size_t * n_out)
{
  NDT2D_C_TRY
  if (n_out == nullptr) return NDT2D_ERR_INVALID;
  *n_out = 0;
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (max_particles == 0) return NDT2D_OK;
  if (n == 0 || n > 0xffffffffull || particles_xyt == nullptr || weights == nullptr ||
      leaf_size3 == nullptr || uniforms == nullptr || indices_out == nullptr ||
      n_uniforms < max_particles)
  {
    return NDT2D_ERR_INVALID;
  }
  ndt2d_resampler * r = nullptr;
  int rc = ndt2d_resampler_create(h, n, max_particles, &r);
  if (rc != NDT2D_OK) return rc;
  const size_t b_particles = align_up(3 * n * sizeof(double)), b_weights = align_up(n * sizeof(double));
  const size_t b_uniforms = align_up(max_particles * sizeof(double));
  const size_t b_out_p = align_up(3 * max_particles * sizeof(double));
  const size_t b_idx = align_up(max_particles * sizeof(uint32_t));
  void * block = nullptr;
  rc = ndt2d_device_alloc(h, b_particles + b_weights + 2 * b_uniforms + b_out_p + b_idx, &block);
  if (rc == NDT2D_OK)
  {
    char * p = static_cast<char *>(block);
    double * d_particles = reinterpret_cast<double *>(p);
    double * d_weights = reinterpret_cast<double *>(p + b_particles);
    double * d_uniforms = reinterpret_cast<double *>(p + b_particles + b_weights);
    double * d_out_w = reinterpret_cast<double *>(p + b_particles + b_weights + b_uniforms);
    double * d_out_p = reinterpret_cast<double *>(p + b_particles + b_weights + 2 * b_uniforms);
    uint32_t * d_idx = reinterpret_cast<uint32_t *>(p + b_particles + b_weights + 2 * b_uniforms + b_out_p);
    size_t count = 0;
    rc = ndt2d_copy_to_device_async(h, d_particles, particles_xyt, 3 * n * sizeof(double));
    if (rc == NDT2D_OK) rc = ndt2d_copy_to_device_async(h, d_weights, weights, n * sizeof(double));
    if (rc == NDT2D_OK) rc = ndt2d_copy_to_device_async(h, d_uniforms, uniforms, max_particles * sizeof(double));
    if (rc == NDT2D_OK)
    {
      rc = ndt2d_resample_launch(r, d_particles, d_weights, n, min_particles, max_particles, kld_err,
                                 kld_z, leaf_size3, d_uniforms, 0, 0, d_out_p, d_out_w, d_idx);
    }
    if (rc == NDT2D_OK) rc = ndt2d_resample_fetch(r, &count);
    if (rc == NDT2D_OK && count > 0) rc = ndt2d_copy_to_host(h, indices_out, d_idx, count * sizeof(uint32_t));
    if (rc == NDT2D_OK) *n_out = count;
    (void)ndt2d_synchronize(h);   // the caller's arrays are free again whatever happened
  }
  (void)ndt2d_resampler_destroy(r);
  if (block != nullptr) (void)ndt2d_device_free(h, block);
  return rc;
  NDT2D_C_CATCH(nullptr)
}

}  // extern "C"
