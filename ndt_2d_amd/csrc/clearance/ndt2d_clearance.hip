// The clearance map (include/ndt2d_hip.h, "Clearance map"): for every cell of an int8 occupancy map
// the exact squared Euclidean distance, in cells, to the nearest obstacle cell, and a copy of the map
// in which the free cells nearer than a threshold are marked.  The arithmetic is
// clearance/ndt2d_clearance_fn.h; everything is integer, nothing is atomic, two calls give the same
// bits.
//
// The transform is separable.  g[y][x] (uint16) is the vertical distance to the nearest obstacle in
// column x, then d2[y][x] = min over x' of (x - x')^2 + g[y][x']^2.
//
//   strip_kernel    a thread per (strip of 64 rows, column), consecutive lanes consecutive columns:
//                   the strip's obstacle rows as the bits of a uint64, its first and last obstacle row
//   carry_kernel    a thread per column: the nearest obstacle row above and below every strip, carried
//                   across the strip summaries in place
//   column_kernel   a thread per (strip, column): g of its 64 rows from the bits and the two carried
//                   rows -- the map is read once and g is written once
//   row_kernel      a workgroup per row, the row's g in LDS (2 bytes a cell: 64 KB at the widest); a
//                   thread per cell scans outwards and stops at dx^2 >= best (or dx > R under a cap);
//                   a row without any obstacle column writes NDT2D_CLEARANCE_FAR without scanning
//   mask_kernel     grid-stride: byte 0 with d2 < min_d2 becomes 99, every other byte is copied
//
// The object keeps its own copy of the map (a host map is staged into it, a device map copied), so the
// source may change as soon as compute returns and the mask needs no second look at it.  An object of
// its own on the public device-layer calls (particles/ndt2d_device_object.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <string>

#include "clearance/ndt2d_clearance_fn.h"
#include "ndt2d_guard.h"
#include "ndt2d_hip.h"
#include "particles/ndt2d_device_object.h"

using namespace ndt2d::object;

namespace
{

namespace fn = ndt2d::clearance;

static_assert(fn::kFar == NDT2D_CLEARANCE_FAR, "the header's value");

constexpr int kBlock = 256;

// bits[s][x], first[s][x], last[s][x] of strip s = blockIdx.y
__global__ void __launch_bounds__(kBlock) strip_kernel(const signed char * __restrict__ map, uint32_t width,
                                                       uint32_t height, int unknown_is_obstacle,
                                                       unsigned long long * __restrict__ bits,
                                                       uint16_t * __restrict__ first,
                                                       uint16_t * __restrict__ last)
{
  const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= width) return;
  const uint32_t s = blockIdx.y;
  const uint32_t y0 = s * fn::kStrip;
  const uint32_t rows = height - y0 < fn::kStrip ? height - y0 : fn::kStrip;
  uint64_t m = 0;
  for (uint32_t r = 0; r < rows; ++r)
  {
    const signed char v = map[static_cast<size_t>(y0 + r) * width + x];
    m |= static_cast<uint64_t>(fn::is_obstacle(v, unknown_is_obstacle != 0)) << r;
  }
  const size_t at = static_cast<size_t>(s) * width + x;
  bits[at] = m;
  first[at] = m != 0 ? static_cast<uint16_t>(y0 + fn::low_bit(m)) : fn::kNone;
  last[at] = m != 0 ? static_cast<uint16_t>(y0 + fn::top_bit(m)) : fn::kNone;
}

// last[s][x] becomes the nearest obstacle row above strip s, first[s][x] the nearest below it
__global__ void __launch_bounds__(kBlock) carry_kernel(uint32_t width, uint32_t n_strips,
                                                       uint16_t * __restrict__ first,
                                                       uint16_t * __restrict__ last)
{
  const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= width) return;
  uint16_t carry = fn::kNone;
  for (uint32_t s = 0; s < n_strips; ++s)
  {
    const size_t at = static_cast<size_t>(s) * width + x;
    const uint16_t own = last[at];
    last[at] = carry;
    if (own != fn::kNone) carry = own;
  }
  carry = fn::kNone;
  for (uint32_t s = n_strips; s-- > 0;)
  {
    const size_t at = static_cast<size_t>(s) * width + x;
    const uint16_t own = first[at];
    first[at] = carry;
    if (own != fn::kNone) carry = own;
  }
}

__global__ void __launch_bounds__(kBlock) column_kernel(uint32_t width, uint32_t height,
                                                        const unsigned long long * __restrict__ bits,
                                                        const uint16_t * __restrict__ below,
                                                        const uint16_t * __restrict__ above,
                                                        uint16_t * __restrict__ g)
{
  const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= width) return;
  const uint32_t s = blockIdx.y;
  const uint32_t y0 = s * fn::kStrip;
  const uint32_t rows = height - y0 < fn::kStrip ? height - y0 : fn::kStrip;
  const size_t at = static_cast<size_t>(s) * width + x;
  const uint64_t m = bits[at];
  const uint16_t up = above[at], down = below[at];
  for (uint32_t r = 0; r < rows; ++r)
  {
    g[static_cast<size_t>(y0 + r) * width + x] = fn::column_distance(m, y0, r, up, down);
  }
}

// row = blockIdx.x; dynamic LDS: uint16 row[width]
__global__ void __launch_bounds__(kBlock) row_kernel(const uint16_t * __restrict__ g, uint32_t width,
                                                     uint32_t cap, uint32_t * __restrict__ d2)
{
  extern __shared__ uint16_t row[];
  const size_t base = static_cast<size_t>(blockIdx.x) * width;
  int any = 0;
  for (uint32_t x = threadIdx.x; x < width; x += kBlock)
  {
    const uint16_t v = g[base + x];
    row[x] = v;
    any |= v != fn::kNone;
  }
  // (also the barrier between the row's stores and its loads)
  const bool scan = __syncthreads_or(any) != 0;
  for (uint32_t x = threadIdx.x; x < width; x += kBlock)
  {
    d2[base + x] = scan ? fn::row_min(row, width, x, cap) : fn::kFar;
  }
}

__global__ void __launch_bounds__(kBlock) mask_kernel(const signed char * __restrict__ map,
                                                      const uint32_t * __restrict__ d2, uint64_t cells,
                                                      uint32_t min_d2, signed char * __restrict__ out)
{
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < cells;
       i += static_cast<uint64_t>(gridDim.x) * kBlock)
  {
    out[i] = fn::masked(map[i], d2[i], min_d2);
  }
}

}  // namespace

struct ndt2d_clearance : DeviceObject
{
  bool have_d2 = false, have_mask = false;
  uint32_t width = 0, height = 0;
  signed char * d_map = nullptr;    // [cells_cap] the object's copy of the map
  signed char * d_mask = nullptr;   // [mask_cap]
  uint16_t * d_g = nullptr;         // [cells_cap]
  uint32_t * d_d2 = nullptr;        // [cells_cap]
  size_t map_cap = 0, mask_cap = 0, g_cap = 0, d2_cap = 0;
  unsigned long long * d_bits = nullptr;   // [strips_cap] per (strip, column)
  uint16_t * d_first = nullptr, * d_last = nullptr;
  size_t bits_cap = 0, first_cap = 0, last_cap = 0;

  StreamUse use;

  bool timing = false;
  bool transform_timed = false, mask_timed = false;
  hipEvent_t t0 = nullptr, t1 = nullptr, m0 = nullptr, m1 = nullptr;
};

namespace
{

void release(ndt2d_clearance * c)
{
  for (hipEvent_t e : {c->t0, c->t1, c->m0, c->m1})
  {
    if (e != nullptr) (void)hipEventDestroy(e);
  }
  for (void * p : {static_cast<void *>(c->d_map), static_cast<void *>(c->d_mask), static_cast<void *>(c->d_g),
                   static_cast<void *>(c->d_d2), static_cast<void *>(c->d_bits), static_cast<void *>(c->d_first),
                   static_cast<void *>(c->d_last)})
  {
    if (p != nullptr) (void)ndt2d_device_free(c->h, p);
  }
  delete c;
}

constexpr const char * kNoRoom = "ndt2d_clearance_compute: device allocation failed";

// what both forms of compute refuse, before anything is allocated or launched
const char * refusal(const signed char * map, uint32_t width, uint32_t height, int64_t max_cells)
{
  if (map == nullptr) return "ndt2d_clearance_compute: null map";
  if (width == 0 || height == 0) return "ndt2d_clearance_compute: width or height is zero";
  if (width > fn::kMaxSide || height > fn::kMaxSide) return "ndt2d_clearance_compute: width or height above 32768";
  if (max_cells < 0) return "ndt2d_clearance_compute: max_cells is negative";
  return nullptr;
}

// the map into the object's copy, then the four launches; returns when complete
int transform(ndt2d_clearance * c, const signed char * map, hipMemcpyKind kind, uint32_t width, uint32_t height,
              int unknown_is_obstacle, int64_t max_cells)
{
  hipStream_t stream;
  int rc = current_stream(c, &c->use, &stream);
  if (rc != NDT2D_OK) return rc;
  NDT2D_OBJ_HIP(c, hipStreamSynchronize(stream));   // nothing in flight reads the blocks reserve may replace
  const size_t cells = static_cast<size_t>(width) * height;
  const uint32_t n_strips = (height + fn::kStrip - 1) / fn::kStrip;
  const size_t summaries = static_cast<size_t>(n_strips) * width;
  c->have_d2 = c->have_mask = false;
  c->transform_timed = c->mask_timed = false;
  if ((rc = reserve(c, &c->d_map, &c->map_cap, cells, kNoRoom)) != NDT2D_OK) return rc;
  if ((rc = reserve(c, &c->d_g, &c->g_cap, cells, kNoRoom)) != NDT2D_OK) return rc;
  if ((rc = reserve(c, &c->d_d2, &c->d2_cap, cells, kNoRoom)) != NDT2D_OK) return rc;
  if ((rc = reserve(c, &c->d_bits, &c->bits_cap, summaries, kNoRoom)) != NDT2D_OK) return rc;
  if ((rc = reserve(c, &c->d_first, &c->first_cap, summaries, kNoRoom)) != NDT2D_OK) return rc;
  if ((rc = reserve(c, &c->d_last, &c->last_cap, summaries, kNoRoom)) != NDT2D_OK) return rc;
  NDT2D_OBJ_HIP(c, hipMemcpyAsync(c->d_map, map, cells, kind, stream));
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->t0, stream));
  const dim3 columns((width + kBlock - 1) / kBlock, n_strips);   // n_strips <= 512
  hipLaunchKernelGGL(strip_kernel, columns, dim3(kBlock), 0, stream, c->d_map, width, height, unknown_is_obstacle,
                     c->d_bits, c->d_first, c->d_last);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(carry_kernel, dim3(columns.x), dim3(kBlock), 0, stream, width, n_strips, c->d_first, c->d_last);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(column_kernel, columns, dim3(kBlock), 0, stream, width, height, c->d_bits, c->d_first,
                     c->d_last, c->d_g);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  // (width <= 32768: at most 65,536 bytes of LDS)
  hipLaunchKernelGGL(row_kernel, dim3(height), dim3(kBlock), static_cast<size_t>(width) * sizeof(uint16_t), stream,
                     c->d_g, width, fn::effective_cap(max_cells), c->d_d2);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->t1, stream));
  NDT2D_OBJ_HIP(c, hipStreamSynchronize(stream));   // the caller's map is free again
  c->transform_timed = c->timing;
  c->width = width;
  c->height = height;
  c->have_d2 = true;
  return NDT2D_OK;
}

// a rectangle of a resident [height][width] array of T into HOST out[h][row_stride]
template <typename T>
int read_rect(ndt2d_clearance * c, const T * d_src, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, T * out,
              size_t row_stride, const char * leaves, const char * null_text)
{
  if (static_cast<uint64_t>(x0) + w > c->width || static_cast<uint64_t>(y0) + h > c->height)
  {
    return fail(c, NDT2D_ERR_INVALID, leaves);
  }
  if (w == 0 || h == 0) return NDT2D_OK;
  if (out == nullptr || row_stride < w) return fail(c, NDT2D_ERR_INVALID, null_text);
  hipStream_t stream;
  const int rc = current_stream(c, &c->use, &stream);
  if (rc != NDT2D_OK) return rc;
  const T * src = d_src + static_cast<size_t>(y0) * c->width + x0;
  NDT2D_OBJ_HIP(c, hipMemcpy2DAsync(out, row_stride * sizeof(T), src, static_cast<size_t>(c->width) * sizeof(T),
                                    static_cast<size_t>(w) * sizeof(T), h, hipMemcpyDeviceToHost, stream));
  NDT2D_OBJ_HIP(c, hipStreamSynchronize(stream));
  return NDT2D_OK;
}

}  // namespace

extern "C" {

int ndt2d_clearance_create(ndt2d_handle h, ndt2d_clearance ** out)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (h == nullptr) return NDT2D_ERR_INVALID;
  ndt2d_clearance * c = new ndt2d_clearance();
  c->h = h;
  c->device = ndt2d_device_id(h);
  hipError_t e = hipSetDevice(c->device);
  // the widest row is 64 KB of dynamic LDS (gfx950 has 160 KB a workgroup)
  if (e == hipSuccess)
  {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(fn::kMaxSide * sizeof(uint16_t)));
  }
  if (e == hipSuccess) e = hipEventCreate(&c->t0);
  if (e == hipSuccess) e = hipEventCreate(&c->t1);
  if (e == hipSuccess) e = hipEventCreate(&c->m0);
  if (e == hipSuccess) e = hipEventCreate(&c->m1);
  if (e != hipSuccess)
  {
    (void)hipGetLastError();
    release(c);
    return NDT2D_ERR_HIP;
  }
  *out = c;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_clearance_destroy(ndt2d_clearance * c)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (c->use.used) (void)hipStreamSynchronize(c->use.last_stream);
  release(c);
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

const char * ndt2d_clearance_last_error(ndt2d_clearance * c) { return c != nullptr ? c->err.c_str() : ""; }

int ndt2d_clearance_set_timing(ndt2d_clearance * c, int enabled)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  c->timing = enabled != 0;
  if (!c->timing) c->transform_timed = c->mask_timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_clearance_last_ms(ndt2d_clearance * c, float * transform_ms, float * mask_ms)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (transform_ms == nullptr || mask_ms == nullptr) return fail(c, NDT2D_ERR_INVALID, "ndt2d_clearance_last_ms: null argument");
  if (!c->transform_timed && !c->mask_timed) return fail(c, NDT2D_ERR_STATE, "ndt2d_clearance_last_ms: no timed launch");
  *transform_ms = 0.0f;
  *mask_ms = 0.0f;
  NDT2D_OBJ_HIP(c, hipSetDevice(c->device));
  if (c->transform_timed) NDT2D_OBJ_HIP(c, hipEventElapsedTime(transform_ms, c->t0, c->t1));
  if (c->mask_timed) NDT2D_OBJ_HIP(c, hipEventElapsedTime(mask_ms, c->m0, c->m1));
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_clearance_compute(ndt2d_clearance * c, const signed char * map, uint32_t width, uint32_t height,
                            int unknown_is_obstacle, int64_t max_cells)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  const char * why = refusal(map, width, height, max_cells);
  if (why != nullptr) return fail(c, NDT2D_ERR_INVALID, why);
  return transform(c, map, hipMemcpyHostToDevice, width, height, unknown_is_obstacle, max_cells);
  NDT2D_C_CATCH(c)
}

int ndt2d_clearance_compute_device(ndt2d_clearance * c, const signed char * d_map, uint32_t width, uint32_t height,
                                   int unknown_is_obstacle, int64_t max_cells)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  const char * why = refusal(d_map, width, height, max_cells);
  if (why != nullptr) return fail(c, NDT2D_ERR_INVALID, why);
  return transform(c, d_map, hipMemcpyDeviceToDevice, width, height, unknown_is_obstacle, max_cells);
  NDT2D_C_CATCH(c)
}

int ndt2d_clearance_min_d2(double clearance_m, double resolution, int64_t max_cells, uint32_t * min_d2)
{
  NDT2D_C_TRY
  if (min_d2 == nullptr) return NDT2D_ERR_INVALID;
  return fn::min_d2_of(clearance_m, resolution, max_cells, min_d2) ? NDT2D_OK : NDT2D_ERR_INVALID;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_clearance_read(ndt2d_clearance * c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t * out,
                         size_t out_row_stride)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (!c->have_d2) return fail(c, NDT2D_ERR_STATE, "ndt2d_clearance_read: no transform (none computed, or the last one failed)");
  return read_rect(c, c->d_d2, x0, y0, w, h, out, out_row_stride, "ndt2d_clearance_read: the rectangle leaves the map",
                   "ndt2d_clearance_read: null output or a row stride below w");
  NDT2D_C_CATCH(c)
}

int ndt2d_clearance_device(ndt2d_clearance * c, const uint32_t ** d_d2, uint32_t * width, uint32_t * height)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (d_d2 == nullptr || width == nullptr || height == nullptr) return fail(c, NDT2D_ERR_INVALID, "ndt2d_clearance_device: null argument");
  *d_d2 = nullptr;
  if (!c->have_d2) return fail(c, NDT2D_ERR_STATE, "ndt2d_clearance_device: no transform (none computed, or the last one failed)");
  *d_d2 = c->d_d2;
  *width = c->width;
  *height = c->height;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_clearance_mask(ndt2d_clearance * c, uint32_t min_d2, const signed char ** d_masked_map)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (d_masked_map == nullptr) return fail(c, NDT2D_ERR_INVALID, "ndt2d_clearance_mask: null argument");
  *d_masked_map = nullptr;
  if (!c->have_d2) return fail(c, NDT2D_ERR_STATE, "ndt2d_clearance_mask: no transform (none computed, or the last one failed)");
  hipStream_t stream;
  int rc = current_stream(c, &c->use, &stream);
  if (rc != NDT2D_OK) return rc;
  NDT2D_OBJ_HIP(c, hipStreamSynchronize(stream));
  const size_t cells = static_cast<size_t>(c->width) * c->height;
  c->have_mask = false;
  c->mask_timed = false;
  if ((rc = reserve(c, &c->d_mask, &c->mask_cap, cells, "ndt2d_clearance_mask: device allocation failed")) != NDT2D_OK) return rc;
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->m0, stream));
  hipLaunchKernelGGL(mask_kernel, dim3(stride_blocks(cells, kBlock)), dim3(kBlock), 0, stream, c->d_map, c->d_d2,
                     static_cast<uint64_t>(cells), min_d2, c->d_mask);
  NDT2D_OBJ_HIP(c, hipGetLastError());
  if (c->timing) NDT2D_OBJ_HIP(c, hipEventRecord(c->m1, stream));
  NDT2D_OBJ_HIP(c, hipStreamSynchronize(stream));
  c->mask_timed = c->timing;
  c->have_mask = true;
  *d_masked_map = c->d_mask;
  return NDT2D_OK;
  NDT2D_C_CATCH(c)
}

int ndt2d_clearance_read_mask(ndt2d_clearance * c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                              signed char * out, size_t out_row_stride)
{
  NDT2D_C_TRY
  if (c == nullptr) return NDT2D_ERR_INVALID;
  if (!c->have_mask) return fail(c, NDT2D_ERR_STATE, "ndt2d_clearance_read_mask: no mask (none made since the last transform)");
  return read_rect(c, c->d_mask, x0, y0, w, h, out, out_row_stride, "ndt2d_clearance_read_mask: the rectangle leaves the map",
                   "ndt2d_clearance_read_mask: null output or a row stride below w");
  NDT2D_C_CATCH(c)
}

}  // extern "C"
