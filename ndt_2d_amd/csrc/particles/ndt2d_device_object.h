// The host half of an object of its own on the public device-layer calls (ndt2d_get_stream,
// ndt2d_device_id, ndt2d_device_alloc, ndt2d_host_alloc), beside the device context and without a
// field in it: ndt2d_resampler, ndt2d_seeder, ndt2d_clusterer and ndt2d_occupancy_map derive from
// DeviceObject and keep only what is their own.  Here: the handle, the device and the error text;
// guard_note (ndt2d_guard.h) for the object and for nullptr; fail / fail_hip / NDT2D_OBJ_HIP; the
// context's current stream with the wait for a stream the caller has since replaced; workspace
// carving; the grid of a grid-stride kernel; a pinned block with its device pointer.
#ifndef NDT2D_DEVICE_OBJECT_H_
#define NDT2D_DEVICE_OBJECT_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "ndt2d_hip.h"

namespace ndt2d
{
namespace object
{

constexpr uint32_t kMaxBlocks = 4096;   // grid-stride kernels

struct DeviceObject
{
  ndt2d_handle h = nullptr;
  int device = 0;
  std::string err;
  // what else a failed HIP call means for the object (the occupancy map: what was in flight may not
  // have happened), or nullptr
  void (*hip_failed)(DeviceObject *) = nullptr;
};

inline void guard_note(DeviceObject * o, const char * what) noexcept
{
  if (o == nullptr) return;
  try
  {
    o->err = what;
  }
  catch (...)
  {
  }
}
inline void guard_note(std::nullptr_t, const char *) noexcept {}

inline int fail(DeviceObject * o, int code, const char * text)
{
  guard_note(o, text);
  return code;
}

inline int fail_hip(DeviceObject * o, hipError_t e, const char * where)
{
  try
  {
    o->err = std::string(where) + ": " + hipGetErrorString(e);
  }
  catch (...)
  {
  }
  (void)hipGetLastError();
  if (o->hip_failed != nullptr) o->hip_failed(o);
  return NDT2D_ERR_HIP;
}

#define NDT2D_OBJ_HIP(obj, call)                                                           \
  do                                                                                       \
  {                                                                                        \
    const hipError_t hip_status_ = (call);                                                 \
    if (hip_status_ != hipSuccess) return ndt2d::object::fail_hip(obj, hip_status_, #call); \
  } while (0)

// The stream of an object's last launch.
struct StreamUse
{
  hipStream_t last_stream = nullptr;
  bool used = false;
};

// The context's current stream.  A caller that rebinds the context (ndt2d_set_stream) between two
// calls gets the work of the earlier stream finished first.
inline int current_stream(DeviceObject * o, StreamUse * use, hipStream_t * out)
{
  NDT2D_OBJ_HIP(o, hipSetDevice(o->device));
  hipStream_t stream = static_cast<hipStream_t>(ndt2d_get_stream(o->h));
  if (use->used && stream != use->last_stream) NDT2D_OBJ_HIP(o, hipStreamSynchronize(use->last_stream));
  use->last_stream = stream;
  use->used = true;
  *out = stream;
  return NDT2D_OK;
}

inline size_t align_up(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

// the next `count` items of a workspace, 256-byte aligned
template <typename T>
T * carve(char ** p, size_t count)
{
  T * out = reinterpret_cast<T *>(*p);
  *p += align_up(count * sizeof(T));
  return out;
}

// Room for `need` items in a block of the object's own; nothing in flight reads the old block (the
// caller has synchronised).  `refusal` is the error text of a failed allocation.
template <typename T>
int reserve(DeviceObject * o, T ** buf, size_t * cap, size_t need, const char * refusal)
{
  if (need <= *cap) return NDT2D_OK;
  if (*buf != nullptr) (void)ndt2d_device_free(o->h, *buf);
  *buf = nullptr;
  *cap = 0;
  void * p = nullptr;
  const int rc = ndt2d_device_alloc(o->h, need * sizeof(T), &p);
  if (rc != NDT2D_OK) return fail(o, rc, refusal);
  *buf = static_cast<T *>(p);
  *cap = need;
  return NDT2D_OK;
}

// the grid of a grid-stride kernel over n items: at least one block, at most kMaxBlocks
inline uint32_t stride_blocks(uint64_t n, uint32_t block)
{
  const uint64_t need = (n + block - 1) / block;
  return static_cast<uint32_t>(need < kMaxBlocks ? (need > 0 ? need : 1) : kMaxBlocks);
}

// A pinned block the kernels write through and the host reads after a synchronise.
template <typename T>
struct Pinned
{
  T * host = nullptr;
  T * dev = nullptr;   // the same block as the device sees it
};

// (an object being created: a failure is reported by its code alone)
template <typename T>
int pinned_alloc(DeviceObject * o, Pinned<T> * p)
{
  const int rc = ndt2d_host_alloc(o->h, sizeof(T), reinterpret_cast<void **>(&p->host));
  if (rc != NDT2D_OK) return rc;
  hipError_t e = hipSetDevice(o->device);
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&p->dev), p->host, 0);
  if (e == hipSuccess) return NDT2D_OK;
  (void)hipGetLastError();
  return NDT2D_ERR_HIP;
}

template <typename T>
void pinned_free(DeviceObject * o, Pinned<T> * p)
{
  if (p->host != nullptr) (void)ndt2d_host_free(o->h, p->host);
}

}  // namespace object
}  // namespace ndt2d

#endif  // NDT2D_DEVICE_OBJECT_H_
