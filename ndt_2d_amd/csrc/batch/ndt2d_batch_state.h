// The state every batched device object holds beside the context (closure/, starts/, scans/,
// refine/, verify/, posegraph/): the pinned / device stage of a chunk's one upload, the block
// records, the pinned / device pair of what comes back, three timing events, the last error -- with
// its growth, release, failure and timing helpers, the timed round trip of a chunk and the grid
// installed in the context as the kernels take it.  No kernel is defined here or in what this
// includes: a unit that wants BatchHost alone compiles its own kernels only (the search engine on
// top of it is batch/ndt2d_batch_host.h).
// Included by the .hip translation units only.
#ifndef NDT2D_BATCH_STATE_H_
#define NDT2D_BATCH_STATE_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "ndt2d_hip.h"
#include "ndt2d_kernels.h"

namespace ndt2d
{

struct BatchHost
{
  ndt2d_handle h = nullptr;
  int device = 0;
  std::string err;
  // one upload per chunk (doubles), pinned and on the device
  double * h_stage = nullptr, * d_stage = nullptr;
  size_t stage_cap = 0;
  void * d_partials = nullptr;   // [slot][n_th][12] block records
  size_t partials_cap = 0;       // bytes
  // what comes back: [slot][12] records | [slot][lattice] scores (doubles), on the device and pinned
  double * d_out = nullptr, * h_out = nullptr;
  size_t out_cap = 0;
  bool timing = false;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // around the chunk's two timed phases
  bool timed = false;
};

inline void guard_note(BatchHost * s, const char * what) noexcept
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
inline void guard_note(std::nullptr_t, const char *) noexcept {}

inline int batch_fail(BatchHost * s, int code, const std::string & msg)
{
  if (s != nullptr) s->err = msg;
  return code;
}

// The end of a setter: what it refuses (a text of batch/ndt2d_refine_jobs.h's kind), or nothing.
inline int batch_refuse(BatchHost * s, const std::string & refusal)
{
  return refusal.empty() ? NDT2D_OK : batch_fail(s, NDT2D_ERR_INVALID, refusal);
}

inline int batch_fail_hip(BatchHost * s, hipError_t e, const char * what)
{
  (void)hipGetLastError();  // clear sticky state
  return batch_fail(s, NDT2D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define NDT2D_BATCH_HIP(s, call)                                         \
  do                                                                     \
  {                                                                      \
    hipError_t e__ = (call);                                             \
    if (e__ != hipSuccess) return ndt2d::batch_fail_hip(s, e__, #call);  \
  } while (0)

// Device memory of at least `bytes` at *p (contents are not kept).
inline hipError_t grow_device(void ** p, size_t * cap, size_t bytes)
{
  if (bytes <= *cap) return hipSuccess;
  if (*p != nullptr) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = bytes + bytes / 4;
  const hipError_t e = hipMalloc(p, want);
  if (e == hipSuccess) *cap = want;
  return e;
}

// A pinned / device pair of at least `doubles` (contents are not kept).
inline hipError_t grow_pair(double ** host, double ** dev, size_t * cap, size_t doubles)
{
  if (doubles <= *cap) return hipSuccess;
  *cap = 0;
  if (*host != nullptr) (void)hipHostFree(*host);
  if (*dev != nullptr) (void)hipFree(*dev);
  *host = nullptr;
  *dev = nullptr;
  const size_t want = doubles + doubles / 4 + 512;
  hipError_t e = hipHostMalloc(reinterpret_cast<void **>(host), want * sizeof(double), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(dev), want * sizeof(double));
  if (e == hipSuccess) *cap = want;
  return e;
}

// Everything BatchHost owns on the device and in pinned memory (the object itself is the caller's).
inline void batch_release(BatchHost * s)
{
  (void)hipSetDevice(s->device);
  if (s->h_stage != nullptr) (void)hipHostFree(s->h_stage);
  if (s->d_stage != nullptr) (void)hipFree(s->d_stage);
  if (s->d_partials != nullptr) (void)hipFree(s->d_partials);
  if (s->d_out != nullptr) (void)hipFree(s->d_out);
  if (s->h_out != nullptr) (void)hipHostFree(s->h_out);
  for (hipEvent_t ev : s->ev)
  {
    if (ev != nullptr) (void)hipEventDestroy(ev);
  }
}

// The body of ndt2d_<noun>_destroy: the stream is waited out first.
inline void batch_drain(BatchHost * s)
{
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(ndt2d_get_stream(s->h)));
}

// The bodies of ndt2d_<noun>_set_timing / ndt2d_<noun>_last_ms: (ev[0] -> ev[1], ev[1] -> ev[2]) of
// the last timed chunk.
inline int batch_set_timing(BatchHost * s, int enabled)
{
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (enabled != 0 && s->ev[0] == nullptr)
  {
    NDT2D_BATCH_HIP(s, hipSetDevice(s->device));
    for (hipEvent_t & ev : s->ev) NDT2D_BATCH_HIP(s, hipEventCreate(&ev));
  }
  s->timing = enabled != 0;
  s->timed = false;
  return NDT2D_OK;
}

inline int batch_last_ms(BatchHost * s, const char * noun, float * first_ms, float * second_ms)
{
  if (s == nullptr) return NDT2D_ERR_INVALID;
  if (!s->timed)
  {
    return batch_fail(s, NDT2D_ERR_STATE, std::string("ndt2d_") + noun + "_last_ms: no timed match (ndt2d_" + noun + "_set_timing)");
  }
  float a = 0.0f, b = 0.0f;
  NDT2D_BATCH_HIP(s, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
  NDT2D_BATCH_HIP(s, hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
  if (first_ms != nullptr) *first_ms = a;
  if (second_ms != nullptr) *second_ms = b;
  return NDT2D_OK;
}

// The timed round trip of a chunk whose results lie in d_out: ev[0], the chunk's launches, ev[1],
// the one read-back of total_doubles from d_out to h_out, ev[2], and the wait for the stream.
// launch() enqueues the kernels and returns NDT2D_OK or the code of what failed (its last launch's
// error is asked for here).  (The closure's and the scans' chunks place their events otherwise and
// keep their own sequence: batch_reduce_and_fetch.)
template <class LAUNCH>
int batch_round_trip(BatchHost * s, hipStream_t stream, size_t total_doubles, LAUNCH launch)
{
  s->timed = false;
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[0], stream));
  const int rc = launch();
  if (rc != NDT2D_OK) return rc;
  NDT2D_BATCH_HIP(s, hipGetLastError());
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[1], stream));
  NDT2D_BATCH_HIP(s, hipMemcpyAsync(s->h_out, s->d_out, total_doubles * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (s->timing) NDT2D_BATCH_HIP(s, hipEventRecord(s->ev[2], stream));
  NDT2D_BATCH_HIP(s, hipStreamSynchronize(stream));
  s->timed = s->timing;
  return NDT2D_OK;
}

// The grid installed in the context NOW, as the kernels take it; a list install's deferred map
// bytes are not read here and stay deferred.  *rc: NDT2D_OK, what ndt2d_grid_view_get says, or
// NDT2D_ERR_STATE for a grid without records.
inline GridDesc installed_grid(ndt2d_handle h, int * rc)
{
  GridDesc grid{};
  ndt2d_grid_view v;
  *rc = ndt2d_grid_view_get(h, &v);
  if (*rc != NDT2D_OK) return grid;
  grid.cells_global = v.cells_global;
  grid.occ_bits = v.occ_bits;
  grid.size_x = v.size_x;
  grid.size_y = v.size_y;
  grid.ncell = v.ncell;
  grid.pow2 = v.pow2;
  grid.cell_size = v.cell_size;
  grid.inv_cell_size = v.inv_cell_size;
  grid.origin_x = v.origin_x;
  grid.origin_y = v.origin_y;
  if (grid.cells_global == nullptr || grid.occ_bits == nullptr) *rc = NDT2D_ERR_STATE;
  return grid;
}

}  // namespace ndt2d

using ndt2d::guard_note;   // (NDT2D_C_CATCH of the entry points, which live outside the namespace)

#endif  // NDT2D_BATCH_STATE_H_
