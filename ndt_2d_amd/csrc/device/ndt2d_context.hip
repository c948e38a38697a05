// Device layer, the context itself: lifecycle, stream, device and pinned memory, copies, the
// timing ring and the variant switches.  No CPU compute path exists in this layer: every
// compute entry point needs the GPU.
#include <new>

#include "device/ndt2d_context.h"

using namespace ndt2d_device;

extern "C" {

int ndt2d_abi_version(void) { return NDT2D_ABI_VERSION; }

int ndt2d_create(ndt2d_handle * out, int device_id)
{
  NDT2D_C_TRY
  if (out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
  {
    (void)hipGetLastError();
    return NDT2D_ERR_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= count) return NDT2D_ERR_INVALID;
  ndt2d_context * h = new (std::nothrow) ndt2d_context();
  if (h == nullptr) return NDT2D_ERR_INVALID;
  h->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess ||
      hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
  {
    (void)hipGetLastError();
    delete h;
    return NDT2D_ERR_HIP;
  }
  h->stream = h->own_stream;
  *out = h;
  return NDT2D_OK;
  NDT2D_C_CATCH(nullptr)
}

int ndt2d_destroy(ndt2d_handle h)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (h->host_res != nullptr) (void)hipHostFree(h->host_res);
  if (h->done_words != nullptr) (void)hipFree(h->done_words);
  for (int i = 0; i < NDT2D_PIPELINE_PIECES; ++i)
  {
    if (h->pipe_up[i]) (void)hipEventDestroy(h->pipe_up[i]);
    if (h->pipe_scored[i]) (void)hipEventDestroy(h->pipe_scored[i]);
  }
  if (h->pipe_idle) (void)hipEventDestroy(h->pipe_idle);
  if (h->up_stream) (void)hipStreamDestroy(h->up_stream);
  if (h->down_stream) (void)hipStreamDestroy(h->down_stream);
  for (int i = 0; i < NDT2D_TIMING_HISTORY; ++i)
  {
    if (h->ring0[i]) (void)hipEventDestroy(h->ring0[i]);
    if (h->ring1[i]) (void)hipEventDestroy(h->ring1[i]);
  }
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;   // (its DeviceBuffer / PinnedStage members free themselves)
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

const char * ndt2d_last_error(ndt2d_handle h)
{
  return h != nullptr ? h->err.c_str() : "null handle";
}

int ndt2d_set_stream(ndt2d_handle h, void * hip_stream)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->stream = hip_stream != nullptr ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
  h->stage_cap = 0;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

void * ndt2d_get_stream(ndt2d_handle h) { return h != nullptr ? h->stream : nullptr; }

int ndt2d_device_id(ndt2d_handle h) { return h != nullptr ? h->device : -1; }

int ndt2d_device_alloc(ndt2d_handle h, size_t bytes, void ** d_out)
{
  NDT2D_C_TRY
  if (h == nullptr || d_out == nullptr) return NDT2D_ERR_INVALID;
  *d_out = nullptr;
  if (bytes == 0) return fail(h, NDT2D_ERR_INVALID, "ndt2d_device_alloc: zero size");
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_HIP(h, hipMalloc(d_out, bytes));
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_device_free(ndt2d_handle h, void * d_ptr)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (d_ptr == nullptr) return NDT2D_OK;
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_SYNC(h);  // nothing in flight may still use it
  NDT2D_HIP(h, hipFree(d_ptr));
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_copy_to_device(ndt2d_handle h, void * d_dst, const void * h_src, size_t bytes)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (bytes == 0) return NDT2D_OK;
  if (d_dst == nullptr || h_src == nullptr) return fail(h, NDT2D_ERR_INVALID, "ndt2d_copy_to_device: null pointer");
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_HIP(h, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, h->stream));
  NDT2D_SYNC(h);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_copy_to_host(ndt2d_handle h, void * h_dst, const void * d_src, size_t bytes)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (bytes == 0) return NDT2D_OK;
  if (h_dst == nullptr || d_src == nullptr) return fail(h, NDT2D_ERR_INVALID, "ndt2d_copy_to_host: null pointer");
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_HIP(h, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
  NDT2D_SYNC(h);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_copy_to_device_async(ndt2d_handle h, void * d_dst, const void * h_src, size_t bytes)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (bytes == 0) return NDT2D_OK;
  if (d_dst == nullptr || h_src == nullptr) return fail(h, NDT2D_ERR_INVALID, "ndt2d_copy_to_device_async: null pointer");
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_HIP(h, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, h->stream));
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_copy_to_host_async(ndt2d_handle h, void * h_dst, const void * d_src, size_t bytes)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  if (bytes == 0) return NDT2D_OK;
  if (h_dst == nullptr || d_src == nullptr) return fail(h, NDT2D_ERR_INVALID, "ndt2d_copy_to_host_async: null pointer");
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_HIP(h, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_set_timing(ndt2d_handle h, int enabled)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  h->timing = enabled != 0;
  if (!h->timing) h->timed = false;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_host_alloc(ndt2d_handle h, size_t bytes, void ** out)
{
  NDT2D_C_TRY
  if (h == nullptr || out == nullptr) return NDT2D_ERR_INVALID;
  *out = nullptr;
  if (bytes == 0) return fail(h, NDT2D_ERR_INVALID, "ndt2d_host_alloc: zero size");
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_HIP(h, hipHostMalloc(out, bytes, hipHostMallocMapped | hipHostMallocPortable));
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_host_free(ndt2d_handle h, void * ptr)
{
  NDT2D_C_TRY
  if (ptr == nullptr) return h != nullptr ? NDT2D_OK : NDT2D_ERR_INVALID;
  if (h == nullptr)   // the owning context is gone, and with it everything that could use ptr
  {
    const hipError_t e = hipHostFree(ptr);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess ? NDT2D_OK : NDT2D_ERR_HIP;
  }
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_SYNC(h);  // nothing in flight may still use it
  NDT2D_HIP(h, hipHostFree(ptr));
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_synchronize(ndt2d_handle h)
{
  NDT2D_C_TRY
  if (h == nullptr) return NDT2D_ERR_INVALID;
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_SYNC(h);
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_last_launch_ms(ndt2d_handle h, float * ms, int * n_kernels)
{
  NDT2D_C_TRY
  if (h == nullptr || ms == nullptr) return NDT2D_ERR_INVALID;
  if (!h->timed) return fail(h, NDT2D_ERR_STATE, "ndt2d_last_launch_ms: nothing launched");
  NDT2D_HIP(h, hipSetDevice(h->device));
  NDT2D_HIP(h, hipEventSynchronize(h->ev1));
  NDT2D_HIP(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
  if (n_kernels != nullptr) *n_kernels = h->last_kernels;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_launch_history_ms(ndt2d_handle h, float * ms_out, size_t capacity, size_t * n_out)
{
  NDT2D_C_TRY
  if (h == nullptr || n_out == nullptr || (capacity > 0 && ms_out == nullptr)) return NDT2D_ERR_INVALID;
  *n_out = 0;
  NDT2D_HIP(h, hipSetDevice(h->device));
  size_t n = static_cast<size_t>(std::min<uint64_t>(h->n_timed_launches, NDT2D_TIMING_HISTORY));
  if (n > capacity) n = capacity;
  if (n == 0) return NDT2D_OK;
  NDT2D_HIP(h, hipEventSynchronize(h->ev1));  // the newest; the stream is in order
  for (size_t k = 0; k < n; ++k)
  {
    const size_t slot = static_cast<size_t>((h->n_timed_launches - n + k) % NDT2D_TIMING_HISTORY);
    NDT2D_HIP(h, hipEventElapsedTime(&ms_out[k], h->ring0[slot], h->ring1[slot]));
  }
  *n_out = n;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

const char * ndt2d_last_variant(ndt2d_handle h) { return h != nullptr ? h->last_variant : ""; }

int ndt2d_set_pipeline_pieces(ndt2d_handle h, int pieces)
{
  NDT2D_C_TRY
  if (h == nullptr || pieces < 0 || pieces > NDT2D_PIPELINE_PIECES) return NDT2D_ERR_INVALID;
  h->pipeline_pieces = pieces;
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

int ndt2d_last_pipeline_pieces(ndt2d_handle h)
{
  NDT2D_C_TRY
  return h == nullptr ? 0 : h->last_pieces;
  NDT2D_C_CATCH(h)
}

int ndt2d_set_variant(ndt2d_handle h, const char * name)
{
  NDT2D_C_TRY
  if (h == nullptr || name == nullptr) return NDT2D_ERR_INVALID;
  h->batched_only = false;
  if (std::strcmp(name, "auto") == 0) h->force_variant = ndt2d::kVariantAuto;
  else if (std::strcmp(name, "batched") == 0) h->batched_only = true, h->force_variant = ndt2d::kVariantAuto;
  else if (std::strcmp(name, "lds") == 0) h->force_variant = ndt2d::kVariantLds;
  else if (std::strcmp(name, "global") == 0) h->force_variant = ndt2d::kVariantGlobal;
  else if (std::strcmp(name, "wave") == 0) h->force_variant = ndt2d::kVariantWave;
  else if (std::strcmp(name, "wave-lds") == 0) h->force_variant = ndt2d::kVariantWave | ndt2d::kVariantLds;
  else if (std::strcmp(name, "wave-global") == 0) h->force_variant = ndt2d::kVariantWave | ndt2d::kVariantGlobal;
  else if (std::strcmp(name, "lane") == 0) h->force_variant = ndt2d::kVariantLane;
  else if (std::strcmp(name, "lane-noskip") == 0) h->force_variant = ndt2d::kVariantLane | ndt2d::kVariantNoSkip;
  else if (std::strcmp(name, "small") == 0) h->force_variant = ndt2d::kVariantSmall;
  else if (std::strcmp(name, "small-noskip") == 0) h->force_variant = ndt2d::kVariantSmall | ndt2d::kVariantNoSkip;
  else if (std::strcmp(name, "dense") == 0) h->force_variant = ndt2d::kVariantDense;
  else if (std::strcmp(name, "compact-exact") == 0) h->force_variant = ndt2d::kVariantNoSkip;
  else return fail(h, NDT2D_ERR_INVALID, "ndt2d_set_variant: unknown variant");
  return NDT2D_OK;
  NDT2D_C_CATCH(h)
}

}  // extern "C"

#ifdef NDT2D_TEST_HOOKS
extern "C" int ndt2d_test_fail_launch(int kth)
{
  NDT2D_C_TRY
  g_test_fail_launch.store(kth);
  return 0;
  NDT2D_C_CATCH(nullptr)
}
#endif
